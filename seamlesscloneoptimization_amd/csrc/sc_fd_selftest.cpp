// sc_fd_selftest.cpp -- the host eigen-solver of a level's 1-D operators and the two checks sc_hip_selftest_host makes with it: of
// the decomposition itself, and of the closed form the device builds the bottom's matrices from (sc_fd_closed.h, k_fd_build).
// Nothing else calls into this file.
#include "sc_instance.h"
#include "sc_fd_closed.h"
#include <algorithm>
#include <cmath>

namespace sc {

// ---------------------------------------------------------------------------------------------
// Direct solve of the bottom's first level(s) by fast diagonalisation.
// A level's operator is  (A u)[y][x] = sum_x' Tx[x][x'] u[y][x'] + sum_y' Ty[y][y'] u[y'][x]  with
// tridiagonal 1-D parts: rows (1, -2, 1), last row (cw_last, -d_last) (MGDim).  T is not symmetric
// (the last sub-diagonal is cw_last, the super-diagonal above it 1) but E T E^-1 is, with
// E = diag(1, .., 1, 1/sqrt(cw_last)); its eigen-decomposition Q L Q^T gives T = V L V^-1 with
// V = E^-1 Q, V^-1 = Q^T E.  Everything here is double; the device gets float matrices.
// ---------------------------------------------------------------------------------------------
// Eigen-decomposition of a symmetric tridiagonal matrix by implicit QL with Wilkinson shifts.
// d: diagonal (n) -> eigenvalues; e: sub-diagonal, e[i] couples i and i+1 (n-1 used, e[n-1] = 0);
// zt: n x n, row k = eigenvector k on return (kept transposed so the rotation loop is contiguous).
static bool tridiag_ql(int n, std::vector<double> &d, std::vector<double> &e, std::vector<double> &zt)
{
    zt.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) zt[(size_t)i * n + i] = 1.0;
    for (int l = 0; l < n; ++l) {
        int iter = 0, m;
        do {
            for (m = l; m < n - 1; ++m) {
                const double dd = std::fabs(d[m]) + std::fabs(d[m + 1]);
                if (std::fabs(e[m]) <= 1.1e-16 * dd) break;
            }
            if (m != l) {
                if (++iter > 80) return false;
                double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
                double r = std::hypot(g, 1.0);
                g = d[m] - d[l] + e[l] / (g + (g >= 0.0 ? std::fabs(r) : -std::fabs(r)));
                double s = 1.0, c = 1.0, p = 0.0;
                int i;
                for (i = m - 1; i >= l; --i) {
                    double f = s * e[i];
                    const double b = c * e[i];
                    r = std::hypot(f, g);
                    e[i + 1] = r;
                    if (r == 0.0) { d[i + 1] -= p; e[m] = 0.0; break; }
                    s = f / r; c = g / r;
                    g = d[i + 1] - p;
                    r = (d[i] - g) * s + 2.0 * c * b;
                    p = s * r;
                    d[i + 1] = g + p;
                    g = c * r - b;
                    double *zi = &zt[(size_t)i * n], *zi1 = &zt[(size_t)(i + 1) * n];
                    for (int k = 0; k < n; ++k) {
                        f = zi1[k];
                        zi1[k] = s * zi[k] + c * f;
                        zi[k] = c * zi[k] - s * f;
                    }
                }
                if (r == 0.0 && i >= l) continue;
                d[l] -= p; e[l] = g; e[m] = 0.0;
            }
        } while (m != l);
    }
    return true;
}

static bool fd_decompose(const MGDim &g, FD1 &o)
{
    const int n = g.n;
    o.n = n; o.cw_last = g.cw_last; o.d_last = g.d_last;
    o.ee.assign(n, 1.0);
    std::vector<double> d(n, -2.0), e(n, 0.0);
    for (int i = 0; i + 1 < n; ++i) e[i] = 1.0;
    d[n - 1] = -(double)g.d_last;
    if (n >= 2) {
        e[n - 2] = std::sqrt((double)g.cw_last);          // sqrt(sub * super) = sqrt(cw_last * 1)
        o.ee[n - 1] = 1.0 / std::sqrt((double)g.cw_last);
    }
    if (!tridiag_ql(n, d, e, o.q)) return false;
    o.lam = d;
    return true;
}

// host-only check of the decomposition (sc_hip_selftest_host): max |T v_k - l_k v_k| and max |V^-1 V - I| over a few
// level operators, regular and with an irregular last interval
double fd_selftest_error()
{
    double worst = 0.0;
    const int ns[] = { 1, 2, 3, 7, 31, 63, 74, 128 };
    const double alphas[] = { 1.0, 0.5, 0.75, 1.5, 0.96875 };
    for (int n : ns)
        for (double a : alphas) {
            MGDim g = make_dim(n, a, 0);
            FD1 f;
            if (!fd_decompose(g, f)) return 1e30;
            auto T = [&](int i, int j) -> double {          // the level operator itself
                if (i == j) return i == n - 1 ? -(double)g.d_last : -2.0;
                if (j == i + 1) return 1.0;
                if (j == i - 1) return i == n - 1 ? (double)g.cw_last : 1.0;
                return 0.0;
            };
            for (int k = 0; k < n; ++k) {
                for (int i = 0; i < n; ++i) {
                    double tv = 0.0;
                    for (int j = std::max(0, i - 1); j <= std::min(n - 1, i + 1); ++j) tv += T(i, j) * f.q[(size_t)k * n + j] / f.ee[j];
                    worst = std::max(worst, std::fabs(tv - f.lam[k] * f.q[(size_t)k * n + i] / f.ee[i]));
                }
                for (int m = 0; m < n; ++m) {                // rows of V^-1 = Q^T E against columns of V = E^-1 Q
                    double dot = 0.0;
                    for (int i = 0; i < n; ++i) dot += f.q[(size_t)k * n + i] * f.ee[i] * f.q[(size_t)m * n + i] / f.ee[i];
                    worst = std::max(worst, std::fabs(dot - (k == m ? 1.0 : 0.0)));
                }
            }
        }
    return worst;
}

// host-only check of the closed form (sc_hip_selftest_host): its matrices V, V^-1 and eigenvalues against the QL-based
// decomposition over level operators of every size the bottom solve can meet, regular and with an irregular last interval
// on either side of the alpha = 0.7071 threshold (one eigenvalue below -4).  Returns the worst deviation found.
double fd_closed_selftest_error()
{
    double worst = 0.0;
    const double alphas[] = { 1.0, 0.5, 0.625, 0.70703125, 0.7109375, 0.75, 0.875, 1.125, 1.25, 1.5, 0.96875 };
    for (int n = 1; n <= 128; n += (n < 20 ? 1 : 9))
        for (double a : alphas) {
            MGDim g = make_dim(n, a, 0);
            FD1 f;
            if (!fd_decompose(g, f)) return 1e30;
            std::vector<FdPair> p(n);
            for (int k = 0; k < n; ++k) p[k] = fd_pair(k, n, (double)g.cw_last, (double)g.d_last);
            // eigenvalues: the two sets must agree as sets (QL's order is arbitrary)
            std::vector<double> la(f.lam), lb(n);
            for (int k = 0; k < n; ++k) lb[k] = p[k].lam;
            std::sort(la.begin(), la.end()); std::sort(lb.begin(), lb.end());
            for (int k = 0; k < n; ++k) worst = std::max(worst, std::fabs(la[k] - lb[k]));
            // T v = lambda v for the closed form's own vectors, and V^-1 V = I
            auto T = [&](int i, int j) -> double {
                if (i == j) return i == n - 1 ? -(double)g.d_last : -2.0;
                if (j == i + 1) return 1.0;
                if (j == i - 1) return i == n - 1 ? (double)g.cw_last : 1.0;
                return 0.0;
            };
            std::vector<double> V((size_t)n * n), Vi((size_t)n * n);      // V[x][k], Vinv[k][x]
            for (int k = 0; k < n; ++k)
                for (int x = 0; x < n; ++x) {
                    const double v = fd_component(p[k], x + 1, n) * p[k].inv_norm;
                    V[(size_t)x * n + k] = v;
                    Vi[(size_t)k * n + x] = v * (x == n - 1 ? 1.0 / (double)g.cw_last : 1.0);
                }
            for (int k = 0; k < n; ++k) {
                for (int i = 0; i < n; ++i) {
                    double tv = 0.0;
                    for (int j = std::max(0, i - 1); j <= std::min(n - 1, i + 1); ++j) tv += T(i, j) * V[(size_t)j * n + k];
                    worst = std::max(worst, std::fabs(tv - p[k].lam * V[(size_t)i * n + k]));
                }
                for (int m = 0; m < n; ++m) {
                    double dot = 0.0;
                    for (int x = 0; x < n; ++x) dot += Vi[(size_t)k * n + x] * V[(size_t)x * n + m];
                    worst = std::max(worst, std::fabs(dot - (k == m ? 1.0 : 0.0)));
                }
            }
        }
    return worst;
}

} // namespace sc
