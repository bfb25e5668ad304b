"""CPU tests of the direct solvers' size rules: SC_METHOD_FFT's transform lengths (sc_fft.hip `fft_len`, `fft_supported`) mirrored in
Python, the length classes they fall into, and SC_METHOD_AUTO's direct-solve region against them.  tests/test_gpu_direct_lengths.py
takes its sizes from these tables."""
import pytest

FFT_MAX_LOGM = 14               # sc_fft.hip: M <= 2^14 in float, 2^13 in double (16 bytes per element)


def fft_len(n):
    """(r, logM) of sc_fft.hip fft_len: the shortest M = r 2^logM >= 2n - 1 with r in {1, 3, 5}, an odd factor only in front of at
    least a 16-point power-of-two part."""
    need = max(2 * n - 1, 2)
    r, k = 1, 1
    while (r << k) < need:
        k += 1
    for rr in (3, 5):
        kk = 4
        while (rr << kk) < (r << k):
            if (rr << kk) >= need:
                r, k = rr, kk
                break
            kk += 1
    return r, k


def fft_M(n):
    r, k = fft_len(n)
    return r << k


def fft_max_M(fp64):
    return 1 << (FFT_MAX_LOGM - 1 if fp64 else FFT_MAX_LOGM)


def fft_supported(w, h, fp64):
    mx = fft_max_M(fp64)
    return w >= 1 and h >= 1 and fft_M(w) <= mx and fft_M(h) <= mx


def length_classes(fp64):
    """[(M, r, n_lo, n_hi)]: every transform length the precision supports with the unknown counts that take it, in order."""
    out = []
    n = 1
    while fft_M(n) <= fft_max_M(fp64):
        r, k = fft_len(n)
        M = r << k
        if out and out[-1][0] == M:
            out[-1][3] = n
        else:
            out.append([M, r, n, n])
        n += 1
    return [tuple(c) for c in out]


def dst_padded_half(n):
    """sc_dst.hip dst_prepare: the parity fold's half size m = ceil(n / 2), padded to the 128-row tile."""
    m = (n + 1) // 2
    return (m + 127) // 128 * 128


@pytest.mark.parametrize("fp64", [False, True])
def test_length_classes_tile_every_supported_size(fp64):
    cls = length_classes(fp64)
    top = 4096 if fp64 else 8192
    assert cls[0][2] == 1 and cls[-1][3] == top and cls[-1][0] == fft_max_M(fp64)
    for a, b in zip(cls, cls[1:]):
        assert b[2] == a[3] + 1 and b[0] > a[0], (a, b)              # no gap, no overlap, lengths grow
        assert a[0] < 2 * b[2] - 1, (a, b)                          # the shorter length would wrap at the next class's n_lo
    for M, r, lo, hi in cls:
        assert lo <= hi and M >= 2 * hi - 1, (M, lo, hi)            # the circular convolution does not wrap at the tight end
        assert M % r == 0 and ((M // r) & (M // r - 1)) == 0
        assert r == 1 or M // r >= 16
    assert {c[1] for c in cls} == {1, 3, 5}
    assert not fft_supported(top + 1, 9, fp64) and not fft_supported(9, top + 1, fp64)
    assert fft_supported(top, 9, fp64) and fft_supported(9, top, fp64)
    if fp64:
        assert [c[0] for c in cls][-3:] == [5120, 6144, 8192]
    else:
        assert [c[0] for c in cls][-4:] == [8192, 10240, 12288, 16384]
        assert len(cls) == len(length_classes(True)) + 3


def test_every_size_auto_solves_directly_is_supported_in_double():
    from seamlesscloneoptimization_amd import capi
    D, A, N, L = capi.SC_AUTO_DIRECT_MAX, capi.SC_AUTO_DIRECT_AREA, capi.SC_AUTO_NARROW_MAX, capi.SC_AUTO_THIN_LONG_MAX
    assert L == length_classes(True)[-1][3]
    edges = sorted({1, 2, 4, 5, D - 1, D, D + 1, N - 1, N, N + 1, A // L, A // L + 1, L - 1, L, L + 1, 2 * L} |
                   {A // k + d for k in (N + 1, 200, 300, 500, D + 1) for d in (-1, 0, 1)} | {c[3] for c in length_classes(True)})
    seen = {True: 0, False: 0}
    for w in edges:
        for h in edges:
            direct = capi.auto_takes_direct(w, h)
            seen[direct] += 1
            if direct:
                assert fft_supported(w, h, True), (w, h)
    assert seen[True] and seen[False]
    # the rule's own boundaries, one unknown either side
    assert capi.auto_takes_direct(D, D) and not capi.auto_takes_direct(D + 1, D + 1)
    assert capi.auto_takes_direct(L, N) and capi.auto_takes_direct(N, L)
    assert not capi.auto_takes_direct(L + 1, N) and not capi.auto_takes_direct(N, L + 1) and not capi.auto_takes_direct(L + 1, 1)
    assert not capi.auto_takes_direct(L, N + 1)                                        # 4096 x 141 > the area rule
    assert capi.auto_takes_direct(A // (N + 1), N + 1) and not capi.auto_takes_direct(A // (N + 1) + 1, N + 1)
    assert capi.auto_takes_direct(2598, 168) and capi.auto_takes_direct(168, 2598)   # the area rule at 170 pixels across


def test_dst_padding_changes():
    """The padded half size of SC_METHOD_DST changes where m = ceil(n / 2) crosses a multiple of 128: n = 256 | 257, 512 | 513, ..."""
    steps = [n for n in range(2, 1101) if dst_padded_half(n) != dst_padded_half(n - 1)]
    assert steps == [257, 513, 769, 1025]
    assert [dst_padded_half(n) for n in (255, 256, 257, 258)] == [128, 128, 256, 256]
