// sc_u0_bytes.h -- the initial field of a group clone read from the destination's own bytes (k_cycle0 with C0_IN3, sc_cycle0.hip).
//
// The three channels of ROI pixels x .. x + 3 (x a multiple of 4) of one row are the twelve bytes from byte 3 x of the interleaved row: four
// dwords from the 4-byte boundary at or below it hold them all, v_alignbyte_b32 with the shift row & 3 -- 3 x is a multiple of 4, so the
// shift is the same for every lane of a row -- puts them at fixed byte positions of three words, which are then sorted by channel.
// WHICH dwords may be fetched is the pre-process's rule (p4_stage, sc_kernels.hip): a dword only if it holds at least one byte of the
// ROI's row [row, row + 3 W), so nothing is read more than 3 bytes outside that row; the others count as 0.  One definition for the
// kernel, the host walk of tests/test_u0_bytes_host.py (sc_hip_u0_bytes_fetch) and the stand-alone sanitizer program.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace sc {

struct __attribute__((aligned(4))) U0Quad { unsigned d[4]; };

// the dword at address d holds a byte of the ROI row that starts at `row` and is W pixels long
__host__ __device__ __forceinline__ bool u0_dword_in_row(uintptr_t d, uintptr_t row, int W) { return d + 3 >= row && d < row + 3 * (uintptr_t)W; }
// a wave whose lane 0 serves column xw takes the unguarded 16-byte load: all its columns x lie in [4, W - 5], so its first dword starts
// at least 3 x - 3 >= 9 bytes inside the row and its last one at most 3 x + 2 + 12 <= 3 W - 1 (u0_dword_in_row holds for all four)
__host__ __device__ __forceinline__ bool u0_wave_unguarded(int xw, int W) { return xw >= 4 && xw + 255 <= W - 2; }
// the column whose bytes a lane at column x fetches: clamped like the planes' loads (c0_load), no further than the row's end
__host__ __device__ __forceinline__ int u0_clamp_x(int x, int W) { return x < 0 ? 0 : x > W ? W : x; }
// offset in the row of the 4-byte boundary at or below the first byte of the lane's window (channel 0 of pixel xc), and the
// re-alignment shift (the same for every lane of a row whose columns are multiples of 4)
__host__ __device__ __forceinline__ int u0_first_dword(const uint8_t *row, int xc, int &shift)
{
    shift = (int)(((uintptr_t)row + 3 * (uintptr_t)xc) & 3);
    return 3 * xc - shift;
}
__host__ __device__ __forceinline__ unsigned u0_alignbyte(unsigned hi, unsigned lo, int shift)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)shift);
#else
    return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * shift));
#endif
}
// the guarded fetch: dword k of the window at row + q if the rule admits it, else 0.  Every load is issued -- a refused dword's load
// goes to the dword that holds the row's first byte, which the rule admits -- so the loads of a lane's rows leave together, not one
// branch region after the other (see c0_load).  fetched: bit k set where dword k itself was read.
__host__ __device__ __forceinline__ U0Quad u0_fetch_guarded(const uint8_t *__restrict__ row, int W, int q, unsigned &fetched)
{
    U0Quad v;
    fetched = 0u;
    const int first = -(int)((uintptr_t)row & 3);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = u0_dword_in_row((uintptr_t)row + (intptr_t)(q + 4 * k), (uintptr_t)row, W);
        const unsigned w = *reinterpret_cast<const unsigned *>(row + (ok ? q + 4 * k : first));
        v.d[k] = ok ? w : 0u;
        fetched |= ok ? 1u << k : 0u;
    }
    return v;
}
__host__ __device__ __forceinline__ U0Quad u0_fetch_unguarded(const uint8_t *__restrict__ row, int q) { return *reinterpret_cast<const U0Quad *>(row + q); }
// the window's twelve bytes -- four pixels of three channels -- re-aligned, as one word per CHANNEL: byte j of word c is channel c of pixel j
__host__ __device__ __forceinline__ void u0_channels(const U0Quad &v, int shift, unsigned (&ch)[3])
{
    const unsigned w0 = u0_alignbyte(v.d[1], v.d[0], shift), w1 = u0_alignbyte(v.d[2], v.d[1], shift), w2 = u0_alignbyte(v.d[3], v.d[2], shift);
    ch[0] = (w0 & 0xffu) | ((w0 >> 24) << 8) | (((w1 >> 16) & 0xffu) << 16) | (((w2 >> 8) & 0xffu) << 24);
    ch[1] = ((w0 >> 8) & 0xffu) | ((w1 & 0xffu) << 8) | ((w1 >> 24) << 16) | (((w2 >> 16) & 0xffu) << 24);
    ch[2] = ((w0 >> 16) & 0xffu) | (((w1 >> 8) & 0xffu) << 8) | ((w2 & 0xffu) << 16) | ((w2 >> 24) << 24);
}
// the four values of one channel's word: the 8-bit value as float, 0 for a column at or beyond W (what the float16 planes held there)
__host__ __device__ __forceinline__ void u0_values(unsigned word, int xc, int W, float (&out)[4])
{
    out[0] = xc + 0 < W ? (float)(word & 0xffu) : 0.f;
    out[1] = xc + 1 < W ? (float)((word >> 8) & 0xffu) : 0.f;
    out[2] = xc + 2 < W ? (float)((word >> 16) & 0xffu) : 0.f;
    out[3] = xc + 3 < W ? (float)(word >> 24) : 0.f;
}

} // namespace sc
