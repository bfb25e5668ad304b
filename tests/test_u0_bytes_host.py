"""The fetch rule of the first level-0 launch that reads a group's initial field from the members' destination bytes (k_cycle0 with
C0_IN3; csrc/sc_u0_bytes.h), walked on the host: sc_hip_u0_bytes_fetch runs the kernel's own __host__ __device__ functions on a row in
host memory and says which dwords it read.  No GPU.

Every ROI width from 3 to 600, every alignment of the row's first byte, every channel, every lane of the first, a middle and the last
column tile (a tile owns 232 columns, its wave starts 12 columns to the left of them):
 - a dword is read only if it holds at least one byte of the row [row, row + 3 W) -- so nothing more than 3 bytes outside it -- and
   every dword is 4-byte aligned;
 - a wave takes the unguarded 16-byte load only where all four of every lane's dwords pass that same rule;
 - the four values are the row's bytes of that channel at the lane's columns (clamped into [0, W] as the kernel clamps), and 0 for a
   column at or beyond W, which is what the float16 planes held there."""
import numpy as np

from seamlesscloneoptimization_amd import capi

LEAD = 8      # bytes in front of the row inside the buffer (a multiple of 4: the buffer itself is aligned)


def test_every_width_alignment_channel_and_lane():
    rng = np.random.default_rng(5)
    lanes = np.arange(64)
    unguarded_waves = 0
    for W in range(3, 601):
        nbx = (W + 231) // 232
        for al in range(4):
            raw = np.zeros(LEAD + al + 3 * W + 16 + 64, np.uint8)
            start = (-raw.ctypes.data) % 64      # a 64-byte aligned base inside the array
            buf = raw[start:]
            buf[:] = rng.integers(1, 256, buf.size, dtype=np.uint8)      # never 0: a value of 0 is a statement about W
            off = LEAD + al
            row = buf[off:off + 3 * W]
            assert (buf.ctypes.data + off) % 4 == al
            for bx in sorted({0, nbx // 2, nbx - 1}):
                xw = bx * 232 - 12
                o = capi.u0_bytes_fetch(buf, off, W, xw)
                q, shift, mask, whole = o[:, 0], o[:, 1], o[:, 2], o[:, 3]
                assert np.all((q + off) % 4 == 0) and np.all((shift >= 0) & (shift <= 3))
                xc = np.clip(xw + 4 * lanes, 0, W)
                assert np.array_equal(q + shift, 3 * xc)           # the first dword is the one at or below the lane's first byte
                d = q[:, None] + 4 * np.arange(4)[None, :]         # offsets of the four dwords from the row
                read = (mask[:, None] >> np.arange(4)[None, :]) & 1 == 1
                in_row = (d + 3 >= 0) & (d < 3 * W)
                assert np.all(in_row[read]), (W, al, bx)
                assert np.all(d[read] >= -3) and np.all(d[read] + 3 <= 3 * W + 2)
                assert np.array_equal(read, in_row)               # ... and every dword the rule admits is read: no value is lost
                assert len(set(whole)) == 1
                if whole[0]:
                    unguarded_waves += 1
                    assert np.all(mask == 15) and np.all(in_row)
                cols = xc[:, None] + np.arange(4)[None, :]
                for ci in range(3):
                    vals = o[:, 4 + 4 * ci:8 + 4 * ci]
                    want = np.where(cols < W, row[np.minimum(3 * cols + ci, 3 * W - 1)], 0)
                    assert np.array_equal(vals, want), (W, al, bx, ci)
                    assert np.all(vals[cols >= W] == 0) and np.all(vals[cols < W] > 0)
    assert unguarded_waves > 0      # (widths from 262 on have a wave strictly inside: the middle tile of three, or the first of two shifted)
