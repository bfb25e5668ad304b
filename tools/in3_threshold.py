"""Where does the first level-0 launch that reads the members' destination bytes itself (k_cycle0 with C0_IN3, no float16 initial field
stored by the pre-process) beat the float16 planes?  Same-size groups of 2, 4, 8 and 16 members at 512^2, 1024^2 and 2048^2 through the
pool as the bench runs them (two streams, one group each), both readers alternating in ONE process: ms per step, best and median of
the repetitions, and members x level-0 tiles of a group.
    python tools/in3_threshold.py [steps] > profiles/in3_threshold.txt
The rule (csrc/sc_instance.h, SC_IN3_MIN_TILES) puts the cut where the new form is no slower than the old beyond the runs' spread."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
from seamlesscloneoptimization_amd import capi
import bench

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
REPS = 5
VARIANTS = (("planes", capi.SC_LEGACY_U0_PLANES), ("bytes", capi.SC_FORCE_U0_BYTES))
print("roi members tiles(members x level-0 tiles) reader best_ms median_ms spread_ms | bytes - planes (median) ms, %", flush=True)
for roi in (512, 1024, 2048):
    gen = bench.BatchSynth(roi, 1001)
    imgs = [gen.image(b) for b in range(32)]
    for group in (2, 4, 8, 16):
        batch = 2 * group
        pool = capi.Pool(0, 2, group=group, method=capi.SC_METHOD_MULTIGRID)
        inst = pool.instances[0]
        cjobs = pool.make_jobs(batch)
        held = []
        for b in range(batch):
            dst, patch, mask, cx, cy = imgs[b]
            c = cjobs[b]
            c.face, c.face_cols, c.face_rows, c.face_step = inst.to_device(patch), patch.shape[1], patch.shape[0], 3 * patch.shape[1]
            c.body, c.body_cols, c.body_rows, c.body_step = inst.to_device(dst), dst.shape[1], dst.shape[0], 3 * dst.shape[1]
            c.mask, c.mask_cols, c.mask_rows, c.mask_step = inst.to_device(mask), mask.shape[1], mask.shape[0], mask.shape[1]
            c.centerX, c.centerY, c.body_restore = cx, cy, inst.to_device(dst)
            held += [c.face, c.body, c.mask, c.body_restore]
        times = {name: [] for name, _ in VARIANTS}
        for rep in range(REPS):
            for name, bit in (VARIANTS if rep % 2 == 0 else VARIANTS[::-1]):
                o = inst.get_solver()
                o.flags, o.legacy_paths = capi.SC_FLAG_LEGACY_PATHS, bit
                assert pool.L.sc_hip_pool_set_solver(pool.h, C.byref(o)) == 0
                for i in pool.instances:
                    i.u0_reader()
                for _ in range(3):
                    pool.run(cjobs, device_resident=True)
                t0 = time.perf_counter()
                for _ in range(steps):
                    pool.run(cjobs, device_resident=True)
                times[name].append((time.perf_counter() - t0) / steps * 1e3)
                seen = {i.u0_reader() for i in pool.instances} - {0}
                assert seen == {2 if name == "bytes" else 1}, (name, seen)
        tiles = group * ((roi + 231) // 232) * ((roi + 51) // 52)
        med = {}
        for name, _ in VARIANTS:
            t = sorted(times[name])
            med[name] = t[len(t) // 2]
            print("%d %d %d %s %.4f %.4f %.4f" % (roi, group, tiles, name, t[0], med[name], t[-1] - t[0]), flush=True)
        d = med["bytes"] - med["planes"]
        print("%d %d %d | %+.4f ms %+.2f %%" % (roi, group, tiles, d, 100.0 * d / med["planes"]), flush=True)
        for p in held:
            inst.free(p)
        pool.close()
