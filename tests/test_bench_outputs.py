"""bench.py --dump-outputs: what the timed path returned in its last step, as .npy files two builds can compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 64 << 20


def _load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_format_budget_and_seeded_sample(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (700, 650, 3), dtype=np.uint8) for _ in range(5)]
    n = 80                                                      # more images than fit whole: a sample
    r = bench.dump_outputs(str(tmp_path / "a"), lambda k: imgs[k % 5], n, imgs[0].shape, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), lambda k: imgs[k % 5], n, imgs[0].shape, 0, 1)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert sorted(a) == ["clone_channel_sums", "clone_samples", "sample_yx"] and r["files"] == [k + ".npy" for k in sorted(a)]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in r["files"]) <= LIMIT
    S = r["pixels_sampled_per_image"]
    assert 0 < S < 700 * 650 and a["clone_samples"].shape == (n, S, 3) and a["sample_yx"].shape == (S, 2)
    assert all(np.array_equal(a[k], b[k]) for k in a)          # same arguments, same positions, same file
    ys, xs = a["sample_yx"][:, 0].astype(int), a["sample_yx"][:, 1].astype(int)
    assert len(set(zip(ys.tolist(), xs.tolist()))) == S
    for k in (0, 1, 79):
        assert np.array_equal(a["clone_samples"][k], imgs[k % 5][ys, xs, :].astype(np.float32))
        assert np.array_equal(a["clone_channel_sums"][k], imgs[k % 5].reshape(-1, 3).sum(axis=0).astype(np.float64))
    # a batch that fits: every pixel; N ranks: each its own files, names suffixed, within budget / N
    r = bench.dump_outputs(str(tmp_path / "c"), lambda k: imgs[k], 2, imgs[0].shape, 1, 2)
    c = _load_dir(tmp_path / "c")
    assert sorted(c) == ["clone_channel_sums_rank1", "clone_samples_rank1", "sample_yx_rank1"]
    assert r["pixels_sampled_per_image"] == 700 * 650
    assert np.array_equal(c["clone_samples_rank1"][1].reshape(700, 650, 3), imgs[1].astype(np.float32))


def test_bench_rejects_zero_steps_and_dump_with_reference_table():
    import bench
    assert bench.parse_args(["--steps", "3", "--dump-outputs", "d"]).steps == 3
    for argv in (["--steps", "0"], ["--reference-table", "--dump-outputs", "d"]):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)


@pytest.mark.gpu
def test_bench_dump_outputs_is_the_clone_and_repeats(tmp_path):
    """Two runs with the same arguments: the timed step count is --steps, the files stay under 64 MB, the two runs' dumps agree, and
    image 0 (synth(roi, 0), the SURVEY 8d image) is the clone the float-table C oracle computes, within one grey level."""
    import bench
    from oracle import oracle_c as oc
    roi, steps = 256, 3
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--roi", str(roi), "--batch", "4", "--steps", str(steps),
                            "--warmup", "1", "--cpu-seconds", "0", "--kernel-launches", "4", "--host-calls", "3", "--no-float32-leg",
                            "--no-fresh-leg", "--no-c5-projection", "--no-mixed-sizes", "--no-new-size", "--no-c4",
                            "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert d["steps"] == steps and d["ms_per_step"] > 0
        assert abs(d["per_rank"]["elapsed_ms"][0] - d["ms_per_step"] * steps) < 1e-2 * d["per_rank"]["elapsed_ms"][0] + 0.05
        assert d["dump_outputs"]["images"] == 4
        assert sum(os.path.getsize(tmp_path / name / f) for f in d["dump_outputs"]["files"]) <= LIMIT
        runs.append(_load_dir(tmp_path / name))
    a, b = runs
    assert np.array_equal(a["sample_yx"], b["sample_yx"])
    assert np.abs(a["clone_samples"] - b["clone_samples"]).max() <= 1
    dst, patch, mask, cx, cy = bench.synth(roi, 0)
    want = oc.seamless_clone(dst, patch, mask, cx, cy, exact_den=False)
    ys, xs = a["sample_yx"][:, 0].astype(int), a["sample_yx"][:, 1].astype(int)
    got = a["clone_samples"][0]
    assert np.abs(got - want[ys, xs, :].astype(np.float32)).max() <= 1
    assert not np.array_equal(got, dst[ys, xs, :].astype(np.float32))            # the clone changed the destination
    assert a["clone_channel_sums"].shape == (4, 3) and len({tuple(s) for s in a["clone_channel_sums"]}) == 4    # four different images
