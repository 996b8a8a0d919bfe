"""bench.py's own contract: a plain run prints the headline line only, `--full` adds the per-kernel figures, and
`--dump-outputs DIR` writes what the last timed step computed -- seeded, so that two builds can be compared file for file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _FakeContext:
    """download() as libhm_amd.Context has it: three int16 planes of a 4:2:0 picture, here seeded by the handle"""

    def __init__(self, w, h):
        self.w, self.h = w, h

    def download(self, pic):
        rng = np.random.RandomState(pic)
        return [rng.randint(0, 1024, size=s).astype(np.int16) for s in ((self.h, self.w), (self.h // 2, self.w // 2), (self.h // 2, self.w // 2))]


def test_dump_outputs_samples_within_budget_and_repeats(tmp_path):
    import bench
    ctx = _FakeContext(3840, 2160)
    pics = list(range(16))
    for d in ("a", "b"):
        bench.dump_outputs(ctx, pics, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted("pic%02d_%s.npy" % (k, c) for k in pics for c in ("y", "cb", "cr"))
    values = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b)
        values += a.size
    assert bench.DUMP_MAX_VALUES - 16 * 3 < values <= bench.DUMP_MAX_VALUES
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10 ** 6
    assert np.load(tmp_path / "a" / "pic03_y.npy").size < 3840 * 2160                # sampled, not whole


def test_dump_outputs_whole_planes_when_they_fit(tmp_path):
    import bench
    ctx = _FakeContext(416, 240)
    bench.dump_outputs(ctx, [5, 6], str(tmp_path))
    for k, pic in enumerate((5, 6)):
        planes = ctx.download(pic)
        for c, name in enumerate(("y", "cb", "cr")):
            assert np.array_equal(np.load(tmp_path / ("pic%02d_%s.npy" % (k, name))), planes[c].ravel().astype(np.float32))


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(oracle, tmp_path):
    """plain run at a small size: the headline fields and nothing measured on top; the dumped pictures are the oracle's pictures of
    the same seeded inputs (bench.py: picture k of the batch is synthetic picture k % 2, references noise / blocky planes 100 / 200)"""
    w, h, bd, nb = 416, 240, 10, 4
    out = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--width", str(w), "--height", str(h), "--batch", str(nb),
                  "--dump-outputs", str(tmp_path)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert not {"roofline", "kernels", "kernels_bi", "cpu_baseline", "host_inclusive", "hbm_copy_GBps_measured"} & set(out)
    refs = [synth.noise_planes(w, h, bd, 100), synth.blocky_planes(w, h, bd, 200)]
    for i in range(2):
        p = synth.make_picture(w, h, bd, seed=0x484D3136 + i, bi=False, ref_handles=([0], [1]))
        cur = [np.zeros_like(r) for r in refs[0]]
        oracle.decompress_ctus(p.seq, [p.slice], p.meta, p.coeffs, cur, refs)
        oracle.loop_filter_pic(p.seq, [p.slice], p.meta, p.pp, cur, 3)
        prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
        want = oracle.sao_process(p.seq, [p.slice], p.pp, p.meta, prm, cur)
        for k in range(i, nb, 2):
            for c, name in enumerate(("y", "cb", "cr")):
                got = np.load(tmp_path / ("pic%02d_%s.npy" % (k, name)))
                assert np.array_equal(got, want[c].ravel().astype(np.float32)), "picture %d plane %s" % (k, name)


@pytest.mark.gpu
def test_full_run_adds_the_per_kernel_figures():
    out = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "416", "--height", "240", "--batch", "2",
                  "--profile-steps", "1", "--no-cpu-baseline", "--full"])
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["roofline"]["kernel"] == "mc_luma" and "mc_luma" in out["kernels"] and "mc_luma" in out["kernels_bi"]
    assert "host_inclusive" in out and "hbm_copy_GBps_measured" in out
