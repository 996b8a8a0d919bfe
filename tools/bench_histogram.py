"""Times the picture histograms (hmgpu_pictures_histogram) on one GPU: sixteen 3840x2160 4:2:0 10-bit pictures, on
natural-like content (piecewise ramps plus noise: hundreds of occupied bins) and on flat pictures (every sample of a plane equal: all
64 lanes of a wave add to one LDS word) --
  (a) Y + Cb + Cr full-depth histograms, (b) the records alone, (c) Y + maxRGB --
beside the yardsticks on the same pictures: hmgpu_pictures_metrics picture against picture without SSIM (it reads twice the bytes), and
what a user had before the call existed: export_batch to planar uint16 tensors plus torch.bincount per plane and picture.  Device
time per call from torch events around K back-to-back calls on torch's current stream, the cases alternating in one process, R rounds
after one that warms up; prints one JSON line and writes it to --out.  Kernel times come from a run of their own under rocprofv3
--kernel-trace --stats (the kernels are k_histogram<maxrgb>).

    python tools/bench_histogram.py [--rounds 5] [--calls 20] [--out profiles/histogram_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libhm_amd
    from libhm_amd import abi, histogram
    from tests import histogram_ref as href
    from tests import synth
    w, h, n, bd = a.width, a.height, 16, 10
    seq = abi.make_seq(w, h, bd, bd, max_pictures=2 * n + 2)
    rng = np.random.RandomState(11)
    natural = []
    for i in range(4):
        planes = synth.smooth_planes(w, h, bd, 20 + i, 1, bd)
        natural.append([np.clip(p.astype(np.int32) + rng.randint(-100, 101, size=p.shape), 0, (1 << bd) - 1).astype(np.int16) for p in planes])
    flat = [[np.full((h >> s, w >> s), v, dtype=np.int16) for s, v in ((0, 64 + 200 * i), (1, 512), (1, 512))] for i in range(4)]
    with libhm_amd.Context(seq) as ctx:
        sets = {}
        for key, src in (("natural", natural), ("flat", flat)):
            sets[key] = []
            for i in range(n):
                hnd = ctx.acquire()
                ctx.upload(hnd, src[i % 4])
                sets[key].append(hnd)
        ctx.sync()
        # one picture of each content against the model, so that what is timed is known to be right
        coef = list(libhm_amd.histogram_plan(seq, ("maxrgb",)).coef)
        for key, src in (("natural", natural), ("flat", flat)):
            out = ctx.histogram(sets[key][:1], channels=("y", "cb", "cr", "maxrgb"))
            want = href.picture(src[0], 1, (bd, bd), (0, 1, 2, 3), coef=coef)
            for c, name in enumerate(href.NAMES):
                assert np.array_equal(out[name]["hist"][0].cpu().numpy().astype(np.int64), want[c]["hist"]), (key, name)
                assert all(int(out[name][f][0]) == want[c][f] for f in href.FIELDS), (key, name)
        occupied = int((ctx.histogram(sets["natural"][:1])["y"]["hist"][0] > 0).sum())
        planar = {key: ctx.export_batch(sets[key], "planar", bd) for key in sets}

        def before(key):
            planes = ctx.export_batch(sets[key], "planar", bd, out=planar[key])
            # (2-byte elements through int16: the values are below 2^15, and torch.uint16 has few ops)
            return [torch.stack([torch.bincount(p[i].reshape(-1).view(torch.int16).to(torch.int64), minlength=1 << bd) for i in range(n)])
                    for p in planes]
        got = before("natural")
        full = ctx.histogram(sets["natural"])
        for c, name in enumerate(("y", "cb", "cr")):
            assert torch.equal(got[c], full[name]["hist"].long())              # the two ways agree on all 48 histograms
        other = list(reversed(sets["natural"]))
        cases = {}
        for key in ("natural", "flat"):
            pics = sets[key]
            cases["a_ycbcr_hist_" + key] = lambda pics=pics: ctx.histogram(pics)
            cases["b_ycbcr_records_" + key] = lambda pics=pics: ctx.histogram(pics, histogram=False)
            cases["c_y_maxrgb_hist_" + key] = lambda pics=pics: ctx.histogram(pics, channels=("y", "maxrgb"))
            cases["before_export_planar_and_bincount_" + key] = lambda key=key: before(key)
        cases["metrics_pictures_no_ssim_natural"] = lambda: ctx.metrics(sets["natural"], ref_pics=other, ssim=False)
        cases["metrics_pictures_no_ssim_flat"] = lambda: ctx.metrics(sets["flat"], ref_pics=list(reversed(sets["flat"])), ssim=False)
        times = {k: [] for k in cases}
        for rnd in range(a.rounds + 1):
            for name, fn in cases.items():
                calls = max(1, a.calls // 10) if name.startswith("before") else a.calls
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:                                                  # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / calls)
        # algorithmic bytes per call: 2 bytes per sample read; 4:2:0 has 1.5 samples per luma sample.  (a), (b): every plane once;
        # (c): luma once and the chroma of every luma sample, which is the pair plane once (each pair serves four luma samples from
        # the caches); metrics: both pictures.  The histograms and records written are at most 16 x 3 x 4 KiB.
        luma = n * w * h
        nbytes = {"a_": luma * 3, "b_": luma * 3, "c_": luma * 3, "me": luma * 6}
        res = {"pictures": n, "width": w, "height": h, "bit_depth": bd, "rounds": a.rounds, "calls_per_round": a.calls,
               "occupied_luma_bins_natural": occupied, "device": torch.cuda.get_device_name(0), "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            nb = nbytes.get(name[:2])
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": nb,
                                  "GBps": None if nb is None else round(nb / (med * 1e-6) / 1e9, 1)}
        for v in ("a_ycbcr_hist", "b_ycbcr_records", "c_y_maxrgb_hist"):
            res["cases"][v + "_flat"]["flat_to_natural"] = round(res["cases"][v + "_flat"]["us_per_call_median"] /
                                                                 res["cases"][v + "_natural"]["us_per_call_median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
