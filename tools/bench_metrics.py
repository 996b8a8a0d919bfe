"""Times the picture metrics (hmgpu_pictures_metrics) on one GPU: sixteen 3840x2160 4:2:0 10-bit pictures against
sixteen other pictures of the context and against uint16 planes, with SSIM and without, beside what a user had before the call
existed: export_batch of both sets to planar uint16 tensors plus the torch expression for the SSE of every plane (no SSIM, no other
field).  Device time per call from torch events around K back-to-back calls on torch's current stream, the cases alternating in one
process, R rounds after one that warms up; prints one JSON line and writes it to --out.  Kernel times come from a run of their own
under rocprofv3 --kernel-trace --stats (the kernels are k_metrics<reference, ssim>).

    python tools/bench_metrics.py [--rounds 5] [--calls 20] [--out profiles/metrics_bench.json]"""
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
    from libhm_amd import abi, metrics
    from tests import metrics_ref as mref
    w, h, n, bd = a.width, a.height, 16, 10
    seq = abi.make_seq(w, h, bd, bd, max_pictures=2 * n + 2)
    rng = np.random.RandomState(11)
    base = [[rng.randint(0, 1 << bd, size=(h >> s, w >> s)).astype(np.int16) for s in (0, 1, 1)] for _ in range(4)]
    other = [[np.clip(p.astype(np.int32) + rng.randint(-40, 41, size=p.shape), 0, (1 << bd) - 1).astype(np.int16) for p in planes] for planes in base]
    with libhm_amd.Context(seq) as ctx:
        pics, refs = [], []
        for i in range(n):
            for planes, into in ((base[i % 4], pics), (other[i % 4], refs)):
                hnd = ctx.acquire()
                ctx.upload(hnd, planes)
                into.append(hnd)
        ctx.sync()
        planes16 = ctx.export_batch(refs, "planar", bd)                  # the reference as uint16 planes [16, h_c, w_c]
        torch.cuda.synchronize()
        # one picture of each call against the model, so that what is timed is known to be right
        got = {k: metrics.records(ctx.metrics(pics[:1], **kw)).cpu().numpy() for k, kw in
               (("pictures", dict(ref_pics=refs[:1])), ("planes", dict(ref=[t[:1] for t in planes16])))}
        want = mref.picture(base[0], other[0], 1, (bd, bd))
        for k in range(3):
            for f, name in enumerate(mref.FIELDS):
                for key in got:
                    d = abs(int(got[key][0, k, f]) - want[k][name])
                    assert d <= (mref.tolerance(want[k]["ssim_windows"]) if name == "ssim_q32" else 0), (key, k, name, d)
        out_a, out_b = ctx.export_batch(pics, "planar", bd), ctx.export_batch(refs, "planar", bd)

        def before():
            ea, eb = ctx.export_batch(pics, "planar", bd, out=out_a), ctx.export_batch(refs, "planar", bd, out=out_b)
            return [((x.to(torch.int32) - y.to(torch.int32)) ** 2).sum(dim=(1, 2), dtype=torch.int64) for x, y in zip(ea, eb)]

        def before_planes():                                             # the reference already lies in planes: one export
            ea = ctx.export_batch(pics, "planar", bd, out=out_a)
            return [((x.to(torch.int32) - y.to(torch.int32)) ** 2).sum(dim=(1, 2), dtype=torch.int64) for x, y in zip(ea, planes16)]
        sse = torch.stack(before(), dim=1).cpu().numpy()
        full = metrics.records(ctx.metrics(pics, ref_pics=refs, ssim=False)).cpu().numpy()
        assert np.array_equal(sse, full[:, :, 1])                        # the two ways agree on the SSE of all 48 planes
        cases = {
            "metrics_pictures_ssim": lambda: ctx.metrics(pics, ref_pics=refs),
            "metrics_pictures": lambda: ctx.metrics(pics, ref_pics=refs, ssim=False),
            "metrics_planes_u16_ssim": lambda: ctx.metrics(pics, ref=planes16),
            "metrics_planes_u16": lambda: ctx.metrics(pics, ref=planes16, ssim=False),
            "before_export_both_and_torch_sse": before,
            "before_export_one_and_torch_sse": before_planes,
        }
        times = {k: [] for k in cases}
        for rnd in range(a.rounds + 1):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:                                                  # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        # algorithmic bytes per call: 2 bytes of the picture and 2 of the reference per sample, 1.5 samples per luma sample in 4:2:0;
        # the records are 3 KiB.  (The cases before: the same reads, the planar tensors written and read again, and torch's temporaries.)
        samples = n * w * h * 3 // 2
        res = {"pictures": n, "width": w, "height": h, "bit_depth": bd, "rounds": a.rounds, "calls_per_round": a.calls,
               "device": torch.cuda.get_device_name(0), "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            nbytes = samples * 4 if name.startswith("metrics") else None
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": nbytes,
                                  "share_of_8TBps": None if nbytes is None else round(nbytes / (med * 1e-6) / 8e12, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
