"""Batched tensor export measurements, one JSON object on stdout.

Sources: `--pictures` (16) distinct uploaded 3840x2160 Main10 4:2:0 pictures, as tools/bench_export_scaled.py uses.  Per case one
batched call (Context.export_batch into a preallocated tensor) against the path a consumer had before it: sixteen
export(out=u8[i]) calls, then ((u8.float() / 255 - mean) / std).half() in torch (the uint8 case: the sixteen calls alone).  The two
alternate in one process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch events around the calls;
the median round is reported, and every round is kept.

The kernel times come from a separate run under rocprofv3, nothing else traced:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/bench_export_batch.py --kernel-only --iters 20
  python tools/bench_export_batch.py --split-trace DIR/run_kernel_trace.csv --iters 20 --out profiles/export_batch_kernel_cases.json
--kernel-only runs, per case, one warm-up and N batched calls, then the two single-picture references (RGB with a 2-byte container,
unscaled and at 1920x1080 bilinear: the instances that write the same bytes as the float16 ones), 16 N calls each.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libhm_amd  # noqa: E402
from libhm_amd import abi  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, N = 3840, 2160, 16
# name, size (h, w) or None, filter, float16 output
CASES = [("rgb_f16_224_area", (224, 224), "area", True),
         ("rgb_f16_224_bicubic", (224, 224), "bicubic", True),
         ("rgb_f16_1080p_bilinear", (1080, 1920), "bilinear", True),
         ("rgb_f16_unscaled", None, "bilinear", True),
         ("rgb_u8_unscaled", None, "bilinear", False)]
REFERENCES = [("single_rgb_u16_unscaled", None, "bilinear"), ("single_rgb_u16_1080p_bilinear", (1080, 1920), "bilinear")]


def make_context(n):
    seq = abi.make_seq(W, H, 10, 10, max_pictures=n)
    ctx = libhm_amd.Context(seq)
    rng = np.random.default_rng(W)
    pics = []
    for i in range(n):
        p = ctx.acquire()
        base = rng.integers(0, 1024, (H, W)).astype(np.int16)
        ctx.upload(p, [base, base[::2, ::2].copy(), base[1::2, 1::2].copy()])
        pics.append(p)
    ctx.sync()
    return ctx, pics


def time_batches(fn, iters):
    """wall time per call of fn in microseconds, from torch events around `iters` calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def paths(ctx, pics, size, filt, f16):
    import torch
    hw = size or (H, W)
    kw = dict(size=size, filter=filt)
    u8 = torch.empty((N, 3) + hw, dtype=torch.uint8, device="cuda")
    out = torch.empty((N, 3) + hw, dtype=torch.float16 if f16 else torch.uint8, device="cuda")
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    fkw = dict(dtype=torch.float16, mean=MEAN, std=STD) if f16 else {}

    def batched():
        ctx.export_batch(pics, "rgb", 8, out=out, **kw, **fkw)

    def baseline():
        for i, p in enumerate(pics):
            ctx.export(p, "rgb", 8, out=u8[i], **kw)
        if f16:
            return ((u8.float() / 255 - mean) / std).half()
        return u8
    return batched, baseline, out


def bench(a, ctx, pics):
    import torch
    res = {}
    for name, size, filt, f16 in CASES:
        batched, baseline, out = paths(ctx, pics, size, filt, f16)
        for _ in range(3):
            batched()
            ref = baseline()
        torch.cuda.synchronize()
        # (the two paths agree up to the consumer's own arithmetic: its float32 division differs from the two rounded operations)
        diff = float((out.float() - ref.float()).abs().max())
        b_us, c_us = [], []
        for _ in range(a.rounds):
            b_us.append(time_batches(batched, a.iters))
            c_us.append(time_batches(baseline, a.iters))
        b, c = statistics.median(b_us), statistics.median(c_us)
        spread = max(max(b_us) - min(b_us), max(c_us) - min(c_us))
        res[name] = {"size": list(size or (H, W)), "filter": filt if size else None, "dtype": "float16" if f16 else "uint8",
                     "batched_us_per_batch": round(b, 1), "baseline_us_per_batch": round(c, 1), "speedup": round(c / b, 2),
                     "batched_rounds_us": [round(x, 1) for x in b_us], "baseline_rounds_us": [round(x, 1) for x in c_us],
                     "round_spread_us": round(spread, 1), "batched_faster_beyond_spread": bool(c - b > spread),
                     "max_abs_difference_to_baseline": diff}
        del out, ref, batched, baseline
        torch.cuda.empty_cache()
    return res


def kernel_only(a, ctx, pics):
    import torch
    for name, size, filt, f16 in CASES:
        batched, _, out = paths(ctx, pics, size, filt, f16)
        for _ in range(a.iters + 1):
            batched()
        torch.cuda.synchronize()
        del out, batched
        torch.cuda.empty_cache()
    for name, size, filt in REFERENCES:
        hw = size or (H, W)
        dst = torch.empty((3,) + hw, dtype=torch.int16, device="cuda")
        for i in range(16 * a.iters + 1):
            ctx.export(pics[i % len(pics)], "rgb", 10, size=size, filter=filt, out=dst)
        torch.cuda.synchronize()


def split_trace(trace, iters, out):
    """per-case kernel times from the kernel trace CSV of a `--kernel-only --iters N` run: the export launches in start order are
    1 + N per case (one per batched call), then 1 + 16 N per reference; the first of each group is left out"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_export" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    want = len(CASES) * (iters + 1) + len(REFERENCES) * (16 * iters + 1)
    if len(rows) != want:
        raise SystemExit("%s: %d export launches, expected %d (one per batched call)" % (trace, len(rows), want))
    res, pos = {}, 0
    for name, count, per in [(c[0], iters + 1, N) for c in CASES] + [(r[0], 16 * iters + 1, 1) for r in REFERENCES]:
        seg = rows[pos + 1:pos + count]
        pos += count
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg]
        med = statistics.median(us)
        res[name] = {"kernel": seg[0]["Kernel_Name"], "launches": len(seg), "launches_per_call": 1, "pictures_per_launch": per,
                     "kernel_us_median": round(med, 1), "kernel_us_min": round(min(us), 1), "kernel_us_max": round(max(us), 1),
                     "kernel_us_per_picture": round(med / per, 2)}
    for f16, single in (("rgb_f16_unscaled", "single_rgb_u16_unscaled"), ("rgb_f16_1080p_bilinear", "single_rgb_u16_1080p_bilinear")):
        res[f16]["per_picture_ratio_to_" + single] = round(res[f16]["kernel_us_per_picture"] / res[single]["kernel_us_per_picture"], 3)
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="batches per round")
    ap.add_argument("--pictures", type=int, default=N)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-trace", default=None, metavar="TRACE_CSV",
                    help="no GPU: write the per-case kernel times of a --kernel-only trace to --out (JSON) and stop")
    a = ap.parse_args()
    if a.split_trace:
        split_trace(a.split_trace, a.iters, a.out)
        return
    if a.pictures != N:
        raise SystemExit("the cases are batches of %d pictures" % N)
    import torch
    torch.zeros(1, device="cuda")
    ctx, pics = make_context(a.pictures)
    if a.kernel_only:
        kernel_only(a, ctx, pics)
        print(json.dumps({"kernel_only": True, "iters": a.iters}))
        return
    res = {"source_note": "%d distinct uploaded %dx%d Main10 4:2:0 pictures per batch; wall time per batch of %d from torch events, "
                          "%d rounds of %d batches alternated with the baseline, medians" % (N, W, H, N, a.rounds, a.iters),
           "baseline_note": "sixteen export(out=u8[i]) calls, then ((u8.float() / 255 - mean) / std).half() (uint8 case: the calls alone)",
           "cases": bench(a, ctx, pics)}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
