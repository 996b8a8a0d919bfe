"""Packed pixel export measurements, one JSON object on stdout.

Sources: `--pictures` (16) distinct uploaded 3840x2160 Main10 4:2:0 pictures, as tools/bench_export_batch.py uses.  Per case one
packed call (Context.export_batch(pixel= / memory_format=) into a preallocated tensor) against the path a consumer had before it:
the planar export_batch into a preallocated [N, 3, H, W] tensor, then the re-layout in torch -- .permute(0, 2, 3, 1).contiguous()
for RGB, torch.stack of the B, G, R planes and an A plane on the last axis for BGRA, .contiguous(memory_format=torch.channels_last)
for the float cases.  The two alternate in one process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch
events around the calls; the median round is reported, and every round is kept.  Both paths write the same bytes (checked).

The kernel times come from a separate run under rocprofv3, nothing else traced:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/bench_export_pixels.py --kernel-only --iters 20
  python tools/bench_export_pixels.py --split-trace DIR/run_kernel_trace.csv --iters 20 --out profiles/export_pixels_kernel_cases.json
--kernel-only runs, per case, one warm-up and N packed calls, nothing else.
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
from libhm_amd import abi, export  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, N = 3840, 2160, 16
# name, size (h, w) or None, pixel order or None (channels-last), float16 output, random-resized-crop windows
CASES = [("rgb_u8_unscaled", None, "rgb", False, False),
         ("bgra_u8_unscaled", None, "bgra", False, False),
         ("channels_last_f16_unscaled", None, None, True, False),
         ("channels_last_f16_224_bilinear_rrc", (224, 224), None, True, True)]


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


def paths(ctx, pics, size, pixel, f16, rrc):
    """(packed, baseline, the packed destination): the baseline returns its re-laid-out tensor"""
    import torch
    hw = size or (H, W)
    dt = torch.float16 if f16 else torch.uint8
    kw = dict(size=size, filter="bilinear")
    if f16:
        kw.update(dtype=torch.float16, mean=MEAN, std=STD)
    if rrc:
        w, f = export.random_resized_crop(N, W, H, generator=torch.Generator().manual_seed(1), chroma_format=1)
        kw.update(windows=w, flip=f)
    planar = torch.empty((N, 3) + hw, dtype=dt, device="cuda")
    c = 3 if pixel is None else len(pixel)
    out = torch.empty((N,) + hw + (c,), dtype=dt, device="cuda")
    if pixel is None:
        out = out.permute(0, 3, 1, 2)                                    # [N, 3, H, W], channels-last strides

        def packed():
            ctx.export_batch(pics, "rgb", 8, out=out, memory_format=torch.channels_last, **kw)

        def baseline():
            ctx.export_batch(pics, "rgb", 8, out=planar, **kw)
            return planar.contiguous(memory_format=torch.channels_last)
    elif pixel == "rgb":
        def packed():
            ctx.export_batch(pics, "rgb", 8, out=out, pixel="rgb", **kw)

        def baseline():
            ctx.export_batch(pics, "rgb", 8, out=planar, **kw)
            return planar.permute(0, 2, 3, 1).contiguous()
    else:
        alpha = torch.full((N,) + hw, 255, dtype=dt, device="cuda")

        def packed():
            ctx.export_batch(pics, "rgb", 8, out=out, pixel="bgra", **kw)

        def baseline():
            ctx.export_batch(pics, "rgb", 8, out=planar, **kw)
            return torch.stack((planar[:, 2], planar[:, 1], planar[:, 0], alpha), dim=-1)
    return packed, baseline, out


def bench(a, ctx, pics):
    import torch
    res = {}
    for name, size, pixel, f16, rrc in CASES:
        packed, baseline, out = paths(ctx, pics, size, pixel, f16, rrc)
        for _ in range(3):
            packed()
            ref = baseline()
        torch.cuda.synchronize()
        equal = bool(torch.equal(out, ref))
        del ref
        p_us, b_us = [], []
        for _ in range(a.rounds):
            p_us.append(time_batches(packed, a.iters))
            b_us.append(time_batches(baseline, a.iters))
        p, b = statistics.median(p_us), statistics.median(b_us)
        spread = max(max(p_us) - min(p_us), max(b_us) - min(b_us))
        res[name] = {"size": list(size or (H, W)), "filter": "bilinear" if size else None, "dtype": "float16" if f16 else "uint8",
                     "layout": "channels_last" if pixel is None else pixel, "windows": "random_resized_crop" if rrc else None,
                     "output_bytes_per_batch": out.numel() * out.element_size(),
                     "packed_us_per_batch": round(p, 1), "baseline_us_per_batch": round(b, 1), "speedup": round(b / p, 2),
                     "packed_rounds_us": [round(x, 1) for x in p_us], "baseline_rounds_us": [round(x, 1) for x in b_us],
                     "round_spread_us": round(spread, 1), "packed_faster_beyond_spread": bool(b - p > spread),
                     "equal_to_baseline": equal}
        del out, packed, baseline
        torch.cuda.empty_cache()
    return res


def kernel_only(a, ctx, pics):
    import torch
    for name, size, pixel, f16, rrc in CASES:
        packed, _, out = paths(ctx, pics, size, pixel, f16, rrc)
        for _ in range(a.iters + 1):
            packed()
        torch.cuda.synchronize()
        del out, packed
        torch.cuda.empty_cache()


def split_trace(trace, iters, out):
    """per-case kernel times from the kernel trace CSV of a `--kernel-only --iters N` run: the export launches in start order are
    1 + N per case (one per packed call); the first of each group is left out"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_export" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    want = len(CASES) * (iters + 1)
    if len(rows) != want:
        raise SystemExit("%s: %d export launches, expected %d (one per packed call)" % (trace, len(rows), want))
    res, pos = {}, 0
    for name, size, pixel, f16, rrc in CASES:
        seg = rows[pos + 1:pos + iters + 1]
        pos += iters + 1
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg]
        med = statistics.median(us)
        hw = size or (H, W)
        nbytes = N * hw[0] * hw[1] * (3 if pixel is None else len(pixel)) * (2 if f16 else 1)
        res[name] = {"kernel": seg[0]["Kernel_Name"], "launches": len(seg), "launches_per_call": 1, "pictures_per_launch": N,
                     "kernel_us_median": round(med, 1), "kernel_us_min": round(min(us), 1), "kernel_us_max": round(max(us), 1),
                     "kernel_us_per_picture": round(med / N, 2), "output_bytes": nbytes,
                     "output_gb_per_s": round(nbytes / med / 1e3, 1)}
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
           "baseline_note": "the planar export_batch into a preallocated [N, 3, H, W] tensor, then in torch .permute(0, 2, 3, 1).contiguous() "
                            "(rgb), torch.stack((B, G, R, A), -1) (bgra), .contiguous(memory_format=torch.channels_last) (float16)",
           "cases": bench(a, ctx, pics)}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
