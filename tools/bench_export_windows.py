"""Batched export with per-picture windows and mirrors, measurements, one JSON object on stdout.

Sources: 16 distinct uploaded 3840x2160 Main10 4:2:0 pictures, as tools/bench_export_batch.py uses.  Output: RGB float16 224x224,
ImageNet-normalised, bilinear and bicubic.  The windows are random-resized-crop windows (export.random_resized_crop, a fixed seed):
`--sets` sets of 16, one set per call in turn, so that no call repeats the windows of the one before it.

Wall time: one windows call (Context.export_batch(windows=, flip=) into a preallocated tensor) against the path a consumer had
before it: sixteen export(out=u8[i], size=, crop=) calls, then the flips and ((u8.float() / 255 - mean) / std).half() in torch.  The
two alternate in one process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch events around the calls;
the median round is reported and every round kept.  Host time: the Python wall time of the calls alone (time.perf_counter around
`--iters` calls, the device synchronised before and after, not in between), per batch, for both paths.

The kernel times come from a separate run under rocprofv3, nothing else traced:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/bench_export_windows.py --kernel-only --iters 20
  python tools/bench_export_windows.py --split-trace DIR/run_kernel_trace.csv --iters 20 --out profiles/export_windows_kernel_cases.json
--kernel-only runs, per filter, one warm-up and N windows calls, then one warm-up and N batched calls with one crop for all (the
whole picture) at the same output.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import libhm_amd  # noqa: E402
from libhm_amd import abi, export  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, N = 3840, 2160, 16
SIZE = (224, 224)
FILTERS = ["bilinear", "bicubic"]
SEED = 2160


def window_sets(count):
    import torch
    gen = torch.Generator().manual_seed(SEED)
    return [export.random_resized_crop(N, W, H, generator=gen, chroma_format=1) for _ in range(count)]


def coverage(sets):
    return float(np.mean([w * h / float(W * H) for ws, _ in sets for _, _, w, h in ws]))


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
    """(wall time per call from torch events, host time per call) of fn in microseconds over `iters` calls"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters, (t1 - t0) * 1e6 / iters


def paths(ctx, pics, filt, sets):
    import torch
    kw = dict(size=SIZE, filter=filt)
    u8 = torch.empty((N, 3) + SIZE, dtype=torch.uint8, device="cuda")
    out = torch.empty((N, 3) + SIZE, dtype=torch.float16, device="cuda")
    mean = torch.tensor(MEAN, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(STD, device="cuda").view(1, 3, 1, 1)
    masks = [torch.tensor(f, device="cuda").view(N, 1, 1, 1) for _, f in sets]
    turn = [0, 0]

    def windows_call():
        ws, fs = sets[turn[0] % len(sets)]
        turn[0] += 1
        ctx.export_batch(pics, "rgb", 8, out=out, windows=ws, flip=fs, dtype=torch.float16, mean=MEAN, std=STD, **kw)

    def baseline():
        k = turn[1] % len(sets)
        turn[1] += 1
        ws, _ = sets[k]
        for i, p in enumerate(pics):
            x, y, w, h = ws[i]
            ctx.export(p, "rgb", 8, out=u8[i], crop=(x, W - x - w, y, H - y - h), **kw)
        f = ((u8.float() / 255 - mean) / std).half()
        return torch.where(masks[k], f.flip(-1), f)
    return windows_call, baseline, out, turn


def bench(a, ctx, pics):
    import torch
    sets = window_sets(a.sets)
    res = {}
    for filt in FILTERS:
        windows_call, baseline, out, turn = paths(ctx, pics, filt, sets)
        for _ in range(3):
            turn[0] = turn[1] = 0
            windows_call()
            ref = baseline()
        torch.cuda.synchronize()
        # (the two paths agree up to the consumer's own arithmetic: its float32 division differs from the two rounded operations)
        diff = float((out.float() - ref.float()).abs().max())
        b_us, c_us, b_host, c_host = [], [], [], []
        for _ in range(a.rounds):
            t, h = time_batches(windows_call, a.iters)
            b_us.append(t)
            b_host.append(h)
            t, h = time_batches(baseline, a.iters)
            c_us.append(t)
            c_host.append(h)
        b, c = statistics.median(b_us), statistics.median(c_us)
        spread = max(max(b_us) - min(b_us), max(c_us) - min(c_us))
        res["rgb_f16_224_" + filt] = {
            "size": list(SIZE), "filter": filt, "dtype": "float16",
            "windows_us_per_batch": round(b, 1), "baseline_us_per_batch": round(c, 1), "speedup": round(c / b, 2),
            "windows_rounds_us": [round(x, 1) for x in b_us], "baseline_rounds_us": [round(x, 1) for x in c_us],
            "round_spread_us": round(spread, 1), "windows_faster_beyond_spread": bool(c - b > spread),
            "windows_host_us_per_batch": round(statistics.median(b_host), 1), "baseline_host_us_per_batch": round(statistics.median(c_host), 1),
            "windows_host_rounds_us": [round(x, 1) for x in b_host], "baseline_host_rounds_us": [round(x, 1) for x in c_host],
            "max_abs_difference_to_baseline": diff}
        del out, ref, windows_call, baseline
        torch.cuda.empty_cache()
    return res, coverage(sets)


def kernel_only(a, ctx, pics):
    import torch
    sets = window_sets(a.sets)
    for filt in FILTERS:
        windows_call, _, out, _ = paths(ctx, pics, filt, sets)
        for _ in range(a.iters + 1):
            windows_call()
        torch.cuda.synchronize()
        for _ in range(a.iters + 1):
            ctx.export_batch(pics, "rgb", 8, out=out, size=SIZE, filter=filt, dtype=torch.float16, mean=MEAN, std=STD)
        torch.cuda.synchronize()
        del out, windows_call
        torch.cuda.empty_cache()


def split_trace(trace, iters, sets, out):
    """per-case kernel times from the kernel trace CSV of a `--kernel-only --iters N` run: the export launches in start order are,
    per filter, 1 + N windows calls, then 1 + N common-crop calls (one launch per call); the first of each group is left out"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_export" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    want = len(FILTERS) * 2 * (iters + 1)
    if len(rows) != want:
        raise SystemExit("%s: %d export launches, expected %d (one per call)" % (trace, len(rows), want))
    res, pos = {"mean_fraction_of_picture_in_windows": round(coverage(window_sets(sets)), 4)}, 0
    for filt in FILTERS:
        for kind in ("windows", "common_crop"):
            seg = rows[pos + 1:pos + iters + 1]
            pos += iters + 1
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg]
            med = statistics.median(us)
            res["rgb_f16_224_%s_%s" % (filt, kind)] = {
                "kernel": seg[0]["Kernel_Name"], "launches": len(seg), "launches_per_call": 1, "pictures_per_launch": N,
                "kernel_us_median": round(med, 1), "kernel_us_min": round(min(us), 1), "kernel_us_max": round(max(us), 1),
                "kernel_us_per_picture": round(med / N, 2)}
        w, c = (res["rgb_f16_224_%s_%s" % (filt, k)]["kernel_us_per_picture"] for k in ("windows", "common_crop"))
        res["rgb_f16_224_%s_windows" % filt]["per_picture_ratio_to_common_crop"] = round(w / c, 3)
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="batches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=20, help="distinct sets of 16 windows, used in turn")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-trace", default=None, metavar="TRACE_CSV",
                    help="no GPU: write the per-case kernel times of a --kernel-only trace to --out (JSON) and stop")
    a = ap.parse_args()
    if a.split_trace:
        split_trace(a.split_trace, a.iters, a.sets, a.out)
        return
    import torch
    torch.zeros(1, device="cuda")
    ctx, pics = make_context(N)
    if a.kernel_only:
        kernel_only(a, ctx, pics)
        print(json.dumps({"kernel_only": True, "iters": a.iters}))
        return
    cases, cover = bench(a, ctx, pics)
    res = {"source_note": "%d distinct uploaded %dx%d Main10 4:2:0 pictures per batch; random-resized-crop windows (seed %d, %d sets of %d "
                          "used in turn) and flips; wall time per batch from torch events, %d rounds of %d batches alternated with the "
                          "baseline, medians; host time: perf_counter around the calls of a round" % (N, W, H, SEED, a.sets, N, a.rounds, a.iters),
           "baseline_note": "sixteen export(out=u8[i], size=, crop=) calls, then ((u8.float() / 255 - mean) / std).half() and torch.where(flip, "
                            "x.flip(-1), x)",
           "mean_fraction_of_picture_in_windows": round(cover, 4),
           "cases": cases}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
