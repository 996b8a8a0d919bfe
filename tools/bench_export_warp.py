"""Affine warp export, measurements, one JSON object on stdout.

Two shapes, 16 distinct uploaded Main10 4:2:0 pictures each, RGB float16, ImageNet-normalised:
  2160p_to_224   3840x2160 sources, random-resized-crop windows (export.random_resized_crop, a fixed seed), each window through a
                 random rotation / shear / zoom that maps the 224x224 output onto it (export.affine_map; bilinear, edge)
  1080p_identity 1920x1080 sources at their own size, each through a rotation of a few degrees about its centre
Per shape three calls on the same pictures, alternated in one process: the warp call; the existing windows + bilinear scale call
with the same windows and output size; the existing unscaled call (whole pictures).  `--rounds` rounds of `--iters` calls each, wall
time per call from torch events around the calls; the median round is reported and every round kept.

The kernel times come from a separate run under rocprofv3, nothing else traced:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/bench_export_warp.py --kernel-only --iters 20
  python tools/bench_export_warp.py --split-trace DIR/run_kernel_trace.csv --iters 20 --out profiles/export_warp_kernel_cases.json
--kernel-only runs, per shape and call, one warm-up and N calls.
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
N = 16
SEED = 2160
SHAPES = {"2160p_to_224": (3840, 2160, (224, 224)), "1080p_identity": (1920, 1080, (1080, 1920))}
CALLS = ("warp", "windows_bilinear", "unscaled")


def make_context(w, h):
    seq = abi.make_seq(w, h, 10, 10, max_pictures=N)
    ctx = libhm_amd.Context(seq)
    rng = np.random.default_rng(w)
    pics = []
    for _ in range(N):
        p = ctx.acquire()
        base = rng.integers(0, 1024, (h, w)).astype(np.int16)
        ctx.upload(p, [base, base[::2, ::2].copy(), base[1::2, 1::2].copy()])
        pics.append(p)
    ctx.sync()
    return ctx, pics


def geometry(name):
    """(windows, maps) of a shape: fixed for the run"""
    import torch
    w, h, size = SHAPES[name]
    gen = torch.Generator().manual_seed(SEED)
    rng = np.random.default_rng(SEED)
    if name == "1080p_identity":
        wins = [(0, 0, w, h)] * N
        return wins, [export.affine_map(size, (h, w), angle=rng.uniform(-5, 5)) for _ in range(N)]
    wins, _ = export.random_resized_crop(N, w, h, generator=gen, chroma_format=1)
    maps = []
    for (_, _, ww, wh) in wins:
        zoom = min(size[1] / ww, size[0] / wh) * rng.uniform(1.0, 1.3)       # the window fills the output; no prefilter: see the header
        maps.append(export.affine_map(size, (wh, ww), angle=rng.uniform(-30, 30), scale=zoom, shear=(rng.uniform(-10, 10), 0.0)))
    return wins, maps


def calls_of(ctx, pics, name):
    import torch
    w, h, size = SHAPES[name]
    wins, maps = geometry(name)
    kw = dict(dtype=torch.float16, mean=MEAN, std=STD)
    small = torch.empty((N, 3) + size, dtype=torch.float16, device="cuda")
    whole = torch.empty((N, 3, h, w), dtype=torch.float16, device="cuda")
    return {"warp": lambda: ctx.export_batch(pics, "rgb", 8, out=small, windows=wins, warp=maps, size=size, **kw),
            "windows_bilinear": lambda: ctx.export_batch(pics, "rgb", 8, out=small, windows=wins, size=size, filter="bilinear", **kw),
            "unscaled": lambda: ctx.export_batch(pics, "rgb", 8, out=whole, **kw)}


def time_calls(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench(a):
    import torch
    res = {}
    for name, (w, h, size) in SHAPES.items():
        ctx, pics = make_context(w, h)
        fns = calls_of(ctx, pics, name)
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in CALLS}
        for _ in range(a.rounds):
            for k in CALLS:
                rounds[k].append(time_calls(fns[k], a.iters))
        res[name] = {"source": [h, w], "size": list(size), "pictures": N, "dtype": "float16"}
        for k in CALLS:
            res[name][k + "_us_per_call"] = round(statistics.median(rounds[k]), 1)
            res[name][k + "_rounds_us"] = [round(x, 1) for x in rounds[k]]
        del fns
        ctx.close()
        torch.cuda.empty_cache()
    return res


def kernel_only(a):
    import torch
    for name, (w, h, _) in SHAPES.items():
        ctx, pics = make_context(w, h)
        fns = calls_of(ctx, pics, name)
        for k in CALLS:
            for _ in range(a.iters + 1):
                fns[k]()
            torch.cuda.synchronize()
        del fns
        ctx.close()
        torch.cuda.empty_cache()


def split_trace(trace, iters, out):
    """per-case kernel times from the kernel trace CSV of a `--kernel-only --iters N` run: the export launches in start order are,
    per shape and call, 1 + N launches (one launch per call); the first of each group is left out"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_export" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    want = len(SHAPES) * len(CALLS) * (iters + 1)
    if len(rows) != want:
        raise SystemExit("%s: %d export launches, expected %d (one per call)" % (trace, len(rows), want))
    res, pos = {}, 0
    for name in SHAPES:
        for k in CALLS:
            seg = rows[pos + 1:pos + iters + 1]
            pos += iters + 1
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg]
            res["%s_%s" % (name, k)] = {"kernel": seg[0]["Kernel_Name"][:80], "launches": len(seg), "pictures_per_launch": N,
                                        "kernel_us_median": round(statistics.median(us), 1), "kernel_us_min": round(min(us), 1),
                                        "kernel_us_max": round(max(us), 1)}
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-trace", default=None, metavar="TRACE_CSV",
                    help="no GPU: write the per-case kernel times of a --kernel-only trace to --out (JSON) and stop")
    a = ap.parse_args()
    if a.split_trace:
        split_trace(a.split_trace, a.iters, a.out)
        return
    import torch
    torch.zeros(1, device="cuda")
    if a.kernel_only:
        kernel_only(a)
        print(json.dumps({"kernel_only": True, "iters": a.iters}))
        return
    res = {"source_note": "%d distinct uploaded Main10 4:2:0 pictures per call, RGB float16 normalised; wall time per call from torch "
                          "events, %d rounds of %d calls, the three calls alternated, medians" % (N, a.rounds, a.iters),
           "cases": bench(a)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
