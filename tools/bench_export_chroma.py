"""Chroma export measurements, one JSON object on stdout.

Sources: 16 distinct uploaded 3840x2160 Main10 4:2:0 pictures, as tools/bench_export_colour.py uses.  Workloads: unscaled uint8 in
three planes and as packed RGB, and the whole picture scaled to 224x224 float16 [N, 3, H, W].  Per workload two paths alternate in one
process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch events around the calls, the median round
reported and every round kept:
  linear:     Context.export_batch(chroma="linear", chroma_loc=--loc) into a preallocated tensor;
  replicate:  the same call without chroma= (the existing entries and kernel instances).
`--replicate-only` runs the second path alone and never names chroma=: the same tool then runs on a checkout from before the
chroma stage, which is how the existing instances are compared with their parent's.
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
W, H, N, DEPTH = 3840, 2160, 16, 8
WORKLOADS = ["planes_u8_unscaled", "rgb_u8_unscaled", "f16_224_bilinear"]


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


def paths(ctx, pics, name, loc):
    import torch
    if name == "planes_u8_unscaled":
        kw, out = {}, torch.empty((N, 3, H, W), dtype=torch.uint8, device="cuda")
    elif name == "rgb_u8_unscaled":
        kw, out = dict(pixel="rgb"), torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
    else:
        kw = dict(size=(224, 224), filter="bilinear", dtype=torch.float16, mean=MEAN, std=STD)
        out = torch.empty((N, 3, 224, 224), dtype=torch.float16, device="cuda")

    def linear():
        ctx.export_batch(pics, "rgb", DEPTH, out=out, chroma="linear", chroma_loc=loc, **kw)

    def replicate():
        ctx.export_batch(pics, "rgb", DEPTH, out=out, **kw)
    return linear, replicate, out


def spread(us):
    return round((max(us) - min(us)) / statistics.median(us), 4)


def bench(a, ctx, pics):
    import torch
    res = {}
    for name in WORKLOADS:
        linear, replicate, out = paths(ctx, pics, name, a.loc)
        replicate()
        if not a.replicate_only:
            linear()
        torch.cuda.synchronize()
        l_us, r_us = [], []
        for _ in range(a.rounds):
            if not a.replicate_only:
                l_us.append(time_batches(linear, a.iters))
            r_us.append(time_batches(replicate, a.iters))
        r = statistics.median(r_us)
        case = {"replicate_us_per_batch": round(r, 1), "replicate_rounds_us": [round(x, 1) for x in r_us], "replicate_spread": spread(r_us)}
        if l_us:
            m = statistics.median(l_us)
            case.update({"linear_us_per_batch": round(m, 1), "linear_rounds_us": [round(x, 1) for x in l_us], "linear_spread": spread(l_us),
                         "linear_over_replicate": round(m / r, 3), "stage_adds_us": round(m - r, 1)})
        res[name] = case
        del out, linear, replicate
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="batches per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loc", type=int, default=2, help="chroma_sample_loc_type of the linear path")
    ap.add_argument("--replicate-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    ctx, pics = make_context(N)
    res = {"loc": a.loc, "replicate_only": a.replicate_only,
           "source_note": "%d distinct uploaded %dx%d Main10 4:2:0 pictures per batch, 8-bit RGB output; wall time per batch of %d from "
                          "torch events, %d rounds of %d batches, the paths alternated, medians; spread = (max - min) / median of the rounds"
                          % (N, W, H, N, a.rounds, a.iters),
           "cases": bench(a, ctx, pics)}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
