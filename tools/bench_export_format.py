"""Format export measurements, one JSON object on stdout.

Sources: 16 distinct uploaded 3840x2160 Main10 pictures per batch, of the chroma format the case converts from.  Cases:
  4:2:0 -> planar 4:4:4 (one [N, 3, H, W] tensor), chroma replicate and linear, uint8 and float16;
  4:4:4 -> NV12 (uint8) and P010 (uint16, msb_aligned), chroma_down drop and linear;
  4:2:2 -> P010, chroma_down linear.
Per case two paths alternate in one process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch events
around the calls, the median round reported and every round kept:
  format:    Context.export_batch(chroma_format=...) into preallocated tensors;
  baseline:  the existing planar export of the same pictures at their own chroma format, the same element type.
Each path also as achieved bytes/s: the bytes of the source planes (2 per sample, luma and both chroma planes, once) plus the bytes
the plan says the call writes.  `--baseline-only` runs the second path alone and never names chroma_format=: the same tool then runs
on a checkout from before the format export, which is how the existing instances are compared with their parent's.
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
# name: (source format, layout, output format, keywords of the format path, bit_depth, msb_aligned, float16)
CASES = {
    "420_to_planar444_replicate_u8": (1, "planar", "444", dict(chroma="replicate"), 8, False, False),
    "420_to_planar444_linear_u8": (1, "planar", "444", dict(chroma="linear", chroma_loc=2), 8, False, False),
    "420_to_planar444_replicate_f16": (1, "planar", "444", dict(chroma="replicate"), 8, False, True),
    "420_to_planar444_linear_f16": (1, "planar", "444", dict(chroma="linear", chroma_loc=2), 8, False, True),
    "444_to_nv12_drop": (3, "semiplanar", "420", dict(chroma_down="drop"), 8, False, False),
    "444_to_nv12_linear": (3, "semiplanar", "420", dict(chroma_down="linear"), 8, False, False),
    "444_to_p010_drop": (3, "semiplanar", "420", dict(chroma_down="drop"), 10, True, False),
    "444_to_p010_linear": (3, "semiplanar", "420", dict(chroma_down="linear"), 10, True, False),
    "422_to_p010_linear": (2, "semiplanar", "420", dict(chroma_down="linear"), 10, True, False),
}


def shifts(fmt):
    return (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)


def make_context(fmt, n):
    seq = abi.make_seq(W, H, 10, 10, max_pictures=n)
    seq.chroma_format = fmt
    ctx = libhm_amd.Context(seq)
    rng = np.random.default_rng(W + fmt)
    sx, sy = shifts(fmt)
    pics = []
    for i in range(n):
        p = ctx.acquire()
        base = rng.integers(0, 1024, (H, W)).astype(np.int16)
        ctx.upload(p, [base, base[::1 << sy, ::1 << sx].copy(), base[sy::1 << sy, sx::1 << sx].copy()])
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


def nbytes(out):
    return sum(t.numel() * t.element_size() for t in (out if isinstance(out, tuple) else (out,)))


def spread(us):
    return round((max(us) - min(us)) / statistics.median(us), 4)


def bench(a):
    import torch
    res = {}
    for fmt in (1, 3, 2):
        names = [k for k, v in CASES.items() if v[0] == fmt and (not a.cases or k in a.cases)]
        if not names:
            continue
        ctx, pics = make_context(fmt, N)
        sx, sy = shifts(fmt)
        read = N * 2 * (W * H + 2 * (W >> sx) * (H >> sy))
        for name in names:
            _, layout, out_fmt, fkw, depth, msb, f16 = CASES[name]
            kw = dict(msb_aligned=msb)
            if f16:
                kw.update(dtype=torch.float16, mean=MEAN, std=STD)
            base_out = ctx.export_batch(pics, "planar", depth, **kw)
            paths = {"baseline": (lambda: ctx.export_batch(pics, "planar", depth, out=base_out, **kw), base_out)}
            if not a.baseline_only:
                fmt_out = ctx.export_batch(pics, layout, depth, chroma_format=out_fmt, **fkw, **kw)
                paths["format"] = (lambda: ctx.export_batch(pics, layout, depth, out=fmt_out, chroma_format=out_fmt, **fkw, **kw), fmt_out)
            torch.cuda.synchronize()
            rounds = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k in sorted(paths, reverse=True):
                    rounds[k].append(time_batches(paths[k][0], a.iters))
            case = {}
            for k, us in rounds.items():
                m, total = statistics.median(us), read + nbytes(paths[k][1])
                case.update({k + "_us_per_batch": round(m, 1), k + "_rounds_us": [round(x, 1) for x in us], k + "_spread": spread(us),
                             k + "_bytes": total, k + "_gb_per_s": round(total / m / 1e3, 1)})
            if "format" in rounds:
                case["format_over_baseline_bandwidth"] = round(case["format_gb_per_s"] / case["baseline_gb_per_s"], 3)
            res[name] = case
            del paths, base_out
            torch.cuda.empty_cache()
        ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="batches per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--cases", nargs="*", default=None, help="a subset of: " + " ".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    res = {"baseline_only": a.baseline_only,
           "source_note": "%d distinct uploaded %dx%d Main10 pictures per batch; wall time per batch of %d from torch events, %d rounds of %d "
                          "batches, the paths alternated, medians; spread = (max - min) / median of the rounds; bytes = source planes read "
                          "once (2 per sample) + the planned output" % (N, W, H, N, a.rounds, a.iters),
           "cases": bench(a)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
