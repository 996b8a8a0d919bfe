"""Packed YUV export measurements, one JSON object on stdout.

Sources: 16 distinct uploaded 3840x2160 Main10 pictures per batch, a 4:2:0 set and a 4:2:2 set.  Each packed case alternates in one
process with the existing semi-planar format export of the same pictures at the same output chroma format and container -- UYVY
against 8-bit NV16, Y210 and v210 against P210 (msb_aligned), Y410 against 10-bit NV24 -- so that the yardstick is the existing
kernel, not the code under test: the same bytes read, and the same bytes written except for v210 and Y410, which write two thirds of
P210's and of NV24's.
`--rounds` rounds of `--iters` calls each, wall time per call from torch events around the calls, the median round reported and every
round kept.  Each path also as achieved bytes/s over its algorithmic bytes: the source planes once (2 bytes per sample) plus the bytes
the call writes.
Import: UYVY and v210 words into the 4:2:2 pictures, each against the planar import of the same samples (uint8 planes for UYVY,
uint16 planes for v210); bytes = the source once plus the picture's planes written (2 bytes per sample).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_export_format import H, N, W, make_context, nbytes, shifts, spread, time_batches  # noqa: E402

# name: (source format, yuv, yardstick's chroma_format, bit depth, msb_aligned, conversion keywords)
CASES = {
    "420_to_uyvy": (1, "uyvy", "422", 8, False, dict(chroma="linear", chroma_loc=0)),
    "420_to_y210": (1, "y210", "422", 10, True, dict(chroma="linear", chroma_loc=0)),
    "420_to_v210": (1, "v210", "422", 10, True, dict(chroma="linear", chroma_loc=0)),
    "420_to_y410": (1, "y410", "444", 10, False, dict(chroma="linear", chroma_loc=0)),
    "422_to_uyvy": (2, "uyvy", "422", 8, False, {}),
    "422_to_y210": (2, "y210", "422", 10, True, {}),
    "422_to_v210": (2, "v210", "422", 10, True, {}),
}


def written(yuv):
    """the bytes a packed export writes per picture: its rows without the pitch"""
    return H * {"uyvy": 2 * W, "y210": 4 * W, "v210": (W + 5) // 6 * 16, "y410": 4 * W}[yuv]


IMPORTS = {"uyvy_to_422": ("uyvy", 8), "v210_to_422": ("v210", 10)}


def bench_imports(a, res):
    import torch
    names = [k for k in IMPORTS if not a.cases or k in a.cases]
    if not names:
        return
    ctx, pics = make_context(2, N)
    wrote = N * 2 * (W * H + 2 * (W // 2) * H)
    for name in names:
        yuv, depth = IMPORTS[name]
        words = ctx.export_batch(pics, yuv=yuv)
        planes = ctx.export_batch(pics, "planar", depth)
        paths = {"yardstick": (lambda: ctx.import_batch(pics, planes, layout="planar", bit_depth=depth, chroma_format="422"), nbytes(planes)),
                 "packed": (lambda: ctx.import_batch(pics, words, yuv=yuv, size=(H, W)), N * written(yuv))}
        torch.cuda.synchronize()
        rounds = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k in sorted(paths, reverse=True):
                rounds[k].append(time_batches(paths[k][0], a.iters))
        case = {}
        for k, us in rounds.items():
            m, total = statistics.median(us), wrote + paths[k][1]
            case.update({k + "_us_per_call": round(m, 1), k + "_rounds_us": [round(x, 1) for x in us], k + "_spread": spread(us),
                         k + "_bytes": total, k + "_gb_per_s": round(total / m / 1e3, 1)})
        case["packed_over_yardstick_bandwidth"] = round(case["packed_gb_per_s"] / case["yardstick_gb_per_s"], 3)
        res["import_" + name] = case
        del paths, words, planes
        torch.cuda.empty_cache()
    ctx.close()


def bench(a):
    import torch
    res = {}
    for fmt in (1, 2):
        names = [k for k, v in CASES.items() if v[0] == fmt and (not a.cases or k in a.cases)]
        if not names:
            continue
        ctx, pics = make_context(fmt, N)
        sx, sy = shifts(fmt)
        read = N * 2 * (W * H + 2 * (W >> sx) * (H >> sy))
        for name in names:
            _, yuv, cf, depth, msb, kw = CASES[name]
            ref_out = ctx.export_batch(pics, "semiplanar", depth, msb_aligned=msb, chroma_format=cf, **kw)
            out = ctx.export_batch(pics, yuv=yuv, row_align=128 if yuv == "v210" else 1, **kw)
            paths = {"yardstick": (lambda: ctx.export_batch(pics, "semiplanar", depth, msb_aligned=msb, chroma_format=cf, out=ref_out, **kw),
                                   nbytes(ref_out)),
                     "packed": (lambda: ctx.export_batch(pics, yuv=yuv, out=out, row_align=128 if yuv == "v210" else 1, **kw), N * written(yuv))}
            torch.cuda.synchronize()
            rounds = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k in sorted(paths, reverse=True):
                    rounds[k].append(time_batches(paths[k][0], a.iters))
            case = {}
            for k, us in rounds.items():
                m, total = statistics.median(us), read + paths[k][1]
                case.update({k + "_us_per_call": round(m, 1), k + "_rounds_us": [round(x, 1) for x in us], k + "_spread": spread(us),
                             k + "_bytes": total, k + "_gb_per_s": round(total / m / 1e3, 1)})
            case["packed_over_yardstick_bandwidth"] = round(case["packed_gb_per_s"] / case["yardstick_gb_per_s"], 3)
            res[name] = case
            del paths, ref_out, out
            torch.cuda.empty_cache()
        ctx.close()
    bench_imports(a, res)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", nargs="*", default=None, help="a subset of: " + " ".join(list(CASES) + list(IMPORTS)))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    res = {"source_note": "%d distinct uploaded %dx%d Main10 pictures per call; wall time per call from torch events, %d rounds of %d calls, "
                          "the paths alternated, medians; spread = (max - min) / median of the rounds; bytes = source planes read once (2 per "
                          "sample) + the bytes written" % (N, W, H, a.rounds, a.iters),
           "cases": bench(a)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
