"""Scaled device export measurements, one JSON object on stdout:

  (i)   k_export_scale on 3840x2160 Main10 4:2:0 pictures (and 1920x1080 ones for the enlargement), rotating over `--pictures`
        distinct uploaded pictures (16 x 24.9 MB: more than the 256 MiB Infinity Cache holds): device time per export from torch
        events, bytes from the shapes (the visible int16 planes read + bytes written), TB/s and the fraction of the 8 TB/s peak.  The
        kernel times themselves come from a separate `rocprofv3 --kernel-trace --stats` run of `--kernel-only`.
  (ii)  the same cases as torch does them today, alternated with (i) in one process: unscaled export, .float(), F.interpolate,
        round, clamp, uint8 -- device time per picture from torch events
  (iii) Python wall time per call of Context.export: unscaled, with size= (new tensors each call), and with size= and out=
  (iv)  Decoder.frames() on tests/golden/bench_ldp_wpp_main10_3840x2160.bin, size=(1080, 1920) against no size, RGB; pictures/s,
        `--rounds` rounds alternated, median

usage: python tools/bench_export_scaled.py [--iters N] [--pictures P] [--rounds R] [--threads T] [--kernel-only] [--out FILE]
The kernel times of DESIGN.md §9d:
  rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/bench_export_scaled.py --kernel-only --iters 100
  python tools/bench_export_scaled.py --split-trace DIR/run_kernel_trace.csv --iters 100 --out profiles/export_scaled_kernel_cases.csv
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
from libhm_amd import abi, hmdec  # noqa: E402

PEAK = 8.0e12
# name, source (w, h), layout, bit depth, bytes, msb, size (h, w), filter
CASES = [("rgb8_1080p_bilinear", (3840, 2160), "rgb", 8, 1, 0, (1080, 1920), "bilinear"),
         ("rgb8_640x360_bicubic", (3840, 2160), "rgb", 8, 1, 0, (360, 640), "bicubic"),
         ("rgb8_224_bicubic", (3840, 2160), "rgb", 8, 1, 0, (224, 224), "bicubic"),
         ("rgb8_224_area", (3840, 2160), "rgb", 8, 1, 0, (224, 224), "area"),
         ("planar8_1080p_bilinear", (3840, 2160), "planar", 8, 1, 0, (1080, 1920), "bilinear"),
         ("p010_1080p_bilinear", (3840, 2160), "nv12", 10, 2, 1, (1080, 1920), "bilinear"),
         ("rgb8_1080p_to_2160p_bilinear", (1920, 1080), "rgb", 8, 1, 0, (2160, 3840), "bilinear")]
BASELINES = [("unscaled_rgb8_2160p", (3840, 2160)), ("unscaled_rgb8_1080p", (1920, 1080))]
TORCH_MODE = {"bilinear": dict(mode="bilinear", antialias=True, align_corners=False),
              "bicubic": dict(mode="bicubic", antialias=True, align_corners=False), "area": dict(mode="area")}


def make_context(w, h, n):
    seq = abi.make_seq(w, h, 10, 10, max_pictures=n)
    ctx = libhm_amd.Context(seq)
    rng = np.random.default_rng(w)
    pics = []
    for i in range(n):
        p = ctx.acquire()
        base = rng.integers(0, 1024, (h, w)).astype(np.int16)
        ctx.upload(p, [base, base[::2, ::2].copy(), base[1::2, 1::2].copy()])
        pics.append(p)
    ctx.sync()
    return ctx, pics


def planes_of(t):
    return list(t) if isinstance(t, tuple) else [t]


def time_events(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def bench(a, ctxs):
    import torch
    import torch.nn.functional as F
    out = {}
    for name, (w, h), layout, bd, nbytes, msb, size, filt in CASES:
        ctx, pics = ctxs[(w, h)]
        P = len(pics)
        kw = dict(bit_depth=bd, msb_aligned=bool(msb))
        dst = planes_of(ctx.export(pics[0], layout, size=size, filter=filt, **kw))

        def fused(i):
            ctx.export(pics[i % P], layout, size=size, filter=filt, out=tuple(dst) if layout != "rgb" else dst[0], **kw)

        def torch_path(i):
            # as a consumer does it today: per output tensor [C, H, W] (RGB: 3 planes, YUV: 1 plane, CbCr: 2 channels) as one batch
            src = planes_of(ctx.export(pics[i % P], layout, **kw))
            for s, d in zip(src, dst):
                if layout == "rgb":
                    x, hw = s.float()[None], d.shape[1:]
                elif s.dim() == 3:                          # semi-planar CbCr [H, W, 2]
                    x, hw = s.permute(2, 0, 1).float()[None], d.shape[:2]
                else:
                    x, hw = s.float()[None, None], d.shape
                y = F.interpolate(x, size=tuple(hw), **TORCH_MODE[filt]).round_().clamp_(0, (1 << bd) - 1)
                if msb:
                    y = y * (1 << (16 - bd))
                y.to(torch.int32).to(d.dtype if d.dtype == torch.uint8 else torch.int16)

        for _ in range(10):
            fused(0)
            torch_path(0)
        torch.cuda.synchronize()
        f_us, t_us = [], []
        for r in range(3):                                  # alternated
            f_us.append(time_events(fused, a.iters))
            t_us.append(time_events(torch_path, max(10, a.iters // 10)))
        read = 2 * (w * h + 2 * (w // 2) * (h // 2))
        written = sum(d.numel() * d.element_size() for d in dst)
        us = statistics.median(f_us)
        out[name] = {"source": "%dx%d" % (w, h), "size": list(size), "filter": filt, "layout": layout, "bit_depth": bd,
                     "bytes_read": read, "bytes_written": written, "us_per_export_events": round(us, 2),
                     "TBps_events": round((read + written) / (us * 1e-6) / 1e12, 3),
                     "fraction_of_8TBps_events": round((read + written) / (us * 1e-6) / PEAK, 3),
                     "torch_pipeline_us_per_picture": round(statistics.median(t_us), 2),
                     "fused_rounds_us": [round(x, 2) for x in f_us], "torch_rounds_us": [round(x, 2) for x in t_us]}
    for name, (w, h) in BASELINES:
        ctx, pics = ctxs[(w, h)]
        P = len(pics)
        dst = ctx.export(pics[0], "rgb", 8)
        for _ in range(10):
            ctx.export(pics[0], "rgb", 8, out=dst)
        us = time_events(lambda i: ctx.export(pics[i % P], "rgb", 8, out=dst), a.iters)
        read = 2 * (w * h + 2 * (w // 2) * (h // 2))
        out[name] = {"bytes_read": read, "bytes_written": 3 * w * h, "us_per_export_events": round(us, 2),
                     "fraction_of_8TBps_events": round((read + 3 * w * h) / (us * 1e-6) / PEAK, 3)}
    return out


def wall_per_call(ctxs, iters):
    import torch
    ctx, pics = ctxs[(3840, 2160)]
    res = {}
    out224 = ctx.export(pics[0], "rgb", 8, size=(224, 224), filter="bicubic")
    for name, kw in [("unscaled_rgb8", {}), ("scaled_rgb8_224_bicubic", dict(size=(224, 224), filter="bicubic")),
                     ("scaled_rgb8_224_bicubic_out", dict(size=(224, 224), filter="bicubic", out=out224))]:
        for _ in range(20):
            ctx.export(pics[0], "rgb", 8, **kw)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            for i in range(iters):
                ctx.export(pics[i % len(pics)], "rgb", 8, **kw)
            runs.append((time.perf_counter() - t0) * 1e6 / iters)
            torch.cuda.synchronize()
        res[name + "_us_per_call"] = round(statistics.median(runs), 2)
    return res


def decode(stream, threads, size):
    import torch
    n = 0
    with hmdec.Decoder(threads=threads, device_output=True) as d:
        t0 = time.perf_counter()
        kw = {} if size is None else dict(size=size)
        for _ in d.frames(stream, layout="rgb", **kw):
            n += 1
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), n


def split_trace(trace, iters, out):
    """per-case kernel times from the kernel trace CSV of a `--kernel-only --iters N` run (rocprofv3 --kernel-trace --output-format
    csv): the export launches in start order are, per case of CASES and then per baseline, 1 + N launches; the first of each group
    (the allocation call) is left out"""
    import csv
    rows = sorted((r for r in csv.DictReader(open(trace)) if "k_export" in r["Kernel_Name"]), key=lambda r: int(r["Start_Timestamp"]))
    names = [c[0] for c in CASES] + [b[0] for b in BASELINES]
    if len(rows) != len(names) * (iters + 1):
        raise SystemExit("%s: %d export launches, expected %d" % (trace, len(rows), len(names) * (iters + 1)))
    sizes = {c[0]: c for c in CASES}
    with open(out, "w") as f:
        f.write("case,kernel,launches,median_us,bytes,TBps,fraction_of_8TBps\n")
        for i, name in enumerate(names):
            seg = rows[i * (iters + 1) + 1:(i + 1) * (iters + 1)]
            us = statistics.median((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in seg)
            if name in sizes:
                _, (w, h), layout, bd, nbytes, msb, (oh, ow), _ = sizes[name]
                sub = (1, 1) if layout == "rgb" else (2, 2)
                written = nbytes * (3 * oh * ow if layout == "rgb" else oh * ow + 2 * (oh // sub[0]) * (ow // sub[1]))
            else:
                w, h = dict(BASELINES)[name]
                written = 3 * w * h
            nb = 2 * (w * h + 2 * (w // 2) * (h // 2)) + written
            f.write('%s,"%s",%d,%.1f,%d,%.2f,%.3f\n' % (name, seg[0]["Kernel_Name"], len(seg), us, nb, nb / (us * 1e-6) / 1e12,
                                                        nb / (us * 1e-6) / PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--pictures", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--split-trace", default=None, metavar="TRACE_CSV",
                    help="no GPU: write the per-case kernel times of a --kernel-only trace to --out (CSV) and stop")
    a = ap.parse_args()
    if a.split_trace:
        split_trace(a.split_trace, a.iters, a.out)
        return
    import torch
    torch.zeros(1, device="cuda")
    ctxs = {(w, h): make_context(w, h, a.pictures) for (w, h) in [(3840, 2160), (1920, 1080)]}
    if a.kernel_only:                                      # (for rocprofv3: every case and baseline, nothing else; see split_trace)
        for name, (w, h), layout, bd, nbytes, msb, size, filt in CASES:
            ctx, pics = ctxs[(w, h)]
            dst = ctx.export(pics[0], layout, bit_depth=bd, msb_aligned=bool(msb), size=size, filter=filt)
            for i in range(a.iters):
                ctx.export(pics[i % len(pics)], layout, bit_depth=bd, msb_aligned=bool(msb), size=size, filter=filt,
                           out=dst)
        for name, (w, h) in BASELINES:
            ctx, pics = ctxs[(w, h)]
            dst = ctx.export(pics[0], "rgb", 8)
            for i in range(a.iters):
                ctx.export(pics[i % len(pics)], "rgb", 8, out=dst)
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": True, "iters": a.iters}))
        return
    res = {"source_note": "%d distinct uploaded 3840x2160 Main10 4:2:0 pictures (%.0f MB of int16 planes) rotated per export, more than the "
                          "256 MiB Infinity Cache; the enlargement rotates %d 1920x1080 pictures" % (a.pictures, a.pictures * 3840 * 2160 * 3 / 1e6, a.pictures),
           "kernels": bench(a, ctxs), "python_wall": wall_per_call(ctxs, a.iters)}
    for c, _ in ctxs.values():
        c.close()
    with open(os.path.join(ROOT, "tests", "golden", "bench_ldp_wpp_main10_3840x2160.bin"), "rb") as f:
        stream = f.read()
    decode(stream, a.threads, (1080, 1920))                # (warm-up)
    full, scaled = [], []
    for _ in range(a.rounds):
        full.append(decode(stream, a.threads, None))
        scaled.append(decode(stream, a.threads, (1080, 1920)))
    res["decoder_bench_ldp_wpp_main10_3840x2160"] = {
        "threads": a.threads, "pictures": full[0][1], "rounds": a.rounds,
        "rgb_full_size_pictures_per_s": [round(x[0], 2) for x in full], "rgb_1080p_bilinear_pictures_per_s": [round(x[0], 2) for x in scaled],
        "rgb_full_size_median": round(statistics.median(x[0] for x in full), 2),
        "rgb_1080p_bilinear_median": round(statistics.median(x[0] for x in scaled), 2)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
