"""Device export measurements, one JSON object on stdout:

  (i)  k_export on a 3840x2160 Main10 4:2:0 picture uploaded to the device, for each layout at 8 bits and as P010 (10 bits,
       MSB-aligned): device time per export from torch events (the kernel time itself comes from a separate
       `rocprofv3 --kernel-trace --stats` run of `--kernel-only`), bytes from the shapes (visible int16 planes read + bytes
       written), GB/s and the fraction of the 8 TB/s peak
  (ii) the whole decoder on tests/golden/bench_ldp_wpp_main10_3840x2160.bin: host output (libHMDec_get_picture downloads the
       planes) against device output + Picture.export("rgb"); pictures/s alternated in one process, `--rounds` rounds, median;
       hmdec_download_bytes of each

usage: python tools/bench_export.py [--iters N] [--rounds R] [--threads T] [--kernel-only] [--out FILE]
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
CASES = [("planar_8", abi.EXPORT_PLANAR, 8, 1, 0), ("semiplanar_8", abi.EXPORT_SEMIPLANAR, 8, 1, 0), ("rgb_8", abi.EXPORT_RGB, 8, 1, 0),
         ("planar_p010", abi.EXPORT_PLANAR, 10, 2, 1), ("semiplanar_p010", abi.EXPORT_SEMIPLANAR, 10, 2, 1), ("rgb_p010", abi.EXPORT_RGB, 10, 2, 1)]


def bench_kernel(iters):
    import torch
    w, h = 3840, 2160
    seq = abi.make_seq(w, h, 10, 10, max_pictures=2)
    rng = np.random.default_rng(1)
    planes = [rng.integers(0, 1024, (h, w)).astype(np.int16)] + [rng.integers(0, 1024, (h // 2, w // 2)).astype(np.int16) for _ in range(2)]
    read = 2 * (w * h + 2 * (w // 2) * (h // 2))
    out = {}
    with libhm_amd.Context(seq) as ctx:
        pic = ctx.acquire()
        ctx.upload(pic, planes)
        stream = torch.cuda.current_stream().cuda_stream
        for name, layout, bd, nbytes, msb in CASES:
            desc = abi.make_export_desc(layout, bd, nbytes, msb, (0, 0, 0, 0), 1, 0)
            plan = libhm_amd.export_plan(seq, desc)
            bufs = [torch.empty((plan.height[k], plan.row_bytes[k]), dtype=torch.uint8, device="cuda") for k in range(plan.planes)]
            ptrs, pitches = [b.data_ptr() for b in bufs], [plan.row_bytes[k] for k in range(plan.planes)]
            for _ in range(10):
                ctx.export_into(pic, desc, ptrs, pitches, 1, stream)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                ctx.export_into(pic, desc, ptrs, pitches, 1, stream)
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / iters
            written = sum(plan.row_bytes[k] * plan.height[k] for k in range(plan.planes))
            out[name] = {"ms_per_export": round(ms, 4), "bytes_read": read, "bytes_written": written,
                         "GBps": round((read + written) / (ms * 1e-3) / 1e9, 1), "fraction_of_8TBps": round((read + written) / (ms * 1e-3) / PEAK, 3)}
    return out


def decode_host(stream, threads):
    n = [0]
    with hmdec.Decoder(threads=threads) as d:
        t0 = time.perf_counter()

        def on_output(p):
            for c in range(3):
                lib = hmdec.lib()
                assert lib.libHMDEC_get_image_plane(p.h, c)
            n[0] += 1
        d.decode_stream(stream, on_output=on_output)
        dt = time.perf_counter() - t0
        return n[0] / dt, d.download_bytes, n[0]


def decode_device(stream, threads):
    import torch
    n = 0
    with hmdec.Decoder(threads=threads, device_output=True) as d:
        t0 = time.perf_counter()
        for _, t in d.frames(stream, layout="rgb"):
            n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return n / dt, d.download_bytes, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    res = {"kernel_2160p_main10_420": bench_kernel(a.iters)}
    if not a.kernel_only:
        with open(os.path.join(ROOT, "tests", "golden", "bench_ldp_wpp_main10_3840x2160.bin"), "rb") as f:
            stream = f.read()
        decode_device(stream, a.threads)                # (warm-up: code objects, allocator)
        host, dev = [], []
        for _ in range(a.rounds):
            host.append(decode_host(stream, a.threads))
            dev.append(decode_device(stream, a.threads))
        res["decoder_bench_ldp_wpp_main10_3840x2160"] = {
            "threads": a.threads, "pictures": host[0][2], "rounds": a.rounds,
            "host_output_pictures_per_s": [round(x[0], 2) for x in host], "device_rgb_export_pictures_per_s": [round(x[0], 2) for x in dev],
            "host_output_median": round(statistics.median(x[0] for x in host), 2),
            "device_rgb_export_median": round(statistics.median(x[0] for x in dev), 2),
            "host_output_download_bytes": host[0][1], "device_output_download_bytes": dev[0][1]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
