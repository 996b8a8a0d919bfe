"""Times the picture import (hmgpu_pictures_import) on one GPU: sixteen 1920x1080 pictures per call from planar uint8
4:2:0, NV12, RGB uint8 planes and packed RGB float16, beside the only way in there was before: hmgpu_picture_upload of the same
sixteen pictures from page-locked host memory, one call and one wait per picture.  Import: device time per call from torch events
around K back-to-back calls on torch's current stream (the per-call event pair in and out included).  Upload: wall time of the
sixteen synchronous calls (each ends in a stream synchronisation, so wall time is what a caller pays).  The cases alternate in one
process, R rounds after a warm-up round; prints one JSON line and writes it to --out.  These are call times, not kernel times.

    python tools/bench_import.py [--rounds 5] [--calls 50] [--out profiles/import_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libhm_amd
    from libhm_amd import abi
    w, h, n = 1920, 1080, 16
    seq = abi.make_seq(w, h, 8, 8, max_pictures=n)
    gen = torch.Generator(device="cuda").manual_seed(7)

    def rand(shape, dtype=torch.uint8):
        if dtype == torch.uint8:
            return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
        return torch.rand(shape, device="cuda", generator=gen).to(dtype)

    with libhm_amd.Context(seq) as ctx:
        pics = [ctx.acquire() for _ in range(n)]
        planar = (rand((n, h, w)), rand((n, h // 2, w // 2)), rand((n, h // 2, w // 2)))
        nv12 = (rand((n, h, w)), rand((n, h // 2, w // 2, 2)))
        rgb = rand((n, 3, h, w))
        px16 = rand((n, h, w, 3), torch.float16)
        # the yardstick: int16 planes in page-locked memory, as hmgpu_picture_upload takes them
        ysz, csz = w * h * 2, (w // 2) * (h // 2) * 2
        pinned = libhm_amd.PinnedBuffer(n * (ysz + 2 * csz))
        host = []
        rng = np.random.default_rng(7)
        for i in range(n):
            base = i * (ysz + 2 * csz)
            pl = [pinned.array[base:base + ysz].view(np.int16).reshape(h, w),
                  pinned.array[base + ysz:base + ysz + csz].view(np.int16).reshape(h // 2, w // 2),
                  pinned.array[base + ysz + csz:base + ysz + 2 * csz].view(np.int16).reshape(h // 2, w // 2)]
            for p in pl:
                p[...] = rng.integers(0, 256, p.shape)
            host.append(pl)

        def upload_all():
            for p, pl in zip(pics, host):
                ctx.upload(p, pl)

        cases = {
            "import_planar_u8_420": lambda: ctx.import_batch(pics, planar, layout="planar", bit_depth=8),
            "import_nv12": lambda: ctx.import_batch(pics, nv12, layout="semiplanar", bit_depth=8),
            "import_rgb_u8_planes": lambda: ctx.import_batch(pics, rgb, layout="rgb", bit_depth=8),
            "import_rgb_f16_packed": lambda: ctx.import_batch(pics, px16, layout="rgb", pixel="rgb", bit_depth=8),
        }
        times = {k: [] for k in cases}
        times["upload_16_pinned_int16"] = []
        for rnd in range(a.rounds + 1):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ctx.sync()
                if rnd:                                              # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
                reps = max(1, a.calls // 10)
                t0 = time.perf_counter()
                for _ in range(reps):
                    upload_all()
                t1 = time.perf_counter()
                if rnd:
                    times["upload_16_pinned_int16"].append((t1 - t0) * 1e6 / reps)
        # algorithmic bytes per call: every source element read once, every sample of the pictures written once as int16
        written = n * (w * h + 2 * (w // 2) * (h // 2)) * 2
        bytes_ = {"import_planar_u8_420": n * (w * h * 3 // 2) + written, "import_nv12": n * (w * h * 3 // 2) + written,
                  "import_rgb_u8_planes": n * w * h * 3 + written, "import_rgb_f16_packed": n * w * h * 6 + written,
                  "upload_16_pinned_int16": n * (w * h * 3 // 2) * 2 + written}
        res = {"pictures": n, "width": w, "height": h, "rounds": a.rounds, "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0),
               "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": bytes_[name],
                                  "share_of_8TBps": round(bytes_[name] / (med * 1e-6) / 8e12, 4),
                                  "clock": "wall, 16 calls" if name.startswith("upload") else "device, 1 call"}
        pinned.free()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
