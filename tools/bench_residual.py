"""Times the residual export (hmgpu_pictures_export_residual) on one GPU: sixteen synthetic 1920x1080 B pictures,
PLANES with all three components and DENSE 224x224 float16 with random-resized-crop windows, beside the pixel exports of the same
batch (unscaled uint8 RGB, and 224x224 float16 RGB nearest with the same windows).  Device time per call from torch events around K
back-to-back calls on torch's current stream (the per-call event pair in and out included), the cases alternating in one process,
R rounds; prints one JSON line and writes it to --out.

    python tools/bench_residual.py [--rounds 5] [--calls 50] [--out profiles/residual_bench.json]"""
import argparse
import json
import os
import sys

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
    from libhm_amd import abi, export
    from tests import synth
    w, h, n = 1920, 1080, 16
    seq = abi.make_seq(w, h, 10, 10, max_pictures=n + 2)
    gen = torch.Generator().manual_seed(7)
    windows, flips = export.random_resized_crop(n, w, h, generator=gen)
    sc = (1.0 / 512, 1.0 / 512, 1.0 / 512)
    with libhm_amd.Context(seq) as ctx:
        for k in range(2):
            assert ctx.acquire() == k
            ctx.upload(k, synth.noise_planes(w, h, 10, 1 + k))
        pics = []
        for i in range(n):
            p = synth.make_picture(w, h, 10, seed=900 + i, bi=True, intra_frac=0.1, num_refs=2, ref_handles=([0, 1], [1]))
            hnd = ctx.acquire()
            ctx.decompress_pictures([(hnd, p.slices, p.meta, p.coeffs)])
            ctx.filter_pictures([(hnd, p.pp, abi.sao_array_from_raw(p.sao_raw))])
            pics.append(hnd)
        ctx.sync()
        out_p = ctx.export_residual(pics, "planes")
        out_d = ctx.export_residual(pics, "dense", size=(224, 224), windows=windows, flip=flips, dtype=torch.float16, scale=sc)
        out_u8 = ctx.export_batch(pics, "rgb", 8)
        out_px = ctx.export_batch(pics, "rgb", 8, size=(224, 224), filter="nearest", windows=windows, flip=flips, dtype=torch.float16)
        cases = {
            "residual_planes": lambda: ctx.export_residual(pics, "planes", out=out_p),
            "residual_dense_224_f16": lambda: ctx.export_residual(pics, "dense", size=(224, 224), windows=windows, flip=flips, dtype=torch.float16,
                                                                  scale=sc, out=out_d),
            "pixels_unscaled_u8_rgb": lambda: ctx.export_batch(pics, "rgb", 8, out=out_u8),
            "pixels_224_f16_rgb_nearest_windows": lambda: ctx.export_batch(pics, "rgb", 8, size=(224, 224), filter="nearest", windows=windows,
                                                                           flip=flips, dtype=torch.float16, out=out_px),
        }
        times = {k: [] for k in cases}
        for rnd in range(a.rounds + 1):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:                                              # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        # algorithmic bytes per call.  PLANES: per sample of a component 2 bytes of tile read and 2 written (1.5 samples per luma sample in
        # 4:2:0), plus six bytes of the arrays per 4x4 luma partition (part_size, pred_mode, depth, tr_idx, cbf, ipcm) for luma and for
        # each chroma component per 8x8 area.  DENSE: 3 x 2 bytes written per output sample; the reads are at most one 16-byte slot and
        # twelve array bytes per component and sample.
        parts = (w // 4) * (h // 4)
        bytes_ = {"residual_planes": n * (w * h * 3 // 2 * 4 + parts * 6 + 2 * (parts // 4) * 6), "residual_dense_224_f16": n * 224 * 224 * 6,
                  "pixels_unscaled_u8_rgb": n * (w * h * 3 + w * h * 3), "pixels_224_f16_rgb_nearest_windows": None}
        res = {"pictures": n, "width": w, "height": h, "rounds": a.rounds, "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0),
               "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": bytes_[name],
                                  "share_of_8TBps": None if bytes_[name] is None else round(bytes_[name] / (med * 1e-6) / 8e12, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
