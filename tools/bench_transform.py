"""Times the transform export (hmgpu_pictures_export_transform) on one GPU: sixteen synthetic 1920x1080 4:2:0 10-bit B
pictures, all three components and the info grid -- the levels, the coefficients with flat scaling, the coefficients with scaling
lists, the coefficients as float16 -- beside the residual planes (k_residual_planes) of the same pictures in the same run.  Device
time per call from torch events around K back-to-back calls on torch's current stream, the cases alternating in one process, R rounds;
prints one JSON line and writes it to --out.

    python tools/bench_transform.py [--rounds 5] [--calls 50] [--out profiles/transform_bench.json]"""
import argparse
import ctypes as C
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
    from libhm_amd import abi
    from tests import synth
    w, h, n = 1920, 1080, 16
    seq = abi.make_seq(w, h, 10, 10, max_pictures=2 * n + 2)
    rng = np.random.RandomState(0x5CA1)
    lists = abi.ScalingLists()
    for sz in range(4):
        for l in range(6):
            lists.dc[sz][l] = int(rng.randint(1, 256)) if sz >= 2 else 16
            for i in range(64):
                lists.coef[sz][l][i] = int(rng.randint(1, 256)) if i < (16 if sz == 0 else 64) else 16
    with libhm_amd.Context(seq) as ctx:
        for k in range(2):
            assert ctx.acquire() == k
            ctx.upload(k, synth.noise_planes(w, h, 10, 1 + k))
        flat, listed, coded = [], [], 0
        for i in range(n):
            p = synth.make_picture(w, h, 10, seed=900 + i, bi=True, intra_frac=0.1, num_refs=2, ref_handles=([0, 1], [1]))
            coded += int((synth.coded_blocks(p.meta_np, 1, 6)[:, 3] ** 2).sum())
            for handles, use_lists in ((flat, False), (listed, True)):
                for sl in p.slices:
                    sl.scaling_lists = C.pointer(lists) if use_lists else None
                hnd = ctx.acquire()
                ctx.decompress_pictures([(hnd, p.slices, p.meta, p.coeffs)])
                handles.append(hnd)
        ctx.sync()
        out_i = ctx.export_transform(flat, "levels")
        out_f = ctx.export_transform(flat, "coeffs", dtype=torch.float16, scale=(1.0 / 512,) * 3)
        out_r = ctx.export_residual(flat, "planes")
        cases = {
            "transform_levels": lambda: ctx.export_transform(flat, "levels", out=out_i),
            "transform_coeffs_flat": lambda: ctx.export_transform(flat, "coeffs", out=out_i),
            "transform_coeffs_lists": lambda: ctx.export_transform(listed, "coeffs", out=out_i),
            "transform_coeffs_flat_f16": lambda: ctx.export_transform(flat, "coeffs", dtype=torch.float16, scale=(1.0 / 512,) * 3, out=out_f),
            "residual_planes": lambda: ctx.export_residual(flat, "planes", out=out_r),
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
        # algorithmic bytes per call.  Transform: 2 bytes written per component sample (1.5 per luma sample in 4:2:0), 2 bytes of levels
        # read per element of a coded block (`coded`, counted from the arrays), per 4x4 luma partition twelve bytes of the arrays read by
        # the luma and by the chroma workgroup each and six info bytes written; with lists one byte per coded position more.
        # Residual planes: as tools/bench_residual.py.
        parts = (w // 4) * (h // 4)
        base = n * (w * h * 3 // 2 * 2 + parts * (2 * 12 + 6)) + coded * 2
        bytes_ = {"transform_levels": base, "transform_coeffs_flat": base, "transform_coeffs_lists": base + coded, "transform_coeffs_flat_f16": base,
                  "residual_planes": n * (w * h * 3 // 2 * 4 + parts * 6 + 2 * (parts // 4) * 6)}
        res = {"pictures": n, "width": w, "height": h, "rounds": a.rounds, "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0),
               "coded_elements": coded, "cases": {}}
        ref = float(np.median(times["residual_planes"]))
        for name, t in times.items():
            med = float(np.median(t))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": bytes_[name],
                                  "share_of_8TBps": round(bytes_[name] / (med * 1e-6) / 8e12, 4), "ratio_to_residual_planes": round(med / ref, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
