"""Times the loop-filter export (hmgpu_pictures_export_loopfilter) on one GPU: synthetic 3840x2160 4:2:0 10-bit B
pictures, sixteen per call and one per call -- the edge grid, both grids, and the dense form (the whole picture unscaled, uint8) --
beside the BLOCKS form of the motion export (k_motion_blocks, the nearest sibling by shape: one small record read and a few stores
per 8x8 area) of the same pictures in the same run.  Four pictures are drawn and decoded into four handles each.  Device time per
call from torch events around K back-to-back calls on torch's current stream, the cases alternating in one process, R rounds; prints
one JSON line with the bytes written per second of every case and writes it to --out.  No threshold: a measurement, not a test.

    python tools/bench_loopfilter.py [--rounds 5] [--calls 50] [--out profiles/loopfilter_bench.json]"""
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
    from libhm_amd import abi
    from tests import synth
    w, h, n, drawn = 3840, 2160, 16, 4
    seq = abi.make_seq(w, h, 10, 10, max_pictures=n + 2)
    with libhm_amd.Context(seq) as ctx:
        for k in range(2):
            assert ctx.acquire() == k
            ctx.upload(k, synth.noise_planes(w, h, 10, 1 + k))
        pics = [None] * n
        for i in range(drawn):
            p = synth.make_picture(w, h, 10, seed=900 + i, bi=True, intra_frac=0.1, num_refs=2, ref_handles=([0, 1], [1]))
            for k in range(i, n, drawn):
                hnd = ctx.acquire()
                ctx.decompress_pictures([(hnd, p.slices, p.meta, p.coeffs)])
                ctx.filter_pictures([(hnd, p.pp, abi.sao_array_from_raw(p.sao_raw))])
                pics[k] = hnd
        ctx.sync()
        cases, bytes_ = {}, {}
        blocks = (w // 4) * (h // 4)
        for count in (n, 1):
            hs = pics[:count]
            out_e = ctx.export_loopfilter(hs, grids=("edge",))
            out_g = ctx.export_loopfilter(hs)
            out_d = ctx.export_loopfilter(hs, "dense")
            out_m = ctx.export_motion(hs, "blocks")
            tag = "_x%d" % count
            cases["edge_grid" + tag] = lambda hs=hs, o=out_e: ctx.export_loopfilter(hs, grids=("edge",), out=o)
            cases["both_grids" + tag] = lambda hs=hs, o=out_g: ctx.export_loopfilter(hs, out=o)
            cases["dense_u8" + tag] = lambda hs=hs, o=out_d: ctx.export_loopfilter(hs, "dense", out=o)
            cases["motion_blocks" + tag] = lambda hs=hs, o=out_m: ctx.export_motion(hs, "blocks", out=o)
            # bytes written per call: thirteen int16 per block; + eighteen int8 per CTB; three uint8 per sample; 8 + 8 + 4 per block
            bytes_["edge_grid" + tag] = count * blocks * 26
            bytes_["both_grids" + tag] = count * (blocks * 26 + 18 * ctx.num_ctus)
            bytes_["dense_u8" + tag] = count * w * h * 3
            bytes_["motion_blocks" + tag] = count * blocks * 20
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
        res = {"width": w, "height": h, "rounds": a.rounds, "calls_per_round": a.calls, "device": torch.cuda.get_device_name(0), "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "bytes_written": bytes_[name],
                                  "written_GBps": round(bytes_[name] / (med * 1e-6) / 1e9, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
