"""Times error concealment (hmgpu_pictures_conceal) on one GPU: sixteen 3840x2160 4:2:0 10-bit pictures per call,
every CTU masked, COPY and MOTION, each picture from a source of its own (sixteen decoded pictures whose motion arrays are
resident), beside a device-to-device copy of the same number of plane bytes in the same process (a contiguous tensor copy on the
same stream: one hipMemcpyAsync).  Device time per call from events on the context's stream around K back-to-back calls; the cases
alternate, R rounds after a warm-up round; prints one JSON line and writes it to --out.  These are call times -- the concealment
kernel and the margin pass behind it --, not kernel times.

    python tools/bench_conceal.py [--rounds 5] [--calls 20] [--out profiles/conceal_bench.json]"""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libhm_amd
    from libhm_amd import abi
    from tests import synth
    w, h, bd, n = 3840, 2160, 10, 16
    p = synth.make_picture(w, h, bd, seed=5, ref_handles=([0], [0]), intra_frac=0.05)
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    seq.max_pictures = 2 * n + 1
    plane_bytes = n * (w * h + 2 * (w // 2) * (h // 2)) * 2
    with libhm_amd.Context(seq) as ctx:
        ref = ctx.acquire()
        ctx.upload(ref, synth.noise_planes(w, h, bd, 1))
        srcs, dsts = [ctx.acquire() for _ in range(n)], [ctx.acquire() for _ in range(n)]
        start = synth.noise_planes(w, h, bd, 2)
        for k in srcs:
            ctx.upload(k, start)
        ctx.decompress_pictures([(k, p.slices, p.meta, p.coeffs) for k in srcs])
        ctx.filter_pictures([(k, p.pp, abi.sao_array_from_raw(p.sao_raw)) for k in srcs])
        for k in dsts:
            ctx.upload(k, start)
        ctx.sync()
        stream = torch.cuda.ExternalStream(ctx.stream_handle())
        a_buf = torch.empty(plane_bytes, dtype=torch.uint8, device="cuda")
        b_buf = torch.zeros(plane_bytes, dtype=torch.uint8, device="cuda")

        def jobs(mode):
            return [dict(dst=d, src=s, mode=mode, dst_poc=108, src_poc=104) for d, s in zip(dsts, srcs)]

        def copy():
            with torch.cuda.stream(stream):
                a_buf.copy_(b_buf, non_blocking=True)

        cases = {"conceal_copy": lambda: ctx.conceal(jobs("copy")), "conceal_motion": lambda: ctx.conceal(jobs("motion")), "memcpy_d2d": copy}
        times = {k: [] for k in cases}
        for rnd in range(a.rounds + 1):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(stream)
                for _ in range(a.calls):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                ctx.sync()
                if rnd:                                              # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        res = {"pictures": n, "width": w, "height": h, "bit_depth": bd, "rounds": a.rounds, "calls_per_round": a.calls,
               "device": torch.cuda.get_device_name(0), "plane_bytes": plane_bytes, "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2)}
        base = res["cases"]["memcpy_d2d"]["us_per_call_median"]
        for name in ("conceal_copy", "conceal_motion"):
            res["cases"][name]["ratio_to_memcpy"] = round(res["cases"][name]["us_per_call_median"] / base, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
