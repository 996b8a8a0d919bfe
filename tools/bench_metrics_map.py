"""Times the picture metric maps (hmgpu_pictures_metrics_map) on one GPU with the inputs of tools/bench_metrics.py:
sixteen 3840x2160 4:2:0 10-bit pictures against sixteen other pictures of the context and against uint16 planes, blocks of 8, 16 and
64, with SSIM and without -- beside hmgpu_pictures_metrics with the same description in the same process, and beside what a user had
before the call existed: export_batch of both sets to planar uint16 tensors plus the torch expression for the SSE per block of every
plane (reshape and sum; no other field).  Before anything is timed one picture of each case is held against the model.  Device time
per call from torch events around K back-to-back calls on torch's current stream, the cases alternating in one process, R rounds
after one that warms up; prints one JSON line and writes it to --out.  Kernel times come from a run of their own under
rocprofv3 --kernel-trace --stats (the kernels are k_metrics_map<reference, ssim> and k_metrics<reference, ssim>).

    python tools/bench_metrics_map.py [--rounds 5] [--calls 20] [--out profiles/metrics_map_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS = (8, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import libhm_amd
    from libhm_amd import abi, metrics
    from tests import metrics_map_ref as mmap
    from tests import metrics_ref as mref
    w, h, n, bd = a.width, a.height, 16, 10
    seq = abi.make_seq(w, h, bd, bd, max_pictures=2 * n + 2)
    rng = np.random.RandomState(11)
    base = [[rng.randint(0, 1 << bd, size=(h >> s, w >> s)).astype(np.int16) for s in (0, 1, 1)] for _ in range(4)]
    other = [[np.clip(p.astype(np.int32) + rng.randint(-40, 41, size=p.shape), 0, (1 << bd) - 1).astype(np.int16) for p in planes] for planes in base]
    with libhm_amd.Context(seq) as ctx:
        pics, refs = [], []
        for i in range(n):
            for planes, into in ((base[i % 4], pics), (other[i % 4], refs)):
                hnd = ctx.acquire()
                ctx.upload(hnd, planes)
                into.append(hnd)
        ctx.sync()
        planes16 = ctx.export_batch(refs, "planar", bd)                  # the reference as uint16 planes [16, h_c, w_c]
        torch.cuda.synchronize()
        # one picture of each case against the model, so that what is timed is known to be right
        for B in BLOCKS:
            want = mmap.picture(base[0], other[0], 1, (bd, bd), B)
            for ssim in (True, False):
                for key, kw in (("pictures", dict(ref_pics=refs[:1])), ("planes", dict(ref=[t[:1] for t in planes16]))):
                    got = metrics.maps(ctx.metrics_map(pics[:1], block=B, ssim=ssim, **kw)).cpu().numpy()[0]
                    assert np.array_equal(got[:, :4], want[:, :4]), (B, ssim, key)
                    if ssim:
                        d = np.abs(got[:, 4] - want[:, 4])
                        assert np.array_equal(got[:, 5], want[:, 5]) and (d <= 1 + want[:, 5] // 1024).all(), (B, key, int(d.max()))
                        assert all(abs(int((got[k, 4] - want[k, 4]).sum())) <= mref.tolerance(int(want[k, 5].sum())) for k in range(3)), (B, key)
        out_a, out_b = ctx.export_batch(pics, "planar", bd), ctx.export_batch(refs, "planar", bd)

        def blocks_sse(x, y, bw, bh):
            """((x - y) ** 2) per block by reshape-sum; the planes are whole blocks here or padded to them"""
            d = (x.to(torch.int32) - y.to(torch.int32)) ** 2
            ph, pw = -d.shape[1] % bh, -d.shape[2] % bw
            if ph or pw:
                d = torch.nn.functional.pad(d, (0, pw, 0, ph))
            return d.reshape(d.shape[0], d.shape[1] // bh, bh, d.shape[2] // bw, bw).sum(dim=(2, 4), dtype=torch.int64)

        def before(B):
            def run():
                ea, eb = ctx.export_batch(pics, "planar", bd, out=out_a), ctx.export_batch(refs, "planar", bd, out=out_b)
                return [blocks_sse(x, y, B >> (1 if k else 0), B >> (1 if k else 0)) for k, (x, y) in enumerate(zip(ea, eb))]
            return run
        for B in BLOCKS:                                                 # the two ways agree on the SSE of every block
            sse = torch.stack(before(B)(), dim=1)
            assert bool((sse == metrics.maps(ctx.metrics_map(pics, ref_pics=refs, block=B, ssim=False))[:, :, 0]).all()), B
        cases = {}
        for ssim in (True, False):
            tag = "_ssim" if ssim else ""
            cases["metrics_pictures" + tag] = lambda ssim=ssim: ctx.metrics(pics, ref_pics=refs, ssim=ssim)
            cases["metrics_planes_u16" + tag] = lambda ssim=ssim: ctx.metrics(pics, ref=planes16, ssim=ssim)
            for B in BLOCKS:
                cases["map%d_pictures%s" % (B, tag)] = lambda ssim=ssim, B=B: ctx.metrics_map(pics, ref_pics=refs, block=B, ssim=ssim)
                cases["map%d_planes_u16%s" % (B, tag)] = lambda ssim=ssim, B=B: ctx.metrics_map(pics, ref=planes16, block=B, ssim=ssim)
        for B in BLOCKS:
            cases["before_export_both_and_torch_sse_blocks%d" % B] = before(B)
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
                if rnd:                                                  # (round 0 warms up)
                    times[name].append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        # algorithmic bytes per call: 2 bytes of the picture and 2 of the reference per sample, 1.5 samples per luma sample in 4:2:0,
        # plus the maps: 3 components x fields x 8 bytes per block
        samples = n * w * h * 3 // 2
        res = {"pictures": n, "width": w, "height": h, "bit_depth": bd, "rounds": a.rounds, "calls_per_round": a.calls,
               "device": torch.cuda.get_device_name(0), "cases": {}}
        for name, t in times.items():
            med = float(np.median(t))
            nbytes = None
            if name.startswith("metrics"):
                nbytes = samples * 4
            elif name.startswith("map"):
                B = int(name[3:name.index("_")])
                nbytes = samples * 4 + n * 3 * (6 if name.endswith("_ssim") else 4) * 8 * (-(-w // B)) * (-(-h // B))
            res["cases"][name] = {"us_per_call_median": round(med, 2), "us_per_call_min": round(float(min(t)), 2),
                                  "us_per_call_max": round(float(max(t)), 2), "algorithmic_bytes": nbytes,
                                  "share_of_8TBps": None if nbytes is None else round(nbytes / (med * 1e-6) / 8e12, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
