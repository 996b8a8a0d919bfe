"""Colour export measurements, one JSON object on stdout.

Sources: 16 distinct uploaded 3840x2160 Main10 4:2:0 pictures, as tools/bench_export_pixels.py uses.  Two workloads -- unscaled uint8
packed RGB, and 224x224 float16 [N, 3, H, W] with random-resized-crop windows -- each through LUTs of 17, 33 and 65 nodes per axis,
with and without a shaper (seeded random nodes: the cost of a lookup does not depend on what the nodes hold, only on where the
pixels land).  `--content noise`: random samples, whose pixels land everywhere in the table -- the worst case for the caches;
`--content smooth`: slow ramps in Y, Cb and Cr with three bits of noise, where neighbouring pixels hit neighbouring nodes as in
camera material.  The shaper is random under noise and a monotone curve (a square root) under smooth: a random shaper scatters
neighbouring pixels over the table whatever the picture holds.  Per case three paths alternate in one
process, `--rounds` rounds of `--iters` batches each, wall time per batch from torch events around the calls, the median round
reported and every round kept:
  colour:  Context.export_batch(lut=) into a preallocated tensor;
  plain:   the same call without lut= (what the stage adds);
  torch:   the plain export of the integers, then the index arithmetic of the colour stage as tensor operations (what a consumer
           had to write before), `--torch-iters` batches per round.
The colour path and the torch path write the same bytes (checked).
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
from libhm_amd import abi, export  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, N, DEPTH = 3840, 2160, 16, 8
WORKLOADS = [("rgb_u8_unscaled", None), ("f16_224_bilinear_rrc", (224, 224))]
LUTS = [(17, False), (17, True), (33, False), (33, True), (65, False), (65, True)]


def make_context(n, content):
    seq = abi.make_seq(W, H, 10, 10, max_pictures=n)
    ctx = libhm_amd.Context(seq)
    rng = np.random.default_rng(W)
    pics = []
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        p = ctx.acquire()
        if content == "noise":
            base = rng.integers(0, 1024, (H, W)).astype(np.int16)
            planes = [base, base[::2, ::2].copy(), base[1::2, 1::2].copy()]
        else:
            noise = rng.integers(0, 8, (H, W))
            planes = [((xx + 2 * yy) // 8 + 37 * i + noise) % 1024, ((xx[::2, ::2] // 5 + 11 * i + noise[::2, ::2]) % 1024),
                      ((yy[::2, ::2] // 3 + 23 * i + noise[1::2, 1::2]) % 1024)]
            planes = [np.ascontiguousarray(v, np.int16) for v in planes]
        ctx.upload(p, planes)
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


def torch_lut(rgb, lattice, shaper, size):
    """the colour stage on integer tensors rgb [3][...] (int64): shaper or bit replication, cell and fraction, the tetrahedron by
    sorted fractions, four gathers of [L^3, 3] nodes, the rounded sum"""
    import torch
    if shaper is not None:
        u = [shaper[c][rgb[c]] for c in range(3)]
    else:
        u = [(v << (16 - DEPTH)) | (v >> (2 * DEPTH - 16)) for v in rgb]
    t = [v * (size - 1) for v in u]
    i = torch.stack([v >> 16 for v in t])
    f = torch.stack([v & 0xffff for v in t])
    fs, order = torch.sort(f, dim=0, descending=True, stable=True)
    step = torch.tensor([1, size, size * size], device=f.device)[order]
    idx = i[0] + size * (i[1] + size * i[2])
    w = (65536 - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2])
    acc = w[0].unsqueeze(-1) * lattice[idx]
    for k in range(3):
        idx = idx + step[k]
        acc = acc + w[k + 1].unsqueeze(-1) * lattice[idx]
    return (acc + 32768) >> 16                                        # [..., 3]


def paths(ctx, pics, size, lut, tables):
    import torch
    lattice, shaper = tables
    L = lattice.shape[0]
    lat_t = torch.from_numpy(lattice.reshape(-1, 3).astype(np.int64)).cuda()
    sh_t = None if shaper is None else torch.from_numpy(shaper.astype(np.int64)).cuda()
    if size is None:
        kw = dict(pixel="rgb")
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device="cuda")
        ints = torch.empty((N, 3, H, W), dtype=torch.uint8, device="cuda")

        def restated():
            ctx.export_batch(pics, "rgb", DEPTH, out=ints)
            res = torch.empty_like(out)
            for b in range(N):                                        # (picture by picture: the temporaries of all sixteen do not fit)
                res[b] = torch_lut([ints[b, c].long() for c in range(3)], lat_t, sh_t, L).to(torch.uint8)
            return res
    else:
        w, f = export.random_resized_crop(N, W, H, generator=torch.Generator().manual_seed(1), chroma_format=1)
        kw = dict(size=size, filter="bilinear", windows=w, flip=f, dtype=torch.float16, mean=MEAN, std=STD)
        out = torch.empty((N, 3) + size, dtype=torch.float16, device="cuda")
        ints = torch.empty((N, 3) + size, dtype=torch.uint8, device="cuda")
        sc, bi = export.affine(DEPTH, MEAN, STD)
        sc_t = torch.tensor([float(v) for v in sc], device="cuda").view(1, 3, 1, 1)
        bi_t = torch.tensor([float(v) for v in bi], device="cuda").view(1, 3, 1, 1)

        def restated():
            ctx.export_batch(pics, "rgb", DEPTH, out=ints, size=size, filter="bilinear", windows=w, flip=f)
            v = torch_lut([ints[:, c].long() for c in range(3)], lat_t, sh_t, L).permute(0, 3, 1, 2)
            return (v.float() * sc_t + bi_t).to(torch.float16)

    def colour():
        ctx.export_batch(pics, "rgb", DEPTH, out=out, lut=lut, **kw)

    def plain():
        ctx.export_batch(pics, "rgb", DEPTH, out=out, **kw)
    return colour, plain, restated, out


def bench(a, ctx, pics):
    import torch
    res = {}
    rng = np.random.default_rng(7)
    for name, size in WORKLOADS:
        for L, with_shaper in LUTS:
            lattice = rng.integers(0, 1 << DEPTH, (L, L, L, 3)).astype(np.uint16)
            shaper = None
            if with_shaper and a.content == "noise":
                shaper = rng.integers(0, 65536, (3, 1 << DEPTH)).astype(np.uint16)
            elif with_shaper:
                curve = np.sqrt(np.arange(1 << DEPTH) / float((1 << DEPTH) - 1))
                shaper = np.tile(np.floor(curve * 65535 + 0.5).astype(np.uint16), (3, 1))
            with ctx.colour_lut(lattice, shaper, DEPTH) as lut:
                colour, plain, restated, out = paths(ctx, pics, size, lut, (lattice, shaper))
                colour()
                ref = restated()
                torch.cuda.synchronize()
                equal = bool(torch.equal(out, ref))
                del ref
                c_us, p_us, t_us = [], [], []
                for _ in range(a.rounds):
                    c_us.append(time_batches(colour, a.iters))
                    p_us.append(time_batches(plain, a.iters))
                    t_us.append(time_batches(restated, a.torch_iters))
                c, p, t = statistics.median(c_us), statistics.median(p_us), statistics.median(t_us)
                res["%s_L%d%s" % (name, L, "_shaper" if with_shaper else "")] = {
                    "size": list(size or (H, W)), "nodes": L, "shaper": with_shaper, "table_bytes": 8 * L ** 3,
                    "colour_us_per_batch": round(c, 1), "plain_us_per_batch": round(p, 1), "torch_us_per_batch": round(t, 1),
                    "stage_adds_us": round(c - p, 1), "speedup_over_torch": round(t / c, 1),
                    "colour_rounds_us": [round(x, 1) for x in c_us], "plain_rounds_us": [round(x, 1) for x in p_us],
                    "torch_rounds_us": [round(x, 1) for x in t_us], "equal_to_torch": equal}
                del out, colour, plain, restated
                torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="batches per round (colour and plain)")
    ap.add_argument("--torch-iters", type=int, default=2, help="batches per round of the torch restatement")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--content", default="noise", choices=("noise", "smooth"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")
    ctx, pics = make_context(N, a.content)
    res = {"content": a.content,
           "source_note": "%d distinct uploaded %dx%d Main10 4:2:0 pictures per batch, 8-bit RGB output; wall time per batch of %d from "
                          "torch events, %d rounds of %d batches (torch: %d), the three paths alternated, medians"
                          % (N, W, H, N, a.rounds, a.iters, a.torch_iters),
           "cases": bench(a, ctx, pics)}
    ctx.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
