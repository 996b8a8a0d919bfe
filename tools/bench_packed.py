"""Host-inclusive throughput of the packed picture input against the staging blocks, in one process.

The step of bench.py's host_inclusive(): 16 independent 2160p Main10 pictures per hmgpu_decompress_pictures(_packed) + hmgpu_filter_pictures
call, inputs copied host -> device every step, two sets of device pictures so that the copies of a step overlap the kernels of the
previous one.  The two forms run alternately (A B A B ...); per form one JSON line: Mpx/s, bytes staged per picture, PCIe GB/s, host issue
ms per step, host pack ms per picture (packed form: hmgpu_pack_input) and the average time of the `unpack` kernel (a separate, profiled
step).  Picture 0 decoded through each form into handles of its own (the packed one into a handle that held another picture's inputs
just before) must give identical planes.

    python tools/bench_packed.py [--bi] [--steps 20] [--rounds 3]
"""
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
    ap.add_argument("--bi", action="store_true", help="B pictures (bench.py --bi)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    import libhm_amd
    from libhm_amd import abi
    from tests import synth
    w, h, bd, nb = args.width, args.height, 10, 16
    metas = [synth.make_picture(w, h, bd, seed=0x484D3136 + i, bi=args.bi, ref_handles=([0], [1])) for i in range(2)]
    seq = abi.make_seq(w, h, bd, bd, log2_ctu=6, max_pictures=4 * nb)
    ctx = libhm_amd.Context(seq, device=0)
    refs = [synth.noise_planes(w, h, bd, 100), synth.blocky_planes(w, h, bd, 200)]
    refs_of = []
    for i in range(nb):
        r0, r1 = ctx.acquire(), ctx.acquire()
        ctx.upload(r0, refs[0])
        ctx.upload(r1, refs[1])
        refs_of.append((r0, r1))
    sets = [[ctx.acquire() for _ in range(nb)] for _ in range(2)]
    slices = []
    for i in range(nb):
        sl = abi.clone_slice(metas[i % 2].slice)
        for l, r in ((0, refs_of[i][0]), (1, refs_of[i][1])):
            if sl.num_ref_idx[l] > 0:
                sl.ref_pic[l][0] = r
        slices.append(sl)
    sao = [abi.sao_array_from_raw(m.sao_raw) for m in metas]
    fjobs = [ctx.filter_jobs([(hset[i], metas[i % 2].pp, sao[i % 2]) for i in range(nb)]) for hset in sets]

    # ---- staging blocks, as bench.py fills them (compact levels, the groups a picture needs)
    stg, level_bytes = [], 0
    for i in range(nb):
        s = ctx.staging_alloc()
        level_bytes = s.fill_compact(libhm_amd.lib(), seq, metas[i % 2].meta, metas[i % 2].coeffs)
        s.set_groups(intra=bool((metas[i % 2].meta_np["pred_mode"] == 1).any()), flags=False)
        stg.append(s)
    a0 = stg[0].arrays
    base = ["slice_idx", "tile_idx", "depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf_y", "cbf_u", "cbf_v", "mv0", "ref_idx0"]
    stg_bytes = sum(a0[k].nbytes for k in base) + (a0["mv1"].nbytes + a0["ref_idx1"].nbytes if args.bi else 0) + level_bytes + \
        3 * 4 * (ctx.num_ctus + 1)
    djobs_stg = [ctx.picture_jobs([(hset[i], [slices[i]], stg[i], stg[i]) for i in range(nb)]) for hset in sets]

    # ---- packed blobs in page-locked memory
    cap = libhm_amd.packed_max_bytes(seq)
    bufs = [libhm_amd.PinnedBuffer(cap) for _ in range(nb)]
    t0 = time.perf_counter()
    blobs = [libhm_amd.pack_input(seq, metas[i % 2].meta, metas[i % 2].coeffs, out=bufs[i].array) for i in range(nb)]
    pack_ms = (time.perf_counter() - t0) / nb * 1e3
    djobs_pk = [ctx.packed_jobs([(hset[i], [slices[i]], blobs[i], None) for i in range(nb)]) for hset in sets]

    forms = {"staging": (lambda k: ctx.decompress_pictures(djobs_stg[k & 1]), stg_bytes, 0.0),
             "packed": (lambda k: ctx.decompress_pictures_packed(djobs_pk[k & 1]), float(np.mean([b.nbytes for b in blobs])), pack_ms)}
    results = {f: [] for f in forms}
    out0 = {}
    for rnd in range(args.rounds):
        for name, (dec, staged, pms) in forms.items():
            def step(k):
                dec(k)
                ctx.filter_pictures(fjobs[k & 1])
            for k in range(4):
                step(k)
            ctx.sync()
            n = max(4, args.steps)
            t0 = time.perf_counter()
            for k in range(n):
                step(k)
            t_issue = time.perf_counter() - t0
            ctx.sync()
            dt = time.perf_counter() - t0
            results[name].append((n * nb * w * h / dt / 1e6, n * nb * staged / dt / 1e9, t_issue / n * 1e3))
            out0[name] = ctx.download(sets[(n - 1) & 1][0])
    # the expansion kernel on its own: one profiled step of the packed form
    ctx.set_profiling(True)
    ctx.stats(reset=True)
    forms["packed"][0](0)
    ctx.sync()
    ms, launches = ctx.stats(reset=True)["kernels"]["unpack"]
    ctx.set_profiling(False)
    # output identity on handles that the other form cannot have prepared: picture 0 through the staging block into X, and into Y first
    # picture 1 (so that Y's device arrays hold other metadata and levels), then picture 0 through the packed form into Y
    X, Y = sets[0][0], sets[1][0]
    one_stg = lambda hdl, i: ctx.decompress_pictures([(hdl, [slices[i]], stg[i], stg[i])])
    one_flt = lambda hdl, i: ctx.filter_pictures([(hdl, metas[i % 2].pp, sao[i % 2])])
    one_stg(X, 0); one_flt(X, 0)
    one_stg(Y, 1); one_flt(Y, 1)
    ctx.decompress_pictures_packed([(Y, [slices[0]], blobs[0], None)]); one_flt(Y, 0)
    ref, got = ctx.download(X), ctx.download(Y)
    identical = all(np.array_equal(ref[c], got[c]) for c in range(3)) and \
        all(np.array_equal(out0["staging"][c], out0["packed"][c]) for c in range(3))
    for name, (_, staged, pms) in forms.items():
        r = np.array(results[name])
        print(json.dumps({"form": name, "picture": "B" if args.bi else "P", "pictures_per_step": nb, "steps": max(4, args.steps),
                          "rounds": args.rounds, "Mpixels_s": round(float(np.median(r[:, 0])), 1),
                          "Mpixels_s_all": [round(float(v), 1) for v in r[:, 0]],
                          "staged_bytes_per_picture": int(staged), "PCIe_GBps": round(float(np.median(r[:, 1])), 2),
                          "host_issue_ms_per_step": round(float(np.median(r[:, 2])), 3),
                          "host_pack_ms_per_picture": round(pms, 3),
                          "unpack_kernel_avg_ms": round(ms / launches, 4) if (name == "packed" and launches) else None,
                          "picture0_identical": identical}))
    for b in bufs:
        b.free()
    for s in stg:
        ctx.staging_free(s)
    ctx.close()
    if not identical:
        sys.exit("bench_packed: the two forms put out different pictures")


if __name__ == "__main__":
    main()
