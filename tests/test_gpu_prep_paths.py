"""What k_prep's forms are selected by, against the C oracle (bit-exact): the per-call list-1 form in a batch that mixes P and B
pictures, slice borders inside a workgroup's four CTUs, partial CTUs with intra CUs, a picture handle that is used again and again
(the TU counters and the per-CTU intra counts carry nothing over) and the partition statistics."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import synth

pytestmark = pytest.mark.gpu


def _oracle_chain(oracle, p, cur, refs):
    rec = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    fin = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, fin, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    return rec, oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, fin)


def _same(got, want, what):
    for c in range(3):
        assert np.array_equal(got[c], want[c]), "%s, comp %d" % (what, c)


def test_p_picture_beside_a_b_picture_in_one_batch(oracle):
    """a call that holds a B picture runs the general list-1 form for every picture of the batch, an all-P call the form without list 1:
    the P picture comes out the same from both, and as the oracle's"""
    import libhm_amd
    w, h, bd = 832, 480, 10
    pp = synth.make_picture(w, h, bd, seed=0x9A01, bi=False, intra_frac=0.1, ref_handles=([0], [1]))
    pb = synth.make_picture(w, h, bd, seed=0x9A02, bi=True, intra_frac=0.1, ref_handles=([0], [1]))
    ref0, ref1 = synth.noise_planes(w, h, bd, 71), synth.blocky_planes(w, h, bd, 72)
    cur = synth.blocky_planes(w, h, bd, 73)
    want_p, fin_p = _oracle_chain(oracle, pp, cur, [ref0, ref1])
    want_b, fin_b = _oracle_chain(oracle, pb, cur, [ref0, ref1])
    with libhm_amd.Context(abi.make_seq(w, h, bd, bd, log2_ctu=6, max_pictures=4)) as ctx:
        h0, h1, hp, hb = [ctx.acquire() for _ in range(4)]
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        for levels in ("dense", "compact"):
            co_p = pp.coeffs if levels == "dense" else ctx.pack_levels(pp.meta, pp.coeffs)
            co_b = pb.coeffs if levels == "dense" else ctx.pack_levels(pb.meta, pb.coeffs)
            ctx.upload(hp, cur)
            ctx.upload(hb, cur)
            ctx.decompress_pictures([(hp, pp.slices, pp.meta, co_p), (hb, pb.slices, pb.meta, co_b)])
            mixed = ctx.download(hp)
            _same(mixed, want_p, "P picture of the mixed batch (%s levels)" % levels)
            _same(ctx.download(hb), want_b, "B picture of the mixed batch (%s levels)" % levels)
            ctx.filter_pictures([(hp, pp.pp, abi.sao_array_from_raw(pp.sao_raw)), (hb, pb.pp, abi.sao_array_from_raw(pb.sao_raw))])
            _same(ctx.download(hp), fin_p, "filtered P picture of the mixed batch")
            _same(ctx.download(hb), fin_b, "filtered B picture of the mixed batch")
            ctx.upload(hp, cur)
            ctx.decompress_pictures([(hp, pp.slices, pp.meta, co_p)])
            alone = ctx.download(hp)
            _same(alone, mixed, "P picture alone vs. in the mixed batch (%s levels)" % levels)
            ctx.filter_pictures([(hp, pp.pp, abi.sao_array_from_raw(pp.sao_raw))])
            _same(ctx.download(hp), fin_p, "filtered P picture of the all-P batch")


@pytest.mark.parametrize("per_slice_calls", [False, True])
def test_slice_borders_inside_a_workgroup(oracle, per_slice_calls):
    """1920 wide: 30 CTUs per row, so k_prep's workgroups of four CTUs straddle the rows.  Slices that start in the middle of a workgroup
    (CTU address not a multiple of four), at a row start that is one (90), inside a row and at a row start that is a multiple of four
    (360), deblocking not allowed across their borders: the slice of a CTU, of its left and of its upper neighbour differ between the waves
    of one workgroup"""
    import libhm_amd
    w, h, bd = 1920, 1080, 10
    starts = [0, 90, 157, 242, 301, 360]
    p = synth.make_picture(w, h, bd, seed=0x9B01, intra_frac=0.1, ref_handles=([0], [0]), num_slices=len(starts), lf_across_slices=0)
    assert p.ctus_w == 30 and p.num_ctus == 510 and len(p.slices) == len(starts)
    m = dict(p.meta_np)
    m["slice_idx"] = np.zeros(p.num_ctus, dtype=np.uint16)
    p.slice_ranges = []
    for k, a in enumerate(starts):
        b = starts[k + 1] if k + 1 < len(starts) else p.num_ctus
        m["slice_idx"][a:b] = k
        p.slice_ranges.append((a, b - a))
    p.meta_np, p.meta = m, abi.MetaHolder(m)
    assert any(a % 4 and a % 30 == 0 for a in starts) and any(a % 4 and a % 30 for a in starts) and any(a and a % 4 == 0 for a in starts)
    assert all(sl.lf_across_slices == 0 for sl in p.slices)
    ref = synth.noise_planes(w, h, bd, 81)
    cur = synth.blocky_planes(w, h, bd, 82)
    want_rec, want_fin = _oracle_chain(oracle, p, cur, [ref])
    with libhm_amd.Context(p.seq) as ctx:
        h0, hc = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref)
        ctx.upload(hc, cur)
        if per_slice_calls:
            for k, (first, num) in enumerate(p.slice_ranges):
                ctx.decompress_slice(hc, k, p.slices[k], p.meta, p.coeffs, first_ctu=first, num_ctus=num)
        else:
            ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        _same(ctx.download(hc), want_rec, "reconstruction")
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want_fin, "filtered picture")


@pytest.mark.parametrize("width,height", [(416, 240), (200, 136)])
def test_partial_ctus_with_intra_cus_and_statistics(oracle, width, height):
    """the last CTU column AND row are partly outside the picture (multiples of 8 that are not multiples of 64), with intra CUs in them:
    the areas outside write empty records, emit no TU and count in no statistic; hmgpu_get_stats gives the partitions counted from the
    metadata"""
    import libhm_amd
    bd = 8
    assert width % 64 and height % 64
    p = synth.make_picture(width, height, bd, seed=0x9C01 + width, intra_frac=0.35, cbf_prob=0.7, ref_handles=([0], [0]))
    partial = [a for a in range(p.num_ctus) if not p.inside[a].all()]
    assert partial and p.intra[partial].any() and (p.inside & ~p.intra)[partial].any()
    ref = synth.noise_planes(width, height, bd, 91)
    cur = synth.blocky_planes(width, height, bd, 92)
    want_rec, want_fin = _oracle_chain(oracle, p, cur, [ref])
    n_intra, n_inter = int(p.intra.sum()), int((p.inside & ~p.intra).sum())
    with libhm_amd.Context(p.seq) as ctx:
        h0, hc = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref)
        for rnd, co in enumerate((p.coeffs, ctx.pack_levels(p.meta, p.coeffs))):
            ctx.upload(hc, cur)
            ctx.stats(reset=True)
            if rnd == 0:
                ctx.decompress_slice(hc, 0, p.slice, p.meta, co)
            else:
                ctx.decompress_pictures([(hc, p.slices, p.meta, co)])
            _same(ctx.download(hc), want_rec, "reconstruction, round %d" % rnd)
            st = ctx.stats()
            assert (st["intra_partitions"], st["inter_partitions"]) == (n_intra, n_inter), "round %d" % rnd
            ctx.filter_picture(hc, p.pp, p.sao_raw)
            _same(ctx.download(hc), want_fin, "filtered picture, round %d" % rnd)


def test_one_handle_for_picture_after_picture(oracle):
    """one picture handle decodes three different pictures in turn -- intra CUs and many coded TUs, then none and few, then intra CUs in
    other CTUs -- and the last one is then replayed on two streams: no TU count, no per-CTU intra count and no "done" flag of an earlier
    picture (or an earlier replay iteration) may survive into the next"""
    import libhm_amd
    w, h, bd = 832, 480, 10
    pics = [synth.make_picture(w, h, bd, seed=0x9D01, intra_frac=0.3, cbf_prob=0.8, ref_handles=([0], [0])),
            synth.make_picture(w, h, bd, seed=0x9D02, intra_frac=0.0, cbf_prob=0.1, ref_handles=([0], [0])),
            synth.make_picture(w, h, bd, seed=0x9D03, intra_frac=0.15, cbf_prob=0.5, ref_handles=([0], [0]))]
    per_ctu = [q.intra.any(axis=1) for q in pics]
    assert not per_ctu[1].any() and (per_ctu[0] & ~per_ctu[2]).any() and (per_ctu[2] & ~per_ctu[0]).any()
    ref = synth.noise_planes(w, h, bd, 95)
    cur = synth.blocky_planes(w, h, bd, 96)
    want = [_oracle_chain(oracle, q, cur, [ref]) for q in pics]
    with libhm_amd.Context(abi.make_seq(w, h, bd, bd, log2_ctu=6, max_pictures=3)) as ctx:
        h0, hc, hd = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref)
        for levels in ("dense", "compact"):
            for i, q in enumerate(pics):
                co = q.coeffs if levels == "dense" else ctx.pack_levels(q.meta, q.coeffs)
                for pic in (hc, hd):
                    ctx.upload(pic, cur)
                ctx.decompress_pictures([(hc, q.slices, q.meta, co), (hd, q.slices, q.meta, co)])
                for pic in (hc, hd):
                    _same(ctx.download(pic), want[i][0], "picture %d, %s levels: reconstruction" % (i, levels))
                sao = abi.sao_array_from_raw(q.sao_raw)
                ctx.filter_pictures([(hc, q.pp, sao), (hd, q.pp, sao)])
                for pic in (hc, hd):
                    _same(ctx.download(pic), want[i][1], "picture %d, %s levels: filtered" % (i, levels))
        # the last picture again, as the benchmark runs it: both handles as one batch, then as two lanes on two streams
        ctx.replay([hc, hd], 15, 3)
        for pic in (hc, hd):
            _same(ctx.download(pic), want[2][1], "replay on one stream")
        ctx.set_streams(2)
        ctx.replay([hc, hd], 15, 4)
        for pic in (hc, hd):
            _same(ctx.download(pic), want[2][1], "replay on two streams")
        ctx.set_streams(1)
        # ... and the handle takes another picture afterwards
        ctx.upload(hc, cur)
        ctx.decompress_pictures([(hc, pics[1].slices, pics[1].meta, pics[1].coeffs)])
        _same(ctx.download(hc), want[1][0], "picture 1 after the replays")
