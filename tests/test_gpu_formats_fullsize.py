"""GPU parity at full size for the shapes beyond 4:2:0 with 64-sample CTUs: 4:2:2, 4:4:4 (with cross-component prediction), 4:0:0,
16- and 32-sample CTUs, luma and chroma of different bit depths -- synthetic HM-shaped pictures (tests/synth.py, whose layout for these
shapes tests/test_synth_formats_cpu.py pins to HM) against the C oracle, bit-exact at every stage.  The HM-made streams of these shapes are
208x120: eight CTUs of 64.  Here grids, batches (blockIdx.z), TU-list capacities, pitches past the first rows, partial CTUs on both
borders and slice borders inside a workgroup are in play; every case asserts that its picture holds what its name says."""
import ctypes

import numpy as np
import pytest

from libhm_amd import abi
from tests import synth

pytestmark = pytest.mark.gpu

STAGES = ("reconstruction", "deblocking (stages=3)", "SAO (stages=4)", "all stages in one call")


def _planes(p, seeds):
    """reference 0 (noise), reference 1 (blocky), the picture's start contents (blocky: overwritten wherever something is decoded)"""
    a = (p.width, p.height, p.bit_depth)
    g = (p.chroma_format, p.bit_depth_chroma)
    return synth.noise_planes(*a, seeds[0], *g), synth.blocky_planes(*a, seeds[1], *g), synth.blocky_planes(*a, seeds[2], *g)


def _oracle_chain(oracle, p, cur, refs):
    rec = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    fin = oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, dbk)
    return rec, dbk, fin


def _same(got, want, what):
    for c in range(3):
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            raise AssertionError("%s, component %d: %d samples differ, first at (y, x) = %s" % (what, c, len(bad), tuple(bad[0])))


def _decompress(ctx, hc, p, per_slice_calls=False):
    if per_slice_calls:
        for k, (first, num) in enumerate(p.slice_ranges):
            ctx.decompress_slice(hc, k, p.slices[k], p.meta, p.coeffs, first_ctu=first, num_ctus=num)
    elif len(p.slices) == 1:
        ctx.decompress_slice(hc, 0, p.slice, p.meta, p.coeffs)
    else:
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])


def _check_all_stages(oracle, p, seeds=(11, 12, 13), per_slice_calls=False, what=""):
    """one picture: reconstruction, after deblocking, after SAO, then the same picture again with all filter stages in one call"""
    import libhm_amd
    ref0, ref1, cur = _planes(p, seeds)
    want = _oracle_chain(oracle, p, cur, [ref0, ref1])
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        _decompress(ctx, hc, p, per_slice_calls)
        _same(ctx.download(hc), want[0], what + STAGES[0])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=3)
        _same(ctx.download(hc), want[1], what + STAGES[1])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=4)
        _same(ctx.download(hc), want[2], what + STAGES[2])
        st = ctx.stats()
        assert st["intra_partitions"] == int(p.intra.sum()) and st["inter_partitions"] == int((p.inside & ~p.intra).sum())
        ctx.upload(hc, cur)
        _decompress(ctx, hc, p, per_slice_calls)
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want[2], what + STAGES[3])
    return want


def _partial(p):
    """(CTUs cut by the right border, by the lower border, intra partitions inside partial CTUs)"""
    ctu = 1 << p.log2_ctu
    a = np.arange(p.num_ctus)
    right = ((a % p.ctus_w) + 1) * ctu > p.width
    below = ((a // p.ctus_w) + 1) * ctu > p.height
    return int(right.sum()), int(below.sum()), int(p.intra[right | below].sum())


def _blocks(p):
    return synth.coded_blocks(p.meta_np, p.chroma_format, p.log2_ctu)


def _square_kinds_422(p):
    """transform units of a 4:2:2 picture whose chroma block has only the upper / only the lower square coded (Cb and Cr together)"""
    m = p.meta_np
    parts = m["depth"].shape[1]
    z = np.arange(parts)[None, :]
    log2tu = p.log2_ctu - m["depth"] - m["tr_idx"]
    blk = np.where(log2tu == 2, 4, 1 << (2 * np.maximum(log2tu - 2, 0)))
    org = p.inside & ((z % blk) == 0)
    up_only = lo_only = 0
    for key in ("cbf_u", "cbf_v"):
        sub = (m[key] >> (m["tr_idx"] + 1)) & 1
        lo = np.take_along_axis(sub, np.minimum(z + blk // 2, parts - 1), axis=1)
        up_only += int((org & (sub == 1) & (lo == 0)).sum())
        lo_only += int((org & (sub == 0) & (lo == 1)).sum())
    return up_only, lo_only


# ------------------------------------------------------------------------------------------------ 4:2:2 and 4:4:4: the matrix
# Axes: size {1920x1080, 832x480, 416x240 (6.5 x 3.75 CTUs: partial CTUs on both borders)}, picture type {P, B}, intra fraction {0, 0.1,
# 0.6}, bit depths luma / chroma {8/8, 10/10, 12/12, 10/8, 8/10, 12/10}.  Not the cross product: six cases per format, case i taking depth
# pair i, size i mod 3, type i mod 2 (i mod 6 runs through all six size x type pairs) and intra fraction (i + i div 3) mod 3 -- every value
# of every axis occurs with both formats, every size with both types, and the heavy-intra cases fall on the two smaller sizes (4:2:2 intra
# chroma is one serial wave per picture: k_intra_chroma_422), the 1080p cases on 0 and 10 % intra.
_SIZES = [(1920, 1080), (832, 480), (416, 240)]
_DEPTHS = [(8, 8), (10, 10), (12, 12), (10, 8), (8, 10), (12, 10)]
_INTRA = [0.0, 0.1, 0.6]
MATRIX = [(fmt, i) for fmt in (2, 3) for i in range(6)]


@pytest.mark.parametrize("fmt,i", MATRIX)
def test_format_matrix_matches_oracle(oracle, fmt, i):
    (w, h), (bd, bdc), bi, intra = _SIZES[i % 3], _DEPTHS[i], bool(i % 2), _INTRA[(i + i // 3) % 3]
    p = synth.make_picture(w, h, bd, seed=0xF0 + 16 * fmt + i, bi=bi, intra_frac=intra, ref_handles=([0], [1]), chroma_format=fmt,
                           bit_depth_chroma=bdc, ccp_prob=(0.5 if fmt == 3 and i % 2 == 0 else 0.0))
    assert (p.seq.chroma_format, p.seq.bit_depth_luma, p.seq.bit_depth_chroma) == (fmt, bd, bdc)
    assert (int(p.intra.sum()) == 0) == (intra == 0.0)
    if intra == 0.1:
        assert 0.05 < p.intra.sum() / p.inside.sum() < 0.15
    if (w, h) == (416, 240):
        right, below, intra_parts = _partial(p)
        assert right == 4 and below == 7 and (intra_parts > 0) == (intra > 0)      # (i = 2: intra CUs in the partial CTUs; i = 5: none anywhere)
    if bi:
        assert ((p.meta_np["ref_idx0"] >= 0) & (p.meta_np["ref_idx1"] >= 0)).any()
    if fmt == 2:
        up, lo = _square_kinds_422(p)
        assert up > 100 and lo > 100                                  # both squares coded independently
    _check_all_stages(oracle, p, what="format %d case %d: " % (fmt, i))


@pytest.mark.parametrize("fmt,log2_ctu,w,h,bi", [(2, 4, 832, 480, True), (2, 5, 200, 136, False), (3, 5, 1920, 1080, True), (3, 4, 200, 136, False)])
def test_formats_with_small_ctus_match_oracle(oracle, fmt, log2_ctu, w, h, bi):
    """the two axes together (HM's own streams of this kind: 104 CTUs of 16 at 208x120)"""
    p = synth.make_picture(w, h, 10, seed=0x5C + fmt + log2_ctu, bi=bi, intra_frac=0.15, ref_handles=([0], [1]), chroma_format=fmt, log2_ctu=log2_ctu,
                           bit_depth_chroma=8, mode_probs=(0.2, 0.2, 0.2, 0.2, 0.2), ccp_prob=0.4 if fmt == 3 else 0.0)
    if (w, h) == (200, 136):
        right, below, intra_parts = _partial(p)
        assert right > 0 and below > 0 and intra_parts > 0
    _check_all_stages(oracle, p, what="format %d, %d-sample CTUs: " % (fmt, 1 << log2_ctu))


# ------------------------------------------------------------------------------------------------ 4:0:0
@pytest.mark.parametrize("bi,intra,bd", [(False, 0.1, 8), (True, 0.3, 10)])
def test_monochrome_matches_oracle_and_leaves_chroma_alone(oracle, bi, intra, bd):
    """4:0:0 through the 4:2:0 kernels and the fused filter: luma bit-exact, and the chroma planes -- which exist, 4:2:0-shaped, and which
    include/hmgpu.h says are left alone -- untouched by every stage, on the device as in the oracle.  Intra CUs are present on purpose:
    their Bs 2 edges are the ones a chroma deblocking that forgot about the format would filter."""
    w, h = 1920, 1080
    p = synth.make_picture(w, h, bd, seed=400 + bd, bi=bi, intra_frac=intra, ref_handles=([0], [1]), chroma_format=0)
    assert not p.meta_np["cbf_u"].any() and not p.coeffs.arrays[1].any() and p.intra.any()
    want = _check_all_stages(oracle, p, seeds=(41, 42, 43), what="4:0:0: ")
    cur = _planes(p, (41, 42, 43))[2]
    for stage in want:                                                # (the oracle's side of the claim; the device's is the comparison above)
        assert np.array_equal(stage[1], cur[1]) and np.array_equal(stage[2], cur[2])
    assert not np.array_equal(want[2][0], cur[0])


# ------------------------------------------------------------------------------------------------ 4:2:0 with 16- and 32-sample CTUs
@pytest.mark.parametrize("log2_ctu,w,h,bi,intra,slices,mode_probs", [
    (4, 1920, 1080, False, 0.1, 1, (0.1, 0.3, 0.3, 0.2, 0.1)),        # 8160 CTUs of 16 partitions (1080 = 67.5 x 16: a partial last row)
    (4, 1920, 1080, True, 0.25, 1, (0.1, 0.3, 0.3, 0.2, 0.1)),
    (4, 1920, 1080, False, 1.0, 1, (0.3, 0.3, 0.2, 0.2, 0)),          # all intra: the wavefront order over thousands of CTUs
    (4, 200, 136, True, 0.3, 1, (0, 0, 0, 1, 0)),                     # partial CTUs on both borders
    (4, 1920, 1088, False, 0.2, 5, (0.1, 0.2, 0.2, 0.2, 0.3)),        # five slices whose starts are not multiples of four CTUs (k_prep: four CTUs per wave)
    (5, 1920, 1080, True, 0.1, 1, (0.1, 0.3, 0.3, 0.2, 0.1)),
    (5, 1920, 1080, False, 1.0, 1, (0.3, 0.3, 0.2, 0.2, 0)),
    (5, 200, 136, False, 0.3, 1, (0, 0, 0, 1, 0)),
    (5, 1920, 1080, True, 0.2, 5, (0.1, 0.3, 0.3, 0.2, 0.1))])
def test_small_ctus_420_match_oracle(oracle, log2_ctu, w, h, bi, intra, slices, mode_probs):
    """4:2:0 with 16- and 32-sample CTUs at full size, through the fused loop filter: k_prep's groups of CTUs per wave, the intra wavefront
    order (d_ctu_order) and the fused filter's per-CTU SAO parameters over thousands of CTUs"""
    ctu = 1 << log2_ctu
    for attempt in range(16):          # (multi-slice cases: the first seed whose slice starts are all off the four-CTU grid)
        p = synth.make_picture(w, h, 10, seed=0x16 + log2_ctu + int(10 * intra) + slices + 100 * attempt, bi=bi, intra_frac=intra, ref_handles=([0], [1]),
                               log2_ctu=log2_ctu, num_slices=slices, lf_across_slices=0, mode_probs=mode_probs)
        if all(a % 4 for a, _ in p.slice_ranges[1:]):
            break
    assert p.num_ctus == ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu) and p.meta_np["depth"].shape[1] == ctu * ctu // 16
    if intra == 1.0:
        amp = p.meta_np["part_size"] >= abi.SIZE_2NxnU
        assert p.intra[p.inside & ~amp].all() and p.num_ctus >= 2040
        for sl in p.slices:
            sl.slice_type = abi.I_SLICE
    if (w, h) == (200, 136):
        right, below, intra_parts = _partial(p)
        assert right > 0 and below > 0 and intra_parts > 0
    if slices > 1:
        starts = [a for a, _ in p.slice_ranges]
        assert len(starts) == 5 and all(a % 4 for a in starts[1:]) and any(a % p.ctus_w for a in starts[1:])
    if mode_probs[4] and log2_ctu == 4:
        m = p.meta_np
        narrow = (m["part_size"] == abi.SIZE_nLx2N) | (m["part_size"] == abi.SIZE_nRx2N)
        assert narrow.any() and (m["depth"][narrow] == 0).all()      # 16x16 CUs with a 4-sample and a 12-sample wide PU
    _check_all_stages(oracle, p, seeds=(51, 52, 53), what="%d-sample CTUs: " % ctu)


# ------------------------------------------------------------------------------------------------ 4:2:0, 64 CTUs, two bit depths
@pytest.mark.parametrize("bd,bdc,bi,intra", [(10, 8, True, 0.1), (8, 10, False, 0.05), (12, 10, True, 0.0)])
def test_420_with_two_bit_depths_matches_oracle(oracle, bd, bdc, bi, intra):
    """the LDS-staged k_mc_chroma and the fused filter with a chroma depth of its own (HM's streams of this kind are 208x120)"""
    p = synth.make_picture(1920, 1080, bd, seed=0xBD + bd + bdc, bi=bi, intra_frac=intra, ref_handles=([0], [1]), bit_depth_chroma=bdc)
    assert (p.seq.bit_depth_luma, p.seq.bit_depth_chroma) == (bd, bdc)
    ref0, _, _ = _planes(p, (11, 12, 13))
    assert ref0[0].max() >= (1 << bd) - 8 and (1 << bdc) - 8 <= ref0[1].max() < (1 << bdc)
    _check_all_stages(oracle, p, what="%d / %d bits: " % (bd, bdc))


# ------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("fmt", [2, 3])
def test_batches_of_format_pictures_match_oracle(oracle, fmt):
    """four different pictures per call through hmgpu_decompress_pictures / hmgpu_filter_pictures (grid z = picture), one B picture among P
    pictures, one from a staging block (4:2:2) or with cross-component prediction beside pictures without (4:4:4); then one handle again
    for a much sparser picture: nothing of the first picture's residual tiles or transform-unit counts may survive"""
    import libhm_amd
    w, h, bd, bdc, n = 832, 480, 10, 8, 4
    kw = dict(ref_handles=([0], [1]), chroma_format=fmt, bit_depth_chroma=bdc)
    pics = [synth.make_picture(w, h, bd, seed=0xBA7C + 10 * fmt + i, bi=(i == 2), intra_frac=0.1 * i, cbf_prob=0.8,
                               ccp_prob=(0.6 if fmt == 3 and i == 1 else 0.0), **kw) for i in range(n)]
    sparse = synth.make_picture(w, h, bd, seed=0xBA7C + 99, cbf_prob=0.03, intra_frac=0.0, mode_probs=(0.6, 0.4, 0, 0, 0), sao=False, **kw)
    assert sum(len(_blocks(q)) for q in pics[:1]) > 20 * len(_blocks(sparse)) > 0
    assert len({q.coeffs.arrays[0].tobytes() for q in pics}) == n
    ref0, ref1, cur = _planes(pics[0], (41, 42, 43))
    want = [_oracle_chain(oracle, q, cur, [ref0, ref1]) for q in pics]
    want_sparse = _oracle_chain(oracle, sparse, cur, [ref0, ref1])
    seq = abi.make_seq(w, h, bd, bdc, log2_ctu=6, max_pictures=2 + n)
    seq.chroma_format = fmt
    with libhm_amd.Context(seq) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        hs = [ctx.acquire() for _ in range(n)]
        sao = [abi.sao_array_from_raw(q.sao_raw) for q in pics]
        stg = ctx.staging_alloc() if fmt == 2 else None
        assert stg is None or stg.levels[1].size == pics[3].coeffs.arrays[1].size      # the block's level arrays have the format's size
        for rnd in range(2):
            for hp in hs:
                ctx.upload(hp, cur)
            jobs = [(hs[i], pics[i].slices, pics[i].meta, pics[i].coeffs) for i in range(n)]
            if stg is not None:
                ctx.sync()
                stg.fill(pics[3].meta, pics[3].coeffs)
                stg.coeffs.ctu_level_start[0] = stg.coeffs.ctu_level_start[1] = stg.coeffs.ctu_level_start[2] = None      # dense levels
                jobs[3] = (hs[3], pics[3].slices, stg, stg)
            ctx.decompress_pictures(jobs)
            for i in range(n):
                _same(ctx.download(hs[i]), want[i][0], "round %d, picture %d of the batch, reconstruction" % (rnd, i))
            ctx.filter_pictures([(hs[i], pics[i].pp, sao[i]) for i in range(n)])
            for i in range(n):
                _same(ctx.download(hs[i]), want[i][2], "round %d, picture %d of the batch, filtered" % (rnd, i))
        # the handle of the densest picture again, for the sparse one, in a batch with a dense neighbour
        ctx.upload(hs[0], cur)
        ctx.upload(hs[1], cur)
        ctx.decompress_pictures([(hs[0], sparse.slices, sparse.meta, sparse.coeffs), (hs[1], pics[1].slices, pics[1].meta, pics[1].coeffs)])
        _same(ctx.download(hs[0]), want_sparse[0], "sparse picture on a reused handle, reconstruction")
        _same(ctx.download(hs[1]), want[1][0], "its neighbour in the batch, reconstruction")
        ctx.filter_pictures([(hs[0], sparse.pp, None), (hs[1], pics[1].pp, sao[1])])
        _same(ctx.download(hs[0]), want_sparse[2], "sparse picture on a reused handle, filtered")
        _same(ctx.download(hs[1]), want[1][2], "its neighbour in the batch, filtered")
        if stg is not None:
            ctx.staging_free(stg)


# ------------------------------------------------------------------------------------------------ slices
@pytest.mark.parametrize("across", [0, 1])
@pytest.mark.parametrize("fmt", [2, 3])
def test_format_pictures_in_five_slices_match_oracle(oracle, fmt, across):
    """five slices starting mid-row, each with its own tc / beta offsets and chroma QP offsets, QPs up to 51: k_deblock_chroma_fmt's slice
    lookup and the formats' chroma QP mapping min(qPi, 51) (4:2:0 goes through a table instead)"""
    for attempt in range(16):          # (the first seed whose slices differ enough from slice 0 in their tc offsets)
        p = synth.make_picture(832, 480, 10, seed=0x51 + fmt + across + 100 * attempt, intra_frac=0.3, ref_handles=([0], [1]), num_slices=5,
                               lf_across_slices=across, slice_qp_range=(38, 51), chroma_format=fmt, bit_depth_chroma=8)
        if sum(sl.tc_offset_div2 != p.slices[0].tc_offset_div2 for sl in p.slices[1:]) >= 2:
            break
    assert len(p.slices) == 5 and any(a % p.ctus_w for a, _ in p.slice_ranges)
    assert len({sl.tc_offset_div2 for sl in p.slices}) > 1 and len({sl.beta_offset_div2 for sl in p.slices}) > 1
    assert len({(sl.cb_qp_offset, sl.cr_qp_offset) for sl in p.slices}) > 2 
    assert sum(sl.tc_offset_div2 != p.slices[0].tc_offset_div2 for sl in p.slices[1:]) >= 2        # slice 0's offset is not everybody's
    over = 0                                                          # CTUs whose chroma qPi exceeds 51: the clamp is in play
    for k, (first, num) in enumerate(p.slice_ranges):
        off = max(p.slices[k].cb_qp_offset, p.slices[k].cr_qp_offset)
        over += int((p.meta_np["qp"][first:first + num, 0] + off > 51).sum())
    assert over > 0
    _check_all_stages(oracle, p, seeds=(5, 6, 7), per_slice_calls=(across == 1), what="format %d, five slices, across %d: " % (fmt, across))


# ------------------------------------------------------------------------------------------------ cross-component prediction
@pytest.mark.parametrize("dist", ["typical", "stress"])
@pytest.mark.parametrize("bd,bdc", [(10, 8), (10, 10), (8, 10)])
def test_cross_component_prediction_matches_oracle(oracle, bd, bdc, dist):
    """weights on most transform units, luma minus chroma bit depth +2, 0 and -2 (k_ccp shifts the luma residual right or left); with
    "stress" levels the luma residual saturates and the sum wraps at 16 bits as HM's Pel buffer does"""
    w, h = (1920, 1080) if (bd, bdc, dist) == (10, 8, "typical") else (832, 480)
    p = synth.make_picture(w, h, bd, seed=0xCC + bd + bdc, bi=(dist == "stress"), intra_frac=0.2, cbf_prob=0.8, coef_dist=dist, sao=(dist == "typical"),
                           ref_handles=([0], [1]), chroma_format=3, bit_depth_chroma=bdc, ccp_prob=0.85)
    m = p.meta_np
    chain = (1 << (m["tr_idx"] + 1)) - 1
    inter_coded = p.inside & ~p.intra & ((m["cbf_y"] & chain) == chain)
    for key in ("ccp_u", "ccp_v"):
        nz = int((m[key] != 0).sum())
        assert nz > 0.8 * inter_coded.sum() and (m[key] < 0).any() and (m[key] > 0).any() and (m[key][p.intra] != 0).any()
    # weights on units whose chroma block is not coded (the prediction is the whole chroma residual there) and on coded ones
    cb_coded = (m["cbf_u"] & chain) == chain
    assert ((m["ccp_u"] != 0) & ~cb_coded).any() and ((m["ccp_u"] != 0) & cb_coded).any()
    want = _check_all_stages(oracle, p, what="CCP %d / %d bits, %s levels: " % (bd, bdc, dist))
    zero = dict(m)
    zero["ccp_u"], zero["ccp_v"] = np.zeros_like(m["ccp_u"]), np.zeros_like(m["ccp_v"])
    ref0, ref1, cur = _planes(p, (11, 12, 13))
    plain = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, abi.MetaHolder(zero), p.coeffs, plain, [ref0, ref1])
    assert not np.array_equal(plain[1], want[0][1]) and not np.array_equal(plain[2], want[0][2])      # the weights do something


# ------------------------------------------------------------------------------------------------ residual extremes
@pytest.mark.parametrize("dist", ["stress", "dense"])
@pytest.mark.parametrize("fmt", [2, 3])
def test_full_range_levels_in_444_and_422(oracle, fmt, dist):
    """every block coded, levels over the full int16 range / every position in -3..3, through k_itx with the formats' chroma shapes:
    32x32 chroma blocks (4:4:4 only) and the two squares of 4:2:2, 16x16 down to 4x4"""
    p = synth.make_picture(1920, 1080, 10, seed=0xE0 + fmt, bi=(fmt == 3), intra_frac=(0.2 if fmt == 3 else 0.05), cbf_prob=1.0, coef_dist=dist, sao=False,
                           mode_probs=(0.35, 0.25, 0.2, 0.2, 0), tr_split_prob=0.4, ref_handles=([0], [1]), chroma_format=fmt, bit_depth_chroma=10)
    b = _blocks(p)
    chroma = b[b[:, 0] > 0]
    sizes = {int(s): int((chroma[:, 3] == s).sum()) for s in np.unique(chroma[:, 3])}
    if fmt == 3:
        assert sizes.get(32, 0) > 0 and set(sizes) == {4, 8, 16, 32}, sizes            # 32x32 chroma blocks exist
    else:
        up, lo = _square_kinds_422(p)
        assert set(sizes) == {4, 8, 16} and sizes[16] > 0 and up > 100 and lo > 100, sizes
    _check_all_stages(oracle, p, what="format %d, %s levels: " % (fmt, dist))


# ------------------------------------------------------------------------------------------------ range-extension tools
@pytest.mark.parametrize("flags", [15, 1, 2, 4, 8])
@pytest.mark.parametrize("fmt", [2, 3])
def test_range_extension_residual_tools_in_444_and_422(oracle, fmt, flags):
    """test_range_extension_residual_tools (tests/test_gpu_fullsize.py) in 4:4:4 and 4:2:2: transform skip and lossless blocks with rotation,
    implicit and explicit RDPCM on chroma blocks up to 32x32 (4:4:4) / 16x16 (4:2:2: a flag per square), intra smoothing switched off;
    all tools, then each alone"""
    import libhm_amd
    width, height, bd = 832, 480, 8
    p = synth.make_picture(width, height, bd, seed=0x52457874 + flags + fmt, mode_probs=(0.15, 0.25, 0.3, 0.3, 0), cbf_prob=0.9, sao=False,
                           tr_split_prob=0.4, intra_frac=0.4, ref_handles=([0], [1]), chroma_format=fmt)
    p.seq.range_ext_flags = flags
    m = dict(p.meta_np)
    rng = np.random.RandomState(flags)
    n, parts = p.num_ctus, 256
    z = np.arange(parts)[None, :]
    cu_first = z & ~((256 >> (2 * m["depth"])) - 1)
    per_cu = lambda r: np.take_along_axis(r, cu_first, axis=1)
    log2tu = 6 - m["depth"] - m["tr_idx"]
    tu_parts = np.maximum(256 >> (2 * (m["depth"] + m["tr_idx"])), 1)
    tu_first = z & ~(tu_parts - 1)
    # the partition a chroma block's flags are read at: 4:4:4 the transform unit's first; 4:2:2 the first of the upper / lower half of the
    # block's partitions (the block of four 4x4 luma TUs is that of the 8x8 node)
    if fmt == 3:
        c_first = tu_first
    else:
        half = np.where(log2tu <= 2, 4, tu_parts) // 2
        c_first = z & ~(half - 1)
    m["bypass"] = (per_cu(rng.rand(n, parts)) < 0.3).astype(np.uint8)
    firsts = [tu_first, c_first, c_first]
    sizes = []
    for c, k in enumerate(("ts_y", "ts_u", "ts_v")):
        per_blk = lambda r: np.take_along_axis(r, firsts[c], axis=1)
        ts = ((per_blk(rng.rand(n, parts)) < 0.55) & (m["bypass"] == 0)).astype(np.uint8)
        rd = per_blk(rng.randint(0, 3, size=ts.shape)).astype(np.uint8)
        inter_untransformed = (m["pred_mode"] == 0) & ((ts != 0) | (m["bypass"] != 0))
        m[k] = ts | (np.where(inter_untransformed, rd, 0) << 1).astype(np.uint8)
        coded = p.inside & ((m[("cbf_y", "cbf_u", "cbf_v")[c]] >> m["tr_idx"]) & 1).astype(bool) & (ts != 0)
        sizes.append(set(int(v) for v in np.unique(log2tu[coded])))
    assert sizes[0] == {2, 3, 4, 5} and sizes[1] == {2, 3, 4, 5} and sizes[2] == {2, 3, 4, 5}      # luma TU sizes whose (chroma) block skips the transform
    pick = per_cu(rng.rand(n, parts))
    m["intra_dir_l"] = np.where(pick < 0.3, 10, np.where(pick < 0.6, 26, m["intra_dir_l"])).astype(np.uint8)
    pick = per_cu(rng.rand(n, parts))
    m["intra_dir_c"] = np.where(pick < 0.25, 10, np.where(pick < 0.5, 26, m["intra_dir_c"])).astype(np.uint8)
    p.meta = abi.MetaHolder(m)
    ref0, ref1, cur = _planes(p, (11, 12, 13))
    want = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, want, [ref0, ref1])
    plain = [a.copy() for a in cur]
    p.seq.range_ext_flags = 0
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, plain, [ref0, ref1])
    p.seq.range_ext_flags = flags
    # the tools do something on this picture, on its chroma too (intra smoothing, flag 8, exists for chroma in 4:4:4 only)
    assert any(not np.array_equal(a, b) for a, b in zip(want[1:], plain[1:])) != (fmt == 2 and flags == 8)
    assert any(not np.array_equal(a, b) for a, b in zip(want, plain))
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        ctx.decompress_slice(hc, 0, p.slice, p.meta, p.coeffs)
        _same(ctx.download(hc), want, "format %d, range-extension flags %d: reconstruction" % (fmt, flags))
        ctx.upload(hc, cur)
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        _same(ctx.download(hc), want, "format %d, range-extension flags %d: reconstruction through the batch entry" % (fmt, flags))


# ------------------------------------------------------------------------------------------------ weighted prediction
@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("fmt", [2, 3])
def test_weighted_prediction_in_444_and_422(oracle, fmt, bi):
    """explicit weighted prediction, uni and bi, per reference index and component: launch_mc_chroma_fmt with any_wp"""
    width, height, bd, bdc = 1280, 704, 10, 8
    p = synth.make_picture(width, height, bd, seed=77 + int(bi) + fmt, bi=bi, intra_frac=0.1, num_refs=2, ref_handles=([0, 1], [1]), chroma_format=fmt,
                           bit_depth_chroma=bdc)
    sl = p.slice
    sl.weighted_pred = 1
    sl.wp_log2_denom[0], sl.wp_log2_denom[1] = 5, 4
    rng = np.random.RandomState(5)
    for l in range(2):
        for r in range(2):
            for c in range(3):
                sl.wp_weight[l][r][c] = int((1 << sl.wp_log2_denom[1 if c else 0]) + rng.randint(-12, 13))
                sl.wp_offset[l][r][c] = int(rng.randint(-20, 21))
    assert (p.meta_np["ref_idx0"] == 1).any() and (p.meta_np["ref_idx0"] == 0).any()
    want = _check_all_stages(oracle, p, seeds=(21, 22, 23), what="format %d weighted %s-prediction: " % (fmt, "bi" if bi else "uni"))
    sl.weighted_pred = 0
    ref0, ref1, cur = _planes(p, (21, 22, 23))
    plain = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, plain, [ref0, ref1])
    assert all(not np.array_equal(plain[c], want[0][c]) for c in range(3))             # the weights do something in every component


# ------------------------------------------------------------------------------------------------ scaling lists, 4:4:4
def _lists(rng, chroma32_from_16=False):
    lists = abi.ScalingLists()
    for sz in range(4):
        for l in range(6):
            lists.dc[sz][l] = int(rng.randint(1, 256)) if sz >= 2 else 16
            n = 16 if sz == 0 else 64
            kind = (sz + l) % 3                   # a ramp as encoders send it, a flat one and a wild one, list by list
            for i in range(64):
                v = 16
                if i < n:
                    v = int(rng.randint(1, 256)) if kind == 0 else (min(255, 8 + 3 * i + l + 5 * sz) if kind == 1 else 16 + 8 * l + sz)
                lists.coef[sz][l][i] = v
    if chroma32_from_16:
        for l in (1, 2, 4, 5):
            lists.dc[3][l] = lists.dc[2][l]
            for i in range(64):
                lists.coef[3][l][i] = lists.coef[2][l][i]
    return lists


@pytest.mark.parametrize("bd,slices", [(10, 1), (8, 4)])
def test_custom_scaling_lists_on_every_list_id_in_444(oracle, bd, slices):
    """test_custom_scaling_lists_on_every_list_id in 4:4:4: the 32x32 Cb / Cr lists (coef[3][1, 2, 4, 5], dc[3][...]), which only this
    format uses, differ from every other list, so that a wrong list index shows"""
    import libhm_amd
    p = synth.make_picture(1920, 1080, bd, seed=0x5CA1 + bd + slices, intra_frac=0.4, cbf_prob=0.85, tr_split_prob=0.5, sao=False,
                           mode_probs=(0.3, 0.25, 0.2, 0.15, 0.1), ref_handles=([0], [1]), num_slices=slices, chroma_format=3)
    b = _blocks(p)
    assert int(((b[:, 0] > 0) & (b[:, 3] == 32)).sum()) > 100
    lists = _lists(np.random.RandomState(0x11575 + bd))
    seen = set()
    for sz in range(4):
        for l in range(6):
            seen.add((tuple(lists.coef[sz][l][:]), lists.dc[sz][l]))
    assert len(seen) == 24                                            # no two lists alike
    derived = _lists(np.random.RandomState(0x11575 + bd), chroma32_from_16=True)
    ref0, ref1, cur = _planes(p, (61, 62, 63))
    outs = []
    for ls in (lists, derived):
        for sl in p.slices:
            sl.scaling_lists = ctypes.pointer(ls)
        o = [a.copy() for a in cur]
        oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, o, [ref0, ref1])
        outs.append(o)
    want, other = outs
    assert np.array_equal(want[0], other[0]) and not np.array_equal(want[1], other[1]) and not np.array_equal(want[2], other[2])
    for sl in p.slices:
        sl.scaling_lists = ctypes.pointer(lists)
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        _same(ctx.download(hc), want, "4:4:4 with custom scaling lists, %d slices: reconstruction" % slices)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("fmt", [2, 3])
def test_compact_and_packed_inputs_are_refused_for_422_and_444(fmt):
    """compact levels and the packed entry are defined for 4:0:0 / 4:2:0: HMGPU_EUNSUPPORTED, host side and device side, and the picture
    keeps its samples; staging blocks do serve these formats (level arrays of the format's size, no weights for cross-component prediction:
    test_batches_of_format_pictures_match_oracle runs a 4:2:2 picture through one)"""
    import libhm_amd
    w, h, bd = 416, 240, 8
    p = synth.make_picture(w, h, bd, seed=2, ref_handles=([0], [0]), chroma_format=fmt)
    with pytest.raises(libhm_amd.HmgpuError) as e:
        libhm_amd.pack_levels(p.seq, p.meta, p.coeffs)
    assert e.value.status == abi.HMGPU_EUNSUPPORTED
    cur = synth.noise_planes(w, h, bd, 3, fmt)
    with libhm_amd.Context(p.seq) as ctx:
        h0, hc = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, cur)
        ctx.upload(hc, cur)
        compact = abi.CoeffHolder(*p.coeffs.arrays)
        compact.starts = [np.zeros(p.num_ctus + 1, dtype=np.uint32) for _ in range(3)]
        for k in range(3):
            compact.struct.ctu_level_start[k] = compact.starts[k].ctypes.data
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.decompress_pictures([(hc, p.slices, p.meta, compact)])
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        blob = np.zeros(4096, dtype=np.uint8)
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.decompress_pictures_packed([(hc, p.slices, blob)])
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        ctx.sync()
        _same(ctx.download(hc), cur, "picture after the refused calls")
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])                     # and the context goes on working
        got = ctx.download(hc)
        assert not np.array_equal(got[0], cur[0])
