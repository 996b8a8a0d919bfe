"""GPU parity on the CU shapes that only HM's small streams used to bring to the device: 2NxN / Nx2N / NxN prediction units (8x4 and 4x8
PUs among them: the cells kernels), 16x16 minimum CUs, intra NxN, transform trees up to three levels deep with shared 4x4 chroma blocks
under large CUs and chroma nodes set with nothing below -- at sizes and in call forms where the kernels' variants run.  The pictures are the
parameter sets of tests/cu_shapes.py, which tests/test_synth_shapes_cpu.py pins to HM's syntax and counts; every comparison is bit-exact
against the C oracle: after reconstruction, after deblocking, after SAO, and with all filter stages in one call."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import cu_shapes as cs
from tests import motion_ref as mref
from tests import synth
from tests.test_gpu_formats_fullsize import STAGES, _decompress, _oracle_chain, _same
from tests.test_synth_shapes_cpu import WP_CASES, wp_picture

pytestmark = pytest.mark.gpu


def _planes(p, seeds=(11, 12, 13)):
    """reference 0 (piecewise ramps), reference 1 (blocky), the picture's start contents: the deblocking decisions fall both ways"""
    a, g = (p.width, p.height, p.bit_depth), (p.chroma_format, p.bit_depth_chroma)
    return synth.smooth_planes(*a, seeds[0], *g), synth.blocky_planes(*a, seeds[1], *g), synth.blocky_planes(*a, seeds[2], *g)


def _cells_launches(ctx):
    return ctx.stats()["kernels"]["mc_cells"][1]


def _check_all_stages(oracle, p, what, seeds=(11, 12, 13), cells=None):
    """reconstruction, after deblocking, after SAO, then again with all filter stages in one call; cells: whether the cells kernels must
    have been launched by the reconstruction (None: from the picture, by the host's rule)"""
    import libhm_amd
    ref0, ref1, cur = _planes(p, seeds)
    want = _oracle_chain(oracle, p, cur, [ref0, ref1])
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        ctx.set_profiling(True)
        ctx.stats(reset=True)
        _decompress(ctx, hc, p)
        ctx.sync()
        launches = _cells_launches(ctx)
        ctx.set_profiling(False)
        expect = cs.wants_cells(p) if cells is None else cells
        per_call = 2 if p.chroma_format == 1 else 1                   # luma and 4:2:0 chroma; the other formats' chroma kernel does its own cells
        assert launches == (per_call if expect else 0), "%scells kernels launched %d times, PUs that cut a tile: %s" % (what, launches, expect)
        _same(ctx.download(hc), want[0], what + STAGES[0])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=3)
        _same(ctx.download(hc), want[1], what + STAGES[1])
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=4)
        _same(ctx.download(hc), want[2], what + STAGES[2])
        st = ctx.stats()
        assert st["intra_partitions"] == int(p.intra.sum()) and st["inter_partitions"] == int((p.inside & ~p.intra).sum())
        ctx.upload(hc, cur)
        _decompress(ctx, hc, p)
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want[2], what + STAGES[3])
    assert not all(np.array_equal(want[0][c], want[1][c]) for c in range(3)) and not all(np.array_equal(want[1][c], want[2][c]) for c in range(3))
    return want


# ------------------------------------------------------------------------------------------------ 1. the shape matrix, 4:2:0
@pytest.mark.parametrize("name", sorted(cs.MATRIX))
def test_shape_matrix_matches_oracle(oracle, name):
    p = cs.make("matrix", name)
    kw = cs.keywords("matrix", name)
    if kw.get("min_cu_log2") == 4 and kw.get("mode_probs") == cs.NO_AMP:
        assert not cs.wants_cells(p)                                  # 16x16 minimum CUs, no AMP: no PU cuts an 8x8 tile
    if kw.get("num_slices", 1) > 1:
        assert len(p.slices) == 5 and any(a % p.ctus_w for a, _ in p.slice_ranges) and p.slices[1].lf_across_slices == 0
    if kw["intra_frac"] == 1.0:
        assert p.intra[p.inside].all() and p.slice.slice_type == abi.I_SLICE
    _check_all_stages(oracle, p, "shape matrix %s: " % name)


# ------------------------------------------------------------------------------------------------ 2. symmetric PUs only
@pytest.mark.parametrize("name", sorted(cs.SYMMETRIC))
def test_symmetric_pus_match_oracle(oracle, name):
    """8x4 / 4x8 PUs in every 8x8 CU: every tile of the picture's whole CTUs goes through the cells kernels; 64x32 .. 16x8 PUs only: none does,
    and the PUs start and end the vertical runs of the LDS-staged picture kernels"""
    p = cs.make("symmetric", name)
    m = p.meta_np
    cu_log2 = p.log2_ctu - m["depth"]
    assert np.isin(m["part_size"][p.inside], (abi.SIZE_2NxN, abi.SIZE_Nx2N)).all()
    small = name.endswith("8x8")
    if small:
        assert (cu_log2[p.inside] == 3).mean() > 0.6
    else:
        assert (cu_log2[p.inside] >= 4).all() and {4, 5, 6} <= set(np.unique(cu_log2[p.inside]))
    _check_all_stages(oracle, p, "symmetric PUs %s: " % name, cells=small)


# ------------------------------------------------------------------------------------------------ 3. 4:2:2, 4:4:4, 4:0:0
@pytest.mark.parametrize("name", sorted(cs.FORMATS))
def test_formats_on_the_shape_matrix_match_oracle(oracle, name):
    """the cell path of k_mc_chroma_fmt, PU and TU edges on the chroma planes' own 8-sample grid, 4:4:4 intra NxN with a chroma mode per PU,
    4:2:2 intra NxN through k_intra_chroma_422"""
    p = cs.make("formats", name)
    m = p.meta_np
    nxn = p.intra & (m["part_size"] == abi.SIZE_NxN)
    assert nxn.any()
    if p.chroma_format == 3:
        z = np.arange(m["depth"].shape[1])[None, :]
        cu_first = z & ~((m["depth"].shape[1] >> (2 * m["depth"].astype(np.int64))) - 1)
        assert (nxn & (np.take_along_axis(m["intra_dir_c"], cu_first, axis=1) != m["intra_dir_c"])).any()      # chroma modes differ inside a CU
        assert m["ccp_u"].any()
    _check_all_stages(oracle, p, "%s: " % name)


# ------------------------------------------------------------------------------------------------ 4. input forms, batches, handle reuse
def test_every_input_form_gives_the_oracles_planes(oracle):
    """one picture through ordinary arrays with dense levels, compact levels, a staging block (dense, then compact) and the packed entry"""
    import libhm_amd
    p = cs.make("matrix", "B-intra-bd10-ctu64-min8")
    ref0, ref1, cur = _planes(p)
    want = _oracle_chain(oracle, p, cur, [ref0, ref1])
    sao = abi.sao_array_from_raw(p.sao_raw)
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    seq.max_pictures = 7
    with libhm_amd.Context(seq) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        hs = [ctx.acquire() for _ in range(5)]
        for hnd in hs:
            ctx.upload(hnd, cur)
        compact = ctx.pack_levels(p.meta, p.coeffs)
        blocks = synth.coded_blocks(p.meta_np, 1, 6)
        for c in range(3):
            assert int(compact.starts[c][-1]) == int((blocks[blocks[:, 0] == c][:, 3] ** 2).sum())
        stg = ctx.staging_alloc()
        stg.fill(p.meta, p.coeffs)
        stg.set_groups(intra=True, flags=False)
        blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
        ctx.decompress_pictures([(hs[0], p.slices, p.meta, p.coeffs), (hs[1], p.slices, p.meta, compact), (hs[2], p.slices, stg, stg)])
        ctx.decompress_pictures_packed([(hs[3], p.slices, blob, None)])
        ctx.sync()
        stg.fill_compact(libhm_amd.lib(), ctx.seq, p.meta, p.coeffs)
        ctx.decompress_pictures([(hs[4], p.slices, stg, stg)])
        forms = ("dense arrays", "compact levels", "staging block", "packed entry", "staging block with compact levels")
        for hnd, form in zip(hs, forms):
            _same(ctx.download(hnd), want[0], form + ", reconstruction")
        ctx.filter_pictures([(hnd, p.pp, sao) for hnd in hs])
        for hnd, form in zip(hs, forms):
            _same(ctx.download(hnd), want[2], form + ", filtered")
        ctx.staging_free(stg)


def _batch(oracle, pics, what):
    import libhm_amd
    p0 = pics[0]
    ref0, ref1, cur = _planes(p0, (41, 42, 43))
    want = [_oracle_chain(oracle, q, cur, [ref0, ref1]) for q in pics]
    seq = abi.SeqParams.from_buffer_copy(p0.seq)
    seq.max_pictures = 2 + len(pics)
    with libhm_amd.Context(seq) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        hs = [ctx.acquire() for _ in pics]
        for hnd in hs:
            ctx.upload(hnd, cur)
        ctx.decompress_pictures([(hnd, q.slices, q.meta, q.coeffs) for hnd, q in zip(hs, pics)])
        for i, hnd in enumerate(hs):
            _same(ctx.download(hnd), want[i][0], "%s, picture %d, reconstruction" % (what, i))
        ctx.filter_pictures([(hnd, q.pp, abi.sao_array_from_raw(q.sao_raw)) for hnd, q in zip(hs, pics)])
        for i, hnd in enumerate(hs):
            _same(ctx.download(hnd), want[i][2], "%s, picture %d, filtered" % (what, i))


def test_batch_of_p_pictures_with_scattered_intra_nxn(oracle):
    """five P pictures with 5 .. 25 % intra CUs, NxN among them: the call form the lean intra kernel serves"""
    shares = (0.05, 0.1, 0.15, 0.2, 0.25)
    pics = [synth.make_picture(832, 480, 10, seed=0xB5 + i, intra_frac=fr, **dict(cs.SHAPES, **cs.P_REFS)) for i, fr in enumerate(shares)]
    for q, fr in zip(pics, shares):
        share = q.intra.sum() / q.inside.sum()
        assert 0.4 * fr < share < 1.6 * fr and (q.intra & (q.meta_np["part_size"] == abi.SIZE_NxN)).sum() >= 20
    _batch(oracle, pics, "batch of five P pictures")


def _intra_picture(seed, size=(832, 480)):
    p = synth.make_picture(size[0], size[1], 10, seed=seed, intra_frac=1.0, mode_probs=cs.NO_AMP, **dict(cs.SHAPES, **cs.P_REFS))
    for sl in p.slices:
        sl.slice_type = abi.I_SLICE
        sl.num_ref_idx[0] = sl.num_ref_idx[1] = 0
    assert p.intra[p.inside].all() and (p.meta_np["part_size"] == abi.SIZE_NxN).sum() > 400 and int(p.meta_np["tr_idx"].max()) == 3
    return p


def test_batch_of_all_intra_pictures(oracle):
    """four I pictures in one call (the three-wave intra kernel)"""
    _batch(oracle, [_intra_picture(0x1A + i) for i in range(4)], "batch of four I pictures")


def test_single_intra_picture(oracle):
    """one I picture in a call of its own (the eight-wave intra kernel)"""
    _batch(oracle, [_intra_picture(0x2A)], "single I picture")


def test_handle_reused_for_a_sparse_picture_after_a_deep_tree_one(oracle):
    """a picture with deep transform trees, then in the same handle one of 2Nx2N CUs with hardly a coded block: no transform-unit count,
    residual tile or edge flag of the first may survive"""
    import libhm_amd
    deep = cs.make("matrix", "B-intra-bd10-ctu64-min8", cbf_prob=0.9, tr_split_prob=0.6)
    sparse = synth.make_picture(832, 480, 10, seed=0x5A, cbf_prob=0.03, mode_probs=(0.6, 0.4, 0, 0, 0), sao=False, **cs.CROSSED)
    assert len(synth.coded_blocks(deep.meta_np, 1, 6)) > 20 * len(synth.coded_blocks(sparse.meta_np, 1, 6)) > 0
    ref0, ref1, cur = _planes(deep)
    want_deep = _oracle_chain(oracle, deep, cur, [ref0, ref1])
    want_sparse = _oracle_chain(oracle, sparse, cur, [ref0, ref1])
    with libhm_amd.Context(deep.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        for q, want, what in ((deep, want_deep, "deep trees"), (sparse, want_sparse, "sparse picture in the reused handle"), (deep, want_deep, "deep trees again")):
            ctx.upload(hc, cur)
            ctx.decompress_pictures([(hc, q.slices, q.meta, q.coeffs)])
            _same(ctx.download(hc), want[0], what + ", reconstruction")
            ctx.filter_picture(hc, q.pp, q.sao_raw)
            _same(ctx.download(hc), want[2], what + ", filtered")


# ------------------------------------------------------------------------------------------------ 5. motion export
@pytest.mark.parametrize("name", ["P-intra-bd10-ctu16-min8", "B-intra-bd10-ctu64-min8", "B-intra-bd12-ctu32-min16"])
def test_motion_export_of_shape_pictures(name):
    import libhm_amd
    from libhm_amd import motion
    from tests.test_gpu_motion import bits
    p = cs.make("matrix", name)
    with libhm_amd.Context(p.seq) as ctx:
        for k in range(2):
            ctx.upload(ctx.acquire(), synth.noise_planes(p.width, p.height, p.bit_depth, 5 + k))
        hc = ctx.acquire()
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        got = ctx.export_motion([hc], "blocks", (0, 1))
        want = mref.blocks(p.meta_np, p.slices, p.width, p.height, p.log2_ctu, motion.lists_mask((0, 1)), (0, 0, 0, 0))
        for k in ("mv", "ref_poc", "block"):
            assert got[k].shape[1:] == want[k].shape, k
            assert np.array_equal(bits(got[k][0]), want[k]), (name, k)
    codes = set(int(v) for v in np.unique(want["block"][2]))
    assert {abi.SIZE_2Nx2N, abi.SIZE_2NxN, abi.SIZE_Nx2N, abi.SIZE_NxN} <= codes
    if cs.keywords("matrix", name).get("mode_probs") != cs.NO_AMP and p.log2_ctu == 6:
        assert codes & {abi.SIZE_2NxnU, abi.SIZE_2NxnD, abi.SIZE_nLx2N, abi.SIZE_nRx2N}
    # vectors differ between the PUs of a CU: somewhere the two 4x4 blocks of an 8x8 CU's 2NxN halves carry different list-0 vectors
    m = p.meta_np
    two = p.inside & (m["part_size"] == abi.SIZE_2NxN) & (m["ref_idx0"] >= 0)
    a, z = np.nonzero(two & (np.arange(m["depth"].shape[1])[None, :] % (m["depth"].shape[1] >> (2 * m["depth"].astype(np.int64))) == 0))
    last = z + (m["depth"].shape[1] >> (2 * m["depth"][a, z].astype(np.int64))) - 1
    assert (m["mv0"][a, z] != m["mv0"][a, last]).any()


# ------------------------------------------------------------------------------------------------ 6. weighted prediction
@pytest.mark.parametrize("bd,den,bi", WP_CASES)
def test_weighted_prediction_closed_form_on_the_device(bd, den, bi):
    """whole-sample motion, no residual: the device against TComWeightPrediction's formulas in Python integers (tests/cu_shapes.py), which
    tests/test_synth_shapes_cpu.py holds the oracle to as well"""
    import libhm_amd
    p = wp_picture(bd, den, bi)
    refs = [synth.smooth_planes(p.width, p.height, bd, 61), synth.blocky_planes(p.width, p.height, bd, 62)]
    want = cs.weighted_closed_form(p, refs)
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, refs[0])
        ctx.upload(h1, refs[1])
        ctx.upload(hc, [np.full_like(a, 1) for a in refs[0]])
        ctx.decompress_slice(hc, 0, p.slice, p.meta, p.coeffs)
        _same(ctx.download(hc), want, "weighted prediction %d bits, denominators %s, %s: " % (bd, den, "bi" if bi else "uni"))


@pytest.mark.parametrize("bd,den,bi,fmt", [c + (1,) for c in WP_CASES] + [(10, (0, 7), True, 2), (8, (7, 0), False, 2), (12, (7, 0), True, 3), (8, (5, 4), False, 3)])
def test_weighted_prediction_on_shape_pictures_matches_oracle(oracle, bd, den, bi, fmt):
    """the matrix's shapes with fractional motion, residual and intra CUs under weights, denominators and offsets over their legal range, two
    reference indices per list that name the same two pictures with different weights (the reference index in the cells kernels' tile
    motion, not the picture alone, selects the weights)"""
    kw = dict(cs.SHAPES, **(cs.CROSSED if bi else dict(num_refs=2, ref_handles=([0, 1], [1]))))
    p = synth.make_picture(416, 240, bd, seed=0x77 + bd + den[0] + fmt + int(bi), intra_frac=0.1, chroma_format=fmt, **kw)
    cs.set_weights(p, den, seed=3 * bd + den[1] + fmt)
    m = p.meta_np
    for l in range(2 if bi else 1):
        assert (p.small_pu & (m["ref_idx%d" % l] == 0)).any() and (p.small_pu & (m["ref_idx%d" % l] == 1)).any()
    want = _check_all_stages(oracle, p, "weighted prediction, format %d, %d bits, denominators %s: " % (fmt, bd, den), seeds=(21, 22, 23))
    for sl in p.slices:
        sl.weighted_pred = 0
    ref0, ref1, cur = _planes(p, (21, 22, 23))
    plain = [a.copy() for a in cur]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, plain, [ref0, ref1])
    assert all(not np.array_equal(plain[c], want[0][c]) for c in range(3))
