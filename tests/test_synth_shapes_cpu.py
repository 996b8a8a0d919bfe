"""The picture generator's CU vocabulary beyond 2Nx2N / AMP -- symmetric and NxN prediction units, 16x16 minimum CUs, intra NxN, transform
trees up to three levels deep (tests/synth.py: part_probs, min_cu_log2, intra_nxn_prob, tr_depth_max) -- pinned without a GPU:
  1. synth.check_parser_invariants(), written from the standard's syntax, holds on HM's own arrays (all stream_* dumps, and the parser's
     output for HM-encoded lite streams with 16 / 32-sample CTUs and the other chroma formats) -- so it speaks about HM --, is broken by
     arrays that are wrong in one place, and holds on generated pictures of every format x CTU size x P / B with all options on;
  2. synth.coded_blocks() and the generator's levels agree in both directions on the same pictures, and with hmgpu_pack_levels;
  3. the parameter sets of tests/test_gpu_cu_shapes.py (tests/cu_shapes.py) hold, at 416x240, at least 20 members of every shape class they
     are there for;
  4. oracle properties of such pictures, and explicit weighted prediction in the oracle against its closed form."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import cu_shapes as cs
from tests import golden_util as gu
from tests import synth
from tests.test_synth_formats_cpu import PARSED, _check_layout, _check_pack_levels

ALL_ON = dict(cs.SHAPES, intra_frac=0.2)
GENERATED = [(f, l, b) for f in (0, 1, 2, 3) for l in (4, 5, 6) for b in (False, True)]
SETS = [(g, name) for g in cs.ALL for name in cs.ALL[g]]


def _generated(fmt, log2_ctu, bi, **kw):
    refs = cs.CROSSED if bi else cs.P_REFS
    kw = dict(ALL_ON, min_cu_log2=3 + (log2_ctu + int(bi)) % 2, **refs, **kw) if "min_cu_log2" not in kw else dict(ALL_ON, **refs, **kw)
    return synth.make_picture(416, 240, 10, seed=0x51 + fmt + 4 * log2_ctu + int(bi), chroma_format=fmt, log2_ctu=log2_ctu, bit_depth_chroma=8,
                              mode_probs=(0.15, 0.25, 0.25, 0.2, 0.15), **kw)


def _invariants(p):
    synth.check_parser_invariants(p.meta_np, p.chroma_format, p.log2_ctu, [sl.slice_type for sl in p.slices])


# ------------------------------------------------------------------------------------------------ 1. the invariants
@pytest.mark.parametrize("name", gu.STREAMS + gu.STREAMS_EXT)
def test_invariants_hold_on_hm_dumps(name):
    seen = 0
    for p in gu.stream_pictures(name):
        synth.check_parser_invariants(p.meta_np, p.chroma_format, int(np.log2(p.ctu_size)), [sl.slice_type for sl in p.slices])
        seen += 1
    assert seen


@pytest.mark.parametrize("name", PARSED)
def test_invariants_hold_on_hm_streams_through_the_parser(name):
    from libhm_amd import hmdec
    z = gu.load("lite_" + name)
    seen = []
    names = (("depth", "depth"), ("part_size", "part_size"), ("pred_mode", "pred_mode"), ("qp", "qp"), ("tr_idx", "tr_idx"), ("cbf_y", "cbf0"),
             ("cbf_u", "cbf1"), ("cbf_v", "cbf2"), ("ref_idx0", "ref_idx0"), ("ref_idx1", "ref_idx1"), ("intra_dir_l", "intra_dir0"),
             ("intra_dir_c", "intra_dir1"))
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(pic):
            g = pic.geometry()
            n, parts = g["num_ctbs"], 1 << (2 * g["log2_ctb"] - 4)
            meta = {k: pic.array(a).reshape(n, parts) for k, a in names}
            meta["mv0"], meta["mv1"] = pic.array("mv0").reshape(n, parts, 2), pic.array("mv1").reshape(n, parts, 2)
            meta["slice_idx"] = pic.array("slice_idx")
            synth.check_parser_invariants(meta, g["chroma_format"], g["log2_ctb"], [pic.slice_params(i)[0].slice_type for i in range(pic.num_slices())])
            seen.append(pic.poc)
        d.decode_stream(z["bitstream"], on_output=on_output)
    assert seen


def _break(p, key, ctu_z, value):
    m = {k: np.array(v) for k, v in p.meta_np.items()}
    m[key][ctu_z] = value
    return m


def test_invariants_notice_arrays_that_are_wrong_in_one_place():
    p = _generated(1, 6, True, min_cu_log2=3)
    m = p.meta_np
    types = [sl.slice_type for sl in p.slices]
    z = np.arange(256)[None, :]
    cu_log2 = 6 - m["depth"]
    inter = p.inside & (m["pred_mode"] == abi.MODE_INTER)

    def first(mask):
        a, zz = np.nonzero(mask)
        assert a.size
        return int(a[0]), int(zz[0])
    cases = []
    a, zz = first(inter & (m["part_size"] == abi.SIZE_2NxN) & (cu_log2 == 3) & (z % 4 == 0))       # an 8x4 PU: its second partition moves alone
    cases.append(("mv0", (a, zz + 1), m["mv0"][a, zz] + 4 * (m["ref_idx0"][a, zz] >= 0) + 0, "mv"))
    cases.append(("ref_idx1", (a, zz), 0 if m["ref_idx1"][a, zz] < 0 else -1, "ref"))              # ... / its lists differ over the PU, or it is bi-predicted
    a, zz = first(inter & (m["part_size"] == abi.SIZE_2Nx2N) & (cu_log2 == 3) & (z % 4 == 0))
    cases.append(("part_size", (a, slice(zz, zz + 4)), abi.SIZE_NxN, "NxN"))                        # inter NxN in an 8x8 CU
    a, zz = first(p.intra & (m["part_size"] == abi.SIZE_NxN) & (z % 4 == 0))
    cases.append(("tr_idx", (a, slice(zz, zz + 4)), 0, "intra NxN"))
    a, zz = first(p.inside & (m["tr_idx"] == 2) & (cu_log2 == 5) & (z % 16 == 0))
    cases.append(("tr_idx", (a, zz), 1, "leaf"))                                                    # one partition of an 8x8 leaf at another depth
    cases.append(("cbf_y", (a, zz), m["cbf_y"][a, zz] ^ 1, "cbf"))                                  # the root bit of one partition flipped
    cases.append(("cbf_u", (a, zz), (m["cbf_u"][a, zz] | 4) & ~2, "cbf"))                           # a chroma bit set under a clear one
    a, zz = first(p.intra)
    cases.append(("intra_dir_c", (a, zz), 5, "chroma mode"))
    cases.append(("depth", (a, zz), m["depth"][a, zz] ^ 1, "depth"))
    if m["mv0"][cases[0][1]].tolist() == list(np.atleast_1d(cases[0][2])):                          # (that PU does not use list 0: move list 1 instead)
        cases[0] = ("mv1", cases[0][1], m["mv1"][cases[0][1]] + 4, "mv")
    synth.check_parser_invariants(m, 1, 6, types)
    for key, where, value, what in cases:
        with pytest.raises(AssertionError):
            synth.check_parser_invariants(_break(p, key, where, value), 1, 6, types)


@pytest.mark.parametrize("fmt,log2_ctu,bi", GENERATED)
def test_invariants_hold_on_generated_pictures(fmt, log2_ctu, bi):
    p = _generated(fmt, log2_ctu, bi)
    _invariants(p)
    m = p.meta_np
    assert set(np.unique(m["part_size"][p.inside])) >= {abi.SIZE_2Nx2N, abi.SIZE_2NxN, abi.SIZE_Nx2N, abi.SIZE_NxN}
    assert int(m["tr_idx"].max()) == (3 if log2_ctu >= 5 else 2)
    if bi:                                                                # no 8x4 / 4x8 PU with two lists, though most larger PUs have two
        assert not (p.small_pu & (m["ref_idx0"] >= 0) & (m["ref_idx1"] >= 0)).any()
        assert ((m["ref_idx0"] >= 0) & (m["ref_idx1"] >= 0)).mean() > 0.3


@pytest.mark.parametrize("group,name", SETS)
def test_invariants_hold_on_the_gpu_tests_parameter_sets(group, name):
    _invariants(cs.make(group, name, size=cs.count_size(group, name)))


def test_the_defaults_draw_none_of_the_new_shapes():
    p = synth.make_picture(416, 240, 10, seed=1, bi=True, intra_frac=0.3, ref_handles=([0], [1]))
    ps = p.meta_np["part_size"][p.inside]
    assert not np.isin(ps, (abi.SIZE_2NxN, abi.SIZE_Nx2N, abi.SIZE_NxN)).any() and int(p.meta_np["tr_idx"].max()) == 1 and not p.small_pu.any()


# ------------------------------------------------------------------------------------------------ 2. coded blocks and levels, both directions
@pytest.mark.parametrize("fmt,log2_ctu,bi", GENERATED)
def test_generated_levels_and_coded_blocks_agree_both_ways(fmt, log2_ctu, bi):
    what = "format %d, %d-sample CTUs" % (fmt, 1 << log2_ctu)
    p = _generated(fmt, log2_ctu, bi, coef_dist="dense", cbf_prob=1.0)
    blocks, nz = _check_layout(p.meta_np, p.coeffs.arrays, fmt, log2_ctu, what)       # no level outside a block, no block without a level
    assert (nz > 0) == (fmt != 0)
    # with every flag drawn set, every transform leaf of every decoded CU is a listed luma block: the blocks tile the decoded area
    assert int((blocks[blocks[:, 0] == 0][:, 3] ** 2).sum()) == 16 * int(p.inside.sum())
    q = _generated(fmt, log2_ctu, bi, coef_dist="stress")
    blocks, _ = _check_layout(q.meta_np, q.coeffs.arrays, fmt, log2_ctu, what)
    sizes = set(int(v) for v in np.unique(blocks[blocks[:, 0] == 0, 3]))
    assert sizes == {4, 8, 16, 32} & set(range(4, (1 << log2_ctu) + 1))
    if fmt in (0, 1):
        _check_pack_levels(p.seq, p.meta, p.coeffs, synth.coded_blocks(p.meta_np, fmt, log2_ctu), what)
        _check_pack_levels(q.seq, q.meta, q.coeffs, blocks, what)


# ------------------------------------------------------------------------------------------------ 3. the shapes are there
@pytest.mark.parametrize("group,name", SETS)
def test_parameter_sets_hold_the_shapes_they_are_there_for(group, name):
    size = cs.count_size(group, name)
    p = cs.make(group, name, size=size)
    got, can = cs.counts(p), cs.possible(cs.keywords(group, name), *size)
    assert set(got) == set(can)
    for k in sorted(got):                                             # (both ways: cs.possible() is itself under test here)
        assert (got[k] >= 20) == can[k], "%s / %s at %dx%d: %d %s, expected %s" % ((group, name) + size + (got[k], k, "20 and more" if can[k] else "fewer"))
    if group == "symmetric":
        assert cs.wants_cells(p) == name.endswith("8x8")
        ps = p.meta_np["part_size"][p.inside]
        assert np.isin(ps, (abi.SIZE_2NxN, abi.SIZE_Nx2N)).all()
    if cs.keywords(group, name).get("min_cu_log2") == 4:
        assert int((p.log2_ctu - p.meta_np["depth"])[p.inside].min()) == 4


def test_every_class_and_every_axis_value_is_in_the_matrix():
    seen = {}
    for name, (w, h, kw) in cs.MATRIX.items():
        can = cs.possible(cs.keywords("matrix", name), 416, 240)
        for k, v in can.items():
            seen[k] = seen.get(k, False) or v
        for axis in ("bit_depth", "log2_ctu", "min_cu_log2"):
            for cond in ("any", "B", "intra"):
                if cond == "any" or (cond == "B" and kw.get("bi")) or (cond == "intra" and 0 < kw["intra_frac"] < 1):
                    seen.setdefault((axis, cond), set()).add(kw[axis])
    assert all(v for k, v in seen.items() if isinstance(k, str)), seen
    for cond in ("any", "B", "intra"):
        assert seen[("bit_depth", cond)] == {8, 10, 12} and seen[("log2_ctu", cond)] == {4, 5, 6} and seen[("min_cu_log2", cond)] == {3, 4}
    cells = {name: cs.wants_cells(cs.make("matrix", name, size=(416, 240))) for name in cs.MATRIX}
    assert any(cells.values()) and not all(cells.values())
    assert {(w, h) for w, h, _ in cs.MATRIX.values()} == {(416, 240), (832, 480), (1920, 1080)}


# ------------------------------------------------------------------------------------------------ 4. oracle properties
def _planes_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt,log2_ctu", [(1, 6), (1, 4), (2, 5), (3, 6)])
def test_zero_motion_and_no_levels_reproduce_the_reference(oracle, fmt, log2_ctu):
    w, h, bd, bdc = 416, 240, 10, 8
    p = _generated(fmt, log2_ctu, True, cbf_prob=0.0, mv_range=0, mv_coherence=0.0, sao=False)
    m = dict(p.meta_np)
    m["mv0"], m["mv1"] = np.zeros_like(m["mv0"]), np.zeros_like(m["mv1"])
    meta = abi.MetaHolder(m)
    ref = synth.smooth_planes(w, h, bd, 31, fmt, bdc)
    start = synth.blocky_planes(w, h, bd, 32, fmt, bdc)
    rec = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, meta, p.coeffs, rec, [ref, ref])
    assert p.intra.any()
    for c in range(3):
        keep = ~synth_mask(p, c)
        assert np.array_equal(rec[c][keep], ref[c][keep]), "component %d" % c
    for sl in p.slices:
        sl.deblocking_disable = 1
    fin = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, meta, p.pp, fin, 3)
    assert _planes_equal(fin, rec)


def synth_mask(p, comp):
    """samples of intra CUs in the component's plane"""
    sx, sy = (p.csx, p.csy) if comp else (0, 0)
    mask = np.zeros((p.height >> sy, p.width >> sx), dtype=bool)
    a, z = np.nonzero(p.intra)
    for x, y in zip(p.px[a, z] >> sx, p.py[a, z] >> sy):
        mask[y:y + (4 >> sy), x:x + (4 >> sx)] = True
    return mask


@pytest.mark.parametrize("fmt,log2_ctu,bi", [(1, 6, False), (1, 5, True), (2, 6, True), (3, 4, False)])
def test_cus_whose_pus_share_their_motion_decode_as_2Nx2N(oracle, fmt, log2_ctu, bi):
    """part_size rewritten to 2Nx2N wherever all PUs of an inter CU happen to carry the same motion -- made to happen in half of the CUs by
    copying the first PU's motion over the CU -- changes nothing before deblocking"""
    w, h, bd, bdc = 416, 240, 10, 8
    p = _generated(fmt, log2_ctu, bi, intra_frac=0.1)
    m = {k: np.array(v) for k, v in p.meta_np.items()}
    parts = m["depth"].shape[1]
    z = np.arange(parts)[None, :]
    cu_parts = parts >> (2 * m["depth"].astype(np.int64))
    cu_first = z & ~(cu_parts - 1)
    inter = p.inside & (m["pred_mode"] == abi.MODE_INTER)
    chosen = inter & (m["part_size"] != abi.SIZE_2Nx2N) & np.take_along_axis(np.random.RandomState(3).rand(*inter.shape) < 0.5, cu_first, axis=1)
    # (an 8x4 / 4x8 PU has one list: so has the CU made of two equal ones -- legal as 2Nx2N too)
    for k in ("ref_idx0", "ref_idx1"):
        m[k] = np.where(chosen, np.take_along_axis(m[k], cu_first, axis=1), m[k])
    for k in ("mv0", "mv1"):
        m[k] = np.where(chosen[:, :, None], np.take_along_axis(m[k], cu_first[:, :, None], axis=1), m[k])
    synth.check_parser_invariants(m, fmt, log2_ctu, [sl.slice_type for sl in p.slices])
    ref0, ref1 = synth.smooth_planes(w, h, bd, 31, fmt, bdc), synth.blocky_planes(w, h, bd, 33, fmt, bdc)
    start = synth.blocky_planes(w, h, bd, 32, fmt, bdc)
    as_drawn = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, abi.MetaHolder(m), p.coeffs, as_drawn, [ref0, ref1])
    m2 = dict(m)
    m2["part_size"] = np.where(chosen, abi.SIZE_2Nx2N, m["part_size"])
    assert int(chosen.sum()) > 500 and (m2["part_size"] != m["part_size"]).any()
    merged = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, abi.MetaHolder(m2), p.coeffs, merged, [ref0, ref1])
    assert _planes_equal(as_drawn, merged)
    untouched = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, untouched, [ref0, ref1])
    assert not np.array_equal(untouched[0], as_drawn[0])                                 # the copied motion did change the picture


# ------------------------------------------------------------------------------------------------ weighted prediction: the oracle against its closed form
WP_CASES = [(bd, den, bi) for bd in (8, 10, 12) for den in ((0, 7), (7, 0), (5, 4)) for bi in (False, True)]


def wp_picture(bd, den, bi, fmt=1, size=(416, 240), bdc=None):
    """the matrix's shapes without residual or intra CUs, whole-sample motion, two reference indices per list naming two pictures (in B
    pictures the same two in swapped order), weights and offsets over their whole legal range"""
    kw = dict(cs.SHAPES, **(cs.CROSSED if bi else dict(num_refs=2, ref_handles=([0, 1], [1]))))
    kw.update(cbf_prob=0.0, intra_frac=0.0, sao=False)
    p = synth.make_picture(size[0], size[1], bd, seed=0x3B + bd + den[0] + int(bi), chroma_format=fmt, bit_depth_chroma=bdc, **kw)
    cs.whole_sample_motion(p)
    cs.set_weights(p, den, seed=bd + 16 * den[0] + int(bi))
    return p


@pytest.mark.parametrize("bd,den,bi", WP_CASES)
def test_oracle_weighted_prediction_equals_the_closed_form(oracle, bd, den, bi):
    w, h = 416, 240
    p = wp_picture(bd, den, bi)
    m = p.meta_np
    for l in range(2 if bi else 1):
        assert (m["ref_idx%d" % l] == 0).any() and (m["ref_idx%d" % l] == 1).any()
    refs = [synth.smooth_planes(w, h, bd, 61), synth.blocky_planes(w, h, bd, 62)]
    rec = [np.full_like(a, 1) for a in refs[0]]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    want = cs.weighted_closed_form(p, refs)
    for c in range(3):
        assert np.array_equal(rec[c], want[c]), "component %d: %d samples differ" % (c, int((rec[c] != want[c]).sum()))
    # both clips are hit, and the component with the larger denominator (gains of 0 .. 2 there; up to 128 with denominator 0) is unclipped on a good part of the picture
    top = (1 << bd) - 1
    assert any((v == 0).any() for v in want) and any((v == top).any() for v in want)
    assert max(((v > 0) & (v < top)).mean() for v in want) > 0.1
