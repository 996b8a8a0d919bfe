"""The pattern pictures of tests/filter_patterns.py on the CPU: their reconstruction is the crafted picture, and the crafted picture holds every
case of the deblocking arithmetic in numbers -- conditions on the INPUT of the GPU tests (tests/test_gpu_filter_patterns.py), met by
construction and counted here with the module's own restatement of the decisions.  What the filters make of the pictures comes from the oracle."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import filter_patterns as fp

W, H = 520, 328
LUMA_CLASSES = ["tc = 0", "d >= beta", "strong, 2tc limit active", "strong, 2tc limit inactive", "weak, dEp and dEq", "weak, dEp only", "weak, dEq only",
                "weak, neither", "weak, lines 0 and 3 inside 10tc, line 1 or 2 outside", "delta clipped at +tc", "delta clipped at -tc", "result clipped at 0",
                "result clipped at max", "P side exempt only", "Q side exempt only", "both sides exempt", "Bs 1", "Bs 2"]
CHROMA_CLASSES = ["chroma: delta clipped", "chroma: delta not clipped", "chroma: result clipped at 0", "chroma: result clipped at max",
                  "chroma: P side exempt only", "chroma: Q side exempt only"]


def coverage(oracle, p, direction):
    """class -> number of edge units, with the oracle's own boundary strengths"""
    bv, bh = oracle.boundary_strengths(p.seq, p.slices, p.meta, p.pp)
    units = fp.units_of(p, direction, fp.bs_units(p, bv, bh, direction))
    turn = (lambda a: a) if direction == "ver" else (lambda a: a.T)
    got = fp.classify_luma(turn(p.pat[0]), p.bit_depth, units)
    cs = (p.csx, p.csy) if direction == "ver" else (p.csy, p.csx)
    if p.chroma_format:
        for comp in (1, 2):
            for k, v in fp.classify_chroma(turn(p.pat[comp]), p.bit_depth_chroma, units, comp, *cs).items():
                got[k] = got.get(k, 0) + v
    return got


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_arithmetic_pictures_hold_every_case(oracle, bd, direction):
    p = fp.arith_picture(W, H, bd, bd, 1, 6, direction)
    rec = [np.zeros_like(a) for a in p.pat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [p.pat, p.pat])
    for c in range(3):
        assert np.array_equal(rec[c], p.pat[c]), "the reconstruction is not the crafted picture, component %d" % c
    lo, hi = -6 * (bd - 8), 51
    assert set(np.unique(p.qp)) == set(range(lo, hi + 1))                       # QP per CU over the whole legal range
    assert len(p.slices) == 3 and p.slice_ranges[1][0] % p.ctus_w                # the second slice starts mid-row
    got = coverage(oracle, p, direction)
    print("coverage %d bits %s: %s" % (bd, direction, got))
    for k in LUMA_CLASSES + CHROMA_CLASSES + (["delta beyond 16 bits before the shift"] if bd == 12 else []):
        assert got[k] >= 32, (k, got[k])
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 1 if direction == "ver" else 2)
    share = fp.near_edge_changed(rec[0], dbk[0], direction)
    print("luma samples within 4 of an edge changed by deblocking: %.1f %%" % (100 * share))
    assert share >= 0.30
    assert all(not np.array_equal(rec[c], dbk[c]) for c in (1, 2))


@pytest.mark.parametrize("fmt,bd,bdc,log2_ctu", [(2, 8, 10, 6), (3, 12, 10, 4), (0, 10, 10, 5)])
def test_other_shapes_reconstruct_the_crafted_picture(oracle, fmt, bd, bdc, log2_ctu):
    """the builder's layouts beyond 4:2:0 with 64-sample CTUs (PCM samples of 4:2:2 / 4:4:4 blocks, small CTUs cut by both borders)"""
    for direction in ("ver", "hor"):
        p = fp.arith_picture(W, H, bd, bdc, fmt, log2_ctu, direction)
        rec = [np.zeros_like(a) for a in p.pat]
        oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [p.pat, p.pat])
        assert np.array_equal(rec[0], p.pat[0])
        for c in (1, 2):
            assert np.array_equal(rec[c], p.pat[c] if fmt else np.zeros_like(p.pat[c])), c      # (4:0:0: the chroma planes are left alone)
        got = coverage(oracle, p, direction)
        for k in LUMA_CLASSES + (CHROMA_CLASSES[:4] if fmt else []):
            assert got[k] >= 32, (direction, k, got[k])


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("fmt,log2_ctu", [(1, 6), (2, 4)])
def test_exempt_pictures_hold_every_side(oracle, fmt, log2_ctu, direction):
    p = fp.variant_picture(W, H, 10, 10, fmt, log2_ctu, direction, "exempt")
    rec = [np.zeros_like(a) for a in p.pat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [p.pat, p.pat])
    assert all(np.array_equal(rec[c], p.pat[c]) for c in range(3))
    got = coverage(oracle, p, direction)
    print("coverage exempt format %d %s: %s" % (fmt, direction, got))
    for k in ("P side exempt only", "Q side exempt only", "both sides exempt", "chroma: P side exempt only", "chroma: Q side exempt only"):
        assert got[k] >= 32, (k, got[k])
    # SAO groups of 8 chroma samples (two CUs wide where chroma is subsampled horizontally) with an exempt and an ordinary CU
    exempt = p.pcm | p.bypass
    assert p.csx == 1 and int((exempt[:, 0:-1:2] != exempt[:, 1::2]).sum()) >= 32
    # ... and the exempt CUs come out of deblocking + SAO as they went in, the others do not all
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 3)
    fin = oracle.sao_process(p.seq, p.slices, p.pp, p.meta, oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw), dbk)
    mask = np.kron(exempt, np.ones((8, 8), dtype=bool))
    assert np.array_equal(fin[0][mask], rec[0][mask]) and (fin[0][~mask] != rec[0][~mask]).mean() > 0.3


@pytest.mark.parametrize("variant,fmt,bd,bdc,log2_ctu", [("bo", 1, 8, 8, 6), ("bo", 1, 12, 10, 6), ("bo", 3, 12, 12, 5), ("bo", 1, 10, 10, 4), ("eo0", 1, 10, 10, 6),
                                                         ("eo1", 1, 10, 10, 6), ("eo2", 1, 10, 10, 6), ("eo3", 1, 10, 10, 6), ("eo1", 1, 12, 10, 6), ("eo3", 2, 10, 10, 6)])
def test_sao_pictures_hold_every_case(oracle, variant, fmt, bd, bdc, log2_ctu):
    p = fp.sao_picture(W, H, bd, bdc, fmt, log2_ctu, variant)
    rec = [np.zeros_like(a) for a in p.pat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [p.pat, p.pat])
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 3)
    assert all(np.array_equal(dbk[c], p.pat[c]) for c in range(3))                     # SAO reads the crafted picture
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    cov = fp.sao_coverage(p, prm)
    cw = p.ctus_w
    for comp in range(3):
        mx = (1 << (bdc if comp else bd)) - 1
        assert (cov["min"][comp], cov["max"][comp]) == (0, mx)
        if variant == "bo":
            assert cov["band starts"][comp] == set(range(32)) and cov["bands under BO"][comp] == set(range(32))
            lim = ((1 << (min(bdc if comp else bd, 10) - 5)) - 1) << int(p.pp.sao_offset_shift_chroma if comp else p.pp.sao_offset_shift_luma)
            offs = prm[:, comp, 3:][prm[:, comp, 0] != abi.SAO_OFF]
            assert offs.max() == lim and offs.min() == -lim
            if (bd, bdc) == (12, 10) and comp == 0:
                assert lim == 124
        else:
            nine = {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)}
            for typ in range(4):
                assert cov["sign pairs"][comp][typ] == nine, (comp, typ)
    # different types per component in most CTUs; the merges of sao_layout() resolved by the oracle: chains along a tile's row (the one in the
    # right tile hangs on the column chain), four rows of one column, one into OFF
    types = np.where(prm[:, :, 0] == abi.SAO_OFF, -1, prm[:, :, 1] * 100 + prm[:, :, 2])
    assert (types[:, 0] != types[:, 1]).mean() > 0.5 and (types[:, 1] != types[:, 2]).mean() > 0.5
    split = cw // 2 + 1
    assert all(p.sao_raw[2 * cw + x, 0, 0] == abi.SAO_MERGE for x in range(1, split)) and np.array_equal(prm[2 * cw + split - 1], prm[2 * cw])
    assert all(np.array_equal(prm[y * cw + split], prm[cw + split]) for y in range(2, 5)) and np.array_equal(prm[4 * cw + cw - 1], prm[cw + split])
    assert prm[3 * cw + 2, 0, 0] == abi.SAO_OFF and p.sao_raw[3 * cw + 2, 0, 0] == abi.SAO_MERGE
    sl, tl = p.meta_np["slice_idx"].astype(int), p.meta_np["tile_idx"].astype(int)
    for a in p.merges:                                                                  # every merge stays inside its slice and tile
        o = a - 1 if p.merges[a] == 0 else a - cw
        assert sl[o] == sl[a] and tl[o] == tl[a]
    # a CTU whose above-left neighbour lies in another slice while its above and left neighbours do not (slice 1 starts mid-row)
    a = np.arange(cw, p.num_ctus)
    a = a[a % cw > 0]
    assert ((sl[a - cw - 1] != sl[a]) & (sl[a - cw] == sl[a]) & (sl[a - 1] == sl[a])).any()
    assert [s.lf_across_slices for s in p.slices] == [1, 0, 1] and p.pp.lf_across_tiles == 0 and len(set(tl)) == 4
    fin = oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, dbk)
    for comp in range(3 if fmt else 1):
        ch = fin[comp] != dbk[comp]
        print("SAO %s component %d changes %.1f %% of the samples" % (variant, comp, 100 * ch.mean()))
        assert ch.mean() > 0.1
        mx = (1 << (bdc if comp else bd)) - 1
        assert ((fin[comp] == 0) & ch).any() and ((fin[comp] == mx) & ch).any()          # results clipped to both ends of the range


def _border_cus(p, direction):
    """per CU (frame of `direction`: edges vertical): its left edge is a slice border the later slice forbids filtering across / a tile border
    inside one slice / it lies in the slice whose deblocking is disabled"""
    s, t = (p.cu_slice, p.cu_tile) if direction == "ver" else (p.cu_slice.T, p.cu_tile.T)
    forbids = np.array([o["lf_across_slices"] == 0 for o in p.slice_opts])
    sb, tb = np.zeros(s.shape, dtype=bool), np.zeros(s.shape, dtype=bool)
    sb[:, 1:] = (s[:, 1:] != s[:, :-1]) & forbids[np.maximum(s[:, 1:], s[:, :-1])]
    tb[:, 1:] = (t[:, 1:] != t[:, :-1]) & (s[:, 1:] == s[:, :-1])
    return {"slice border": sb, "tile border": tb, "disabled slice": np.array([o["deblocking_disable"] == 1 for o in p.slice_opts])[s]}


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("fmt,bd,log2_ctu", [(1, 10, 6), (2, 8, 5), (3, 12, 6)])
def test_controls_pictures_forbid_edges_the_filter_would_change(oracle, fmt, bd, log2_ctu, direction):
    """the forbidden edges of the controls pictures are filter-active: the same picture with every control set to "filter" comes out of the
    oracle's deblocking different at slice borders, at tile borders and inside the disabled slice"""
    p = fp.controls_picture(W, H, bd, bd, fmt, log2_ctu, direction, 0)
    q = fp.controls_picture(W, H, bd, bd, fmt, log2_ctu, direction, 0, allow=True)
    assert all(np.array_equal(a, b) for a, b in zip(p.pat, q.pat))
    out = []
    for pic in (p, q):
        rec = [np.zeros_like(a) for a in pic.pat]
        oracle.decompress_ctus(pic.seq, pic.slices, pic.meta, pic.coeffs, rec, [pic.pat, pic.pat])
        assert all(np.array_equal(a, b) for a, b in zip(rec, pic.pat))
        oracle.loop_filter_pic(pic.seq, pic.slices, pic.meta, pic.pp, rec, 1 if direction == "ver" else 2)
        out.append(rec[0] if direction == "ver" else rec[0].T)
    diff = out[0] != out[1]
    q_side = diff.reshape(diff.shape[0] // 8, 8, diff.shape[1] // 8, 8)[:, :, :, :4].any(axis=(1, 3))        # per CU: the Q side of its left edge
    got = {k: (int((q_side & v).sum()), int(v.sum())) for k, v in _border_cus(p, direction).items()}
    print("controls format %d %s: CUs whose left edge the controls keep from being filtered (differing, all): %s" % (fmt, direction, got))
    assert got["slice border"][0] >= (4 if direction == "ver" else 32)          # (a slice border runs down one CTU per slice start, along the rows for CTU rows)
    assert got["tile border"][0] >= 32 and got["disabled slice"][0] >= 32
    # slices of all three types, two with the references the other way round, starting mid-row; six tiles
    assert len({s.slice_type for s in p.slices}) == 3 and sum(o["swap_refs"] for o in p.slice_opts) == 2
    assert all(a % p.ctus_w for a, _ in p.slice_ranges[1:]) and len(set(p.cu_tile.ravel().tolist())) == 6
