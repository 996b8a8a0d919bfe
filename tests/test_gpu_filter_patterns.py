"""The loop filters on content they act on: pattern pictures (tests/filter_patterns.py) whose reconstruction is exactly a crafted picture, so
that every edge unit, SAO band and edge class of the test is there by construction -- tests/test_filter_patterns_cpu.py counts them --
through the device and the C oracle, bit-exact at every stage.  520x328: 9 x 6 CTUs of 64 (the four CTUs of a k_prep workgroup straddle
rows, both borders cut a CTU by 8 samples, the chroma width 260 ends in half an SAO group)."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import filter_patterns as fp

pytestmark = pytest.mark.gpu

W, H = 520, 328


def _same(got, want, what):
    for c in range(3):
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            y, x = (int(v) for v in bad[0])
            raise AssertionError("%s, component %d: %d samples differ, first at (y, x) = (%d, %d): device %d, oracle %d"
                                 % (what, c, len(bad), y, x, got[c][y, x], want[c][y, x]))


def _oracle_stages(oracle, p):
    """the oracle's picture after reconstruction, after each deblocking direction alone, after both, and after SAO on top"""
    rec = [np.zeros_like(a) for a in p.pat]
    handles = {int(s.ref_pic[l][i]) for s in p.slices for l in range(2) for i in range(int(s.num_ref_idx[l]))}
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [p.pat] * (max(handles) + 1))      # (the oracle's references are indexed by handle)
    out = {"rec": rec}
    for mask in (1, 2, 3):
        out[mask] = [a.copy() for a in rec]
        oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, out[mask], mask)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    out["fin"] = oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, out[3])
    return out


def _decompress(ctx, hc, p, per_slice_calls=False):
    ctx.upload(hc, [np.zeros_like(a) for a in p.pat])
    if per_slice_calls:
        for k, (first, num) in enumerate(p.slice_ranges):
            ctx.decompress_slice(hc, k, p.slices[k], p.meta, p.coeffs, first_ctu=first, num_ctus=num)
    else:
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])


def _context(p):
    """a context with the crafted picture in both references (handles 0 and 1) and a third picture to decode into"""
    import libhm_amd
    ctx = libhm_amd.Context(p.seq)
    h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
    assert (h0, h1) == (0, 1)
    ctx.upload(h0, p.pat)
    ctx.upload(h1, p.pat)
    return ctx, hc


def _check_stages(ctx, hc, p, want, what, stage_masks=(1, 2, 3), per_slice_calls=False):
    _decompress(ctx, hc, p, per_slice_calls)
    _same(ctx.download(hc), want["rec"], what + "reconstruction")
    for mask in stage_masks:
        if mask != stage_masks[0]:
            _decompress(ctx, hc, p, per_slice_calls)
        ctx.filter_picture(hc, p.pp, p.sao_raw, stages=mask)
        _same(ctx.download(hc), want[mask], what + "deblocking, stages=%d" % mask)
    ctx.filter_picture(hc, p.pp, p.sao_raw, stages=4)                       # (the last mask was 3)
    _same(ctx.download(hc), want["fin"], what + "SAO (stages=4) after stages=3")
    _decompress(ctx, hc, p, per_slice_calls)
    ctx.filter_picture(hc, p.pp, p.sao_raw)
    _same(ctx.download(hc), want["fin"], what + "all stages in one call")


# ------------------------------------------------------------------------------------------------ deblocking arithmetic
# chroma format x bit depths luma / chroma x CTU size: not the cross product; every format takes every luma depth, 4:2:0 every pair
ARITH = [(1, 8, 8, 6), (1, 10, 10, 4), (1, 12, 12, 6), (1, 12, 12, 4), (1, 12, 10, 6), (1, 8, 10, 4),
         (2, 8, 10, 6), (2, 10, 10, 4), (2, 12, 12, 6), (3, 8, 8, 4), (3, 10, 10, 6), (3, 12, 10, 6), (3, 12, 12, 4),
         (0, 8, 8, 6), (0, 10, 10, 4), (0, 12, 12, 6)]


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("fmt,bd,bdc,log2_ctu", ARITH)
def test_deblocking_arithmetic_matches_oracle(oracle, fmt, bd, bdc, log2_ctu, direction):
    """every decision and every clip of the luma and chroma pel filters (the classes test_filter_patterns_cpu.py counts) in the stand-alone
    kernels -- stages=1 / 2 / 3: k_deblock, k_deblock_chroma_fmt -- and, with SAO on, in one call: k_filter_fused for 4:2:0.  At 12 bits the
    pictures hold the units whose weak-filter delta 9 (q0 - p0) - 3 (q1 - p1) + 8 needs 17 bits: a packed 16-bit form of that expression wraps
    on them (p0 = 0 stays 0 where HM writes tc), which is why filter_core.h computes it in 32 bits above 10 bits."""
    p = fp.arith_picture(W, H, bd, bdc, fmt, log2_ctu, direction, sao_seed=7)
    want = _oracle_stages(oracle, p)
    mine = 1 if direction == "ver" else 2
    assert not np.array_equal(want[mine][0], want["rec"][0])
    ctx, hc = _context(p)
    with ctx:
        _check_stages(ctx, hc, p, want, "format %d, %d / %d bits, CTU %d, %s: " % (fmt, bd, bdc, 1 << log2_ctu, direction), stage_masks=(mine, 3 - mine, 3))


# ------------------------------------------------------------------------------------------------ SAO arithmetic
SAO_SHAPES = [(1, 8, 8, 6), (1, 12, 10, 6), (1, 10, 10, 4), (2, 10, 10, 6), (3, 12, 12, 5)]
SAO_CASES = [("bo",) + s for s in SAO_SHAPES] + [("eo%d" % k, 1, 10, 10, 6) for k in range(4)] + \
            [("eo%d" % k,) + SAO_SHAPES[(k + 1) % 5] for k in range(4)] + [("eo2", 0, 10, 10, 6)]


@pytest.mark.parametrize("variant,fmt,bd,bdc,log2_ctu", SAO_CASES)
def test_sao_arithmetic_matches_oracle(oracle, variant, fmt, bd, bdc, log2_ctu):
    """band offset at every band start with the largest offsets (12 / 10 bits: scaled to +-124, the edge of the device's int8), edge offset of
    every class, different types per component, CTU borders that face the picture border, a slice border whose two slices disagree about
    filtering across it, and a tile border that forbids it; merge chains along a tile's row, up a tile's column and into OFF -- on a picture
    that SAO reads as crafted (deblocking disabled): k_sao after the (idle) deblocking stages, and the single call"""
    p = fp.sao_picture(W, H, bd, bdc, fmt, log2_ctu, variant)
    want = _oracle_stages(oracle, p)
    for mask in (1, 2, 3):
        assert all(np.array_equal(want[mask][c], p.pat[c]) for c in range(3 if fmt else 1))
    assert not np.array_equal(want["fin"][0], p.pat[0])
    ctx, hc = _context(p)
    with ctx:
        _check_stages(ctx, hc, p, want, "SAO %s, format %d, %d / %d bits, CTU %d: " % (variant, fmt, bd, bdc, 1 << log2_ctu), stage_masks=(3,))
        _decompress(ctx, hc, p, per_slice_calls=True)                       # the slices handed over one by one
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want["fin"], "slice by slice, all stages in one call")


@pytest.mark.parametrize("bad", ["slice", "tile_left", "tile_above"])
def test_sao_merge_across_slice_or_tile_border_is_refused(oracle, bad):
    """a merge candidate in another slice or tile does not exist (HM asserts): HMGPU_EINVAL from the host-side staging, before anything is
    enqueued -- the picture stays what it was, through hmgpu_filter_picture_stages and through hmgpu_filter_pictures"""
    import libhm_amd
    good = fp.sao_picture(W, H, 10, 10, 1, 6, "bo")
    p = fp.sao_picture(W, H, 10, 10, 1, 6, "bo", bad_merge=bad)
    assert (p.sao_raw != good.sao_raw).any()
    want = _oracle_stages(oracle, good)
    ctx, hc = _context(p)
    with ctx:
        _decompress(ctx, hc, p)
        for call in ("picture", "pictures"):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                if call == "picture":
                    ctx.filter_picture(hc, p.pp, p.sao_raw)
                else:
                    ctx.filter_pictures([(hc, p.pp, abi.sao_array_from_raw(p.sao_raw))])
            assert e.value.status == abi.HMGPU_EINVAL
            _same(ctx.download(hc), want["rec"], "after the refused call (%s)" % call)
        ctx.filter_picture(hc, good.pp, good.sao_raw)                       # and the legal parameters still work on it
        _same(ctx.download(hc), want["fin"], "legal parameters after the refusals")


# ------------------------------------------------------------------------------------------------ exemptions
@pytest.mark.parametrize("fmt,bd,bdc,log2_ctu", [(1, 10, 10, 6), (1, 8, 8, 4), (2, 10, 8, 6), (3, 12, 12, 5), (1, 12, 12, 6)])
def test_exempt_cus_match_oracle(oracle, fmt, bd, bdc, log2_ctu):
    """lossless CUs and PCM CUs under pcm_loop_filter_disable between ordinary ones: exempt P / Q sides in deblocking (luma and chroma, both
    directions), SAO groups of 8 samples that straddle exempt and ordinary CUs (sao_exempt_mask).  One handle takes a picture with exemptions
    and then one without (nothing of the first may survive: PicDev::any_nofilt); then both in one hmgpu_filter_pictures batch, whose fused
    kernel variant is chosen per batch"""
    a = fp.variant_picture(W, H, bd, bdc, fmt, log2_ctu, "ver", "exempt")
    a2 = fp.variant_picture(W, H, bd, bdc, fmt, log2_ctu, "hor", "exempt")
    b = fp.variant_picture(W, H, bd, bdc, fmt, log2_ctu, "hor", "plain", ref_handles=(2, 3))
    wa, wa2, wb = (_oracle_stages(oracle, p) for p in (a, a2, b))
    import libhm_amd
    with libhm_amd.Context(a.seq) as ctx:
        hs = [ctx.acquire() for _ in range(6)]
        assert hs[:4] == [0, 1, 2, 3]
        for h in (2, 3):
            ctx.upload(h, b.pat)
        for p, want, name in ((a, wa, "exempt CUs, ver: "), (b, wb, "no exempt CU after a picture with some: "), (a2, wa2, "exempt CUs, hor: ")):
            if p is not b:
                for h in (0, 1):
                    ctx.upload(h, p.pat)
            _check_stages(ctx, hs[4], p, want, name)
        # a batch of both kinds (a2's references are in place)
        for order in ((a2, b), (b, a2)):
            for p, h in zip(order, hs[4:]):
                ctx.upload(h, [np.zeros_like(x) for x in p.pat])
            ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs) for p, h in zip(order, hs[4:])])
            ctx.filter_pictures([(h, p.pp, abi.sao_array_from_raw(p.sao_raw)) for p, h in zip(order, hs[4:])])
            for p, h in zip(order, hs[4:]):
                _same(ctx.download(h), (wa2 if p is a2 else wb)["fin"], "batch of a picture with exempt CUs and one without, %s: " % ("with" if p is a2 else "without"))


# ------------------------------------------------------------------------------------------------ controls on filter-active content
@pytest.mark.parametrize("fmt,bd,bdc,log2_ctu,lf_across_tiles", [(1, 10, 10, 6, 0), (1, 12, 12, 5, 1), (2, 8, 8, 5, 0), (2, 10, 10, 6, 1), (3, 12, 10, 6, 0),
                                                                 (3, 10, 10, 5, 1), (0, 10, 10, 6, 0)])
def test_filter_controls_on_active_content_match_oracle(oracle, fmt, bd, bdc, log2_ctu, lf_across_tiles):
    """slice and tile borders, a slice with deblocking disabled, per-slice tc / beta / chroma QP offsets, QP per CU, lossless and PCM CUs in ONE
    picture whose edges the filter acts on (tests/test_filter_patterns_cpu.py: with the controls set to "filter" the oracle's picture differs
    at the borders of every kind): 3 x 2 tiles, five slices starting mid-row -- P, I, B, P, B, two of them listing the references the other way
    round, so that k_prep must take a neighbour CTU's references from the neighbour's own slice.  Slice-by-slice hmgpu_decompress_slice calls,
    then one hmgpu_decompress_pictures call"""
    for direction in ("ver", "hor"):
        p = fp.controls_picture(W, H, bd, bdc, fmt, log2_ctu, direction, lf_across_tiles)
        assert len(p.slices) == 5 and all(a % p.ctus_w for a, _ in p.slice_ranges[1:]) and len(set(p.meta_np["tile_idx"].tolist())) == 6
        assert [s.slice_type for s in p.slices] == [abi.P_SLICE, abi.I_SLICE, abi.B_SLICE, abi.P_SLICE, abi.B_SLICE]
        want = _oracle_stages(oracle, p)
        ctx, hc = _context(p)
        with ctx:
            what = "controls, format %d, %d / %d bits, CTU %d, tiles %d, %s, " % (fmt, bd, bdc, 1 << log2_ctu, lf_across_tiles, direction)
            _check_stages(ctx, hc, p, want, what + "slice by slice: ", stage_masks=(3,), per_slice_calls=True)
            _check_stages(ctx, hc, p, want, what + "one call: ", stage_masks=(1 if direction == "ver" else 2, 3))
