"""The fused loop filter (k_filter_fused: both deblocking directions and SAO on 64x64 tiles in LDS) where its tiles end: pictures whose
last tile column and row are cut at every multiple of 8 the sizes below give, so that the last, short round of a thread's tile loads,
the addresses relative to a tile's first row at every picture border, and the state a workgroup keeps per picture (sizes, pitches,
bases of the planes and grids) all decide samples the oracle knows.  Pattern pictures (tests/filter_patterns.py) through one
filter call with SAO on, against the oracle's final planes, bit for bit.  The 520x328 pictures of tests/test_gpu_filter_patterns.py
stay the main yardstick of the arithmetic."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import filter_patterns as fp

pytestmark = pytest.mark.gpu

SIZES = [(72, 72), (200, 136), (136, 200), (264, 88)]      # tiles: 2 x 2 (8 samples of the second), 4 x 3, 3 x 4, 5 x 2


def _same(got, want, what):
    for c in range(3):
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            y, x = (int(v) for v in bad[0])
            raise AssertionError("%s, component %d: %d samples differ, first at (y, x) = (%d, %d): device %d, oracle %d"
                                 % (what, c, len(bad), y, x, got[c][y, x], want[c][y, x]))


def _oracle_stages(oracle, p, refs):
    """the oracle's picture after reconstruction from `refs` (planes per handle), after deblocking and after SAO"""
    rec = [np.zeros_like(a) for a in p.pat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, refs)
    dbk = [a.copy() for a in rec]
    oracle.loop_filter_pic(p.seq, p.slices, p.meta, p.pp, dbk, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    fin = oracle.sao_process(p.seq, p.slices, p.pp, p.meta, prm, dbk)
    return {"rec": rec, "dbk": dbk, "fin": fin}


def _assert_filters_act_at_the_borders(want, w, h, what):
    """both filters change luma samples in the last tile column and in the last tile row, SAO changes chroma samples"""
    x0, y0 = (w - 1) // 64 * 64, (h - 1) // 64 * 64
    for name, a, b in (("deblocking", want["rec"][0], want["dbk"][0]), ("SAO", want["dbk"][0], want["fin"][0])):
        assert (a[:, x0:] != b[:, x0:]).sum() > 0, "%s: %s changes nothing in the last tile column" % (what, name)
        assert (a[y0:, :] != b[y0:, :]).sum() > 0, "%s: %s changes nothing in the last tile row" % (what, name)
    assert sum(int((want["dbk"][c] != want["fin"][c]).sum()) for c in (1, 2)) > 0, "%s: SAO changes no chroma sample" % what


def _fused_once(p, want, what):
    """p through one context: the references hold the crafted picture, one decompress call, ONE filter call with SAO on (the fused path)"""
    import libhm_amd
    with libhm_amd.Context(p.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        assert (h0, h1) == (0, 1)
        ctx.upload(h0, p.pat)
        ctx.upload(h1, p.pat)
        ctx.upload(hc, [np.zeros_like(a) for a in p.pat])
        ctx.decompress_pictures([(hc, p.slices, p.meta, p.coeffs)])
        ctx.filter_picture(hc, p.pp, p.sao_raw)
        _same(ctx.download(hc), want["fin"], what)


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
@pytest.mark.parametrize("w,h,bd", [s + (10,) for s in SIZES] + [(200, 136, 8)])
def test_fused_filter_at_tile_and_picture_borders(oracle, w, h, bd, log2_ctu, direction):
    """every size x CTU size x direction: the copy's last vectors, the halo at all four picture borders (margins), tiles that hold 1, 4 or
    16 CTUs (SAO parameters and slice indices relative to the tile's first CTU), three slices"""
    p = fp.arith_picture(w, h, bd, bd, 1, log2_ctu, direction, sao_seed=7)
    want = _oracle_stages(oracle, p, [p.pat, p.pat])
    what = "%dx%d, %d bits, CTU %d, %s" % (w, h, bd, 1 << log2_ctu, direction)
    _assert_filters_act_at_the_borders(want, w, h, what)
    _fused_once(p, want, what)


@pytest.mark.parametrize("direction", ["ver", "hor"])
@pytest.mark.parametrize("log2_ctu", [4, 6])
def test_fused_filter_exempt_cus_at_the_borders(oracle, log2_ctu, direction):
    """the variant of the kernel for pictures with lossless / unfiltered PCM CUs (exempt sides of edge units, SAO groups that keep samples)"""
    w, h = 136, 200
    p = fp.variant_picture(w, h, 10, 10, 1, log2_ctu, direction, "exempt")
    assert p.bypass.any() and p.pcm.any() and p.pcm_loop_filter_disable == 1
    want = _oracle_stages(oracle, p, [p.pat, p.pat])
    what = "exempt CUs, %dx%d, CTU %d, %s" % (w, h, 1 << log2_ctu, direction)
    _assert_filters_act_at_the_borders(want, w, h, what)
    _fused_once(p, want, what)


BATCH = [("ver", 7), ("hor", 7), ("ver", 11), ("hor", 12), ("ver", 13)]


@pytest.fixture(scope="module")
def batch_pictures(oracle):
    """five different 200x136 pictures (direction of the content, SAO parameters) that predict from the same two references -- the
    crafted picture of the first --, each with the oracle's stages: shared by the batch sizes, read-only"""
    pics = [fp.arith_picture(200, 136, 10, 10, 1, 6, d, sao_seed=s) for d, s in BATCH]
    refs = [pics[0].pat, pics[0].pat]
    wants = [_oracle_stages(oracle, p, refs) for p in pics]
    for k, want in enumerate(wants):
        _assert_filters_act_at_the_borders(want, 200, 136, "batch picture %d" % k)
    for a in range(len(wants)):
        for b in range(a):
            assert not np.array_equal(wants[a]["fin"][0], wants[b]["fin"][0]) or not np.array_equal(wants[a]["fin"][1], wants[b]["fin"][1])
    return pics, wants


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_fused_filter_batch_of_different_pictures(batch_pictures, n):
    """n pictures in one decompress call and ONE filter call: 1 and 2 pictures take the banded tile-to-picture map, 3 and 5 the interleaved
    one (xcd_remap); every workgroup must work with the state of its own picture"""
    import libhm_amd
    pics, wants = batch_pictures
    with libhm_amd.Context(pics[0].seq) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        assert (h0, h1) == (0, 1)
        ctx.upload(h0, pics[0].pat)
        ctx.upload(h1, pics[0].pat)
        hs = [ctx.acquire() for _ in range(n)]
        for h, p in zip(hs, pics):
            ctx.upload(h, [np.zeros_like(a) for a in p.pat])
        ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs) for h, p in zip(hs, pics)])
        ctx.filter_pictures([(h, p.pp, abi.sao_array_from_raw(p.sao_raw)) for h, p in zip(hs, pics)])
        for k, (h, want) in enumerate(zip(hs, wants)):
            _same(ctx.download(h), want["fin"], "batch of %d, picture %d (%s, SAO seed %d)" % ((n, k) + BATCH[k]))
