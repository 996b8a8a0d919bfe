"""The picture margins a decoder reads through motion compensation, written by the border tiles of the fused loop filter
(k_filter_fused, put_margins) instead of a pass of k_extend over the finished picture.

The margins are observed the way a decoder observes them: picture A is decoded and filtered with SAO on in every CTU and component
(the fused path), then a P picture B predicts from A with vectors so long that TComDataCU::clipMv parks its prediction blocks in A's
margins, and B's planes are compared with the oracle's sample for sample.  Before any device call the test counts, from B's
metadata alone, the PUs whose clipped windows read each of the eight margin regions (left, right, above, below, four corners) of
luma and of chroma, and wants at least one per region: a pass says something about every margin.

Sizes: 64x64 one tile that is all four corners; 72x72 partial right and bottom tiles, 8 valid samples wide; 136x72 an interior tile
column between two border columns; 64x200 an interior tile row, the last tile row 8 valid rows high."""
import functools

import numpy as np
import pytest

from libhm_amd import abi
from tests import synth

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (72, 72), (136, 72), (64, 200)]
MV_RANGE = 160          # luma samples: beyond every picture size above plus what clipMv allows outside the picture
REGIONS = ("left", "right", "above", "below", "above left", "above right", "below left", "below right")


def _sao_everywhere(p, seed):
    """every CTU component that the drawn parameters leave off gets a band offset: SAO on in every CTU and component"""
    rng = np.random.RandomState(seed)
    raw = p.sao_raw
    for a in range(raw.shape[0]):
        for comp in range(3):
            if raw[a, comp, 0] == abi.SAO_OFF:
                band = int(rng.randint(0, 32))
                raw[a, comp, :] = 0
                raw[a, comp, 0], raw[a, comp, 1], raw[a, comp, 2] = abi.SAO_NEW, abi.SAO_BO, band
                for i in range(4):
                    raw[a, comp, 3 + (band + i) % 32] = int(rng.choice([-5, -2, 3, 6]))
    assert (raw[:, :, 0] == abi.SAO_NEW).all()


def _with_bypass_corners(p):
    """cu_transquant_bypass on every CU of the first and of the last CTU (the picture's corner CTUs): the NF variant of the kernel"""
    m = dict(p.meta_np)
    byp = np.zeros(m["depth"].shape, dtype=np.uint8)
    byp[0, :] = 1
    byp[-1, :] = 1
    m["bypass"], m["ipcm"] = byp, np.zeros_like(byp)
    p.meta_np, p.meta = m, abi.MetaHolder(m)


def margin_readers(p):
    """{"luma" / "chroma": {region: number of PUs of p whose window, after clipMv, holds samples of that margin region}}.  The window
    counted is the PU's block moved by the integer part of the clipped vector (the interpolation taps only widen it)."""
    m = p.meta_np
    w, h, ctu = p.width, p.height, 1 << p.log2_ctu
    use = p.inside & (m["pred_mode"] == 0) & (m["ref_idx0"] >= 0)
    cu = ctu >> m["depth"]
    cu_x, cu_y = p.px & ~(cu - 1), p.py & ~(cu - 1)
    mvx = np.minimum((w + 8 - cu_x - 1) << 2, np.maximum((-ctu - 8 - cu_x + 1) * 4, m["mv0"][:, :, 0]))
    mvy = np.minimum((h + 8 - cu_y - 1) << 2, np.maximum((-ctu - 8 - cu_y + 1) * 4, m["mv0"][:, :, 1]))
    pu = np.arange(p.num_ctus)[:, None] * 4096 + p.pu_idx
    out = {}
    for name, s, size in (("luma", 0, 4), ("chroma", 1, 2)):
        pw, ph = w >> s, h >> s
        x0, y0 = (p.px >> s) + (mvx >> (2 + s)), (p.py >> s) + (mvy >> (2 + s))          # the partition's block in the reference
        x1, y1 = x0 + size - 1, y0 + size - 1
        # per PU: the union of its partitions' blocks is a rectangle
        keys = np.unique(pu[use])
        reg = dict.fromkeys(REGIONS, 0)
        for k in keys:
            sel = use & (pu == k)
            xa, xb, ya, yb = x0[sel].min(), x1[sel].max(), y0[sel].min(), y1[sel].max()
            le, ri, ab, be = xa < 0, xb >= pw, ya < 0, yb >= ph
            rows_in, cols_in = yb >= 0 and ya < ph, xb >= 0 and xa < pw
            for r, hit in zip(REGIONS, (le and rows_in, ri and rows_in, ab and cols_in, be and cols_in, ab and le, ab and ri, be and le, be and ri)):
                reg[r] += bool(hit)
        out[name] = reg
    return out


def _assert_every_margin_is_read(p, what):
    got = margin_readers(p)
    for plane, reg in got.items():
        for r in REGIONS:
            assert reg[r] >= 1, "%s: no PU reads the %s margin %s of the reference (%s)" % (what, plane, r, reg)


@functools.lru_cache(maxsize=None)
def _pair(w, h, bd, log2_ctu, seed=0, nf=False, sao=True):
    """picture A (P, from the uploaded handle 0; SAO on everywhere, or off everywhere) and picture B that predicts from A with long vectors.
    Cached: shared by the tests, nobody may change them (B's reference handle is set per use on a clone of its slice)."""
    a = synth.make_picture(w, h, bd, seed=900 + 17 * seed + log2_ctu, ref_handles=([0], [0]), log2_ctu=log2_ctu, sao=sao)
    if sao:
        _sao_everywhere(a, 5 + seed)
    if nf:
        _with_bypass_corners(a)
    # (seed base 951: with it at least two PUs of every B below read each margin region, counted on the CPU; _assert_every_margin_is_read holds it)
    b = synth.make_picture(w, h, bd, seed=951 + 17 * seed + log2_ctu, ref_handles=([0], [0]), log2_ctu=log2_ctu, mv_range=MV_RANGE,
                            mode_probs=(0, 0, 0.25, 0.75, 0))        # 16x16 and 8x8 CUs: enough PUs in a picture of one tile
    return a, b


def _filtered(oracle, p, cur, refs):
    rec = [x.copy() for x in cur]
    oracle.decompress_ctus(p.seq, [p.slice], p.meta, p.coeffs, rec, refs)
    oracle.loop_filter_pic(p.seq, [p.slice], p.meta, p.pp, rec, 3)
    prm = oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw)
    return oracle.sao_process(p.seq, [p.slice], p.pp, p.meta, prm, rec)


def _predicted(oracle, p, cur, ref):
    rec = [x.copy() for x in cur]
    oracle.decompress_ctus(p.seq, [p.slice], p.meta, p.coeffs, rec, [ref])
    return rec


def _wants(oracle, a, b, ref0):
    zero = [np.zeros_like(x) for x in ref0]
    fin = _filtered(oracle, a, zero, [ref0])
    return fin, _predicted(oracle, b, zero, fin)


def _same(got, want, what):
    for c in range(3):
        if not np.array_equal(got[c], want[c]):
            bad = np.argwhere(got[c] != want[c])
            y, x = (int(v) for v in bad[0])
            raise AssertionError("%s, component %d: %d samples differ, first at (y, x) = (%d, %d): device %d, oracle %d"
                                 % (what, c, len(bad), y, x, got[c][y, x], want[c][y, x]))


def _seq(p, max_pictures=6):
    s = type(p.seq).from_buffer_copy(p.seq)
    s.max_pictures = max_pictures
    return s


def _decode(ctx, h, p, ref):
    sl = abi.clone_slice(p.slice)
    sl.ref_pic[0][0] = ref
    ctx.upload(h, [np.zeros((p.height, p.width), dtype=np.int16)] + [np.zeros((p.height >> 1, p.width >> 1), dtype=np.int16)] * 2)
    ctx.decompress_slice(h, 0, sl, p.meta, p.coeffs)


def _fused_kernel_ran(ctx):
    k = ctx.stats()["kernels"]
    return k["filter_fused"][1], k["extend_border"][1]


@pytest.mark.parametrize("log2_ctu", [4, 6])
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_prediction_from_the_margins_of_a_fused_filtered_picture(oracle, w, h, bd, log2_ctu):
    import libhm_amd
    a, b = _pair(w, h, bd, log2_ctu)
    what = "%dx%d, %d bits, CTU %d" % (w, h, bd, 1 << log2_ctu)
    _assert_every_margin_is_read(b, what)
    ref0 = synth.noise_planes(w, h, bd, 3)
    want_a, want_b = _wants(oracle, a, b, ref0)
    with libhm_amd.Context(_seq(a)) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        assert h0 == 0
        ctx.upload(h0, ref0)
        _decode(ctx, ha, a, h0)
        ctx.set_profiling(True)
        ctx.filter_picture(ha, a.pp, a.sao_raw)
        ctx.sync()
        fused, extend = _fused_kernel_ran(ctx)
        ctx.set_profiling(False)
        assert fused == 1 and extend == 0, "%s: the fused kernel must run and no border extension after it (%d, %d launches)" % (what, fused, extend)
        _same(ctx.download(ha), want_a, what + ": picture A")
        _decode(ctx, hb, b, ha)
        _same(ctx.download(hb), want_b, what + ": picture B, predicted from A's margins")


def test_exempt_cus_in_the_corner_ctus(oracle):
    """the kernel's variant for pictures with lossless CUs (NF): cu_transquant_bypass CUs fill A's first and last CTU"""
    import libhm_amd
    w, h, bd, log2_ctu = 136, 72, 10, 4
    a, b = _pair(w, h, bd, log2_ctu, nf=True)
    _assert_every_margin_is_read(b, "exempt CUs")
    ref0 = synth.noise_planes(w, h, bd, 3)
    want_a, want_b = _wants(oracle, a, b, ref0)
    with libhm_amd.Context(_seq(a)) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        _decode(ctx, ha, a, h0)
        ctx.filter_picture(ha, a.pp, a.sao_raw)
        _same(ctx.download(ha), want_a, "exempt CUs: picture A")
        _decode(ctx, hb, b, ha)
        _same(ctx.download(hb), want_b, "exempt CUs: picture B")


def test_batch_with_a_picture_without_sao_keeps_the_extension_kernel(oracle):
    """two pictures in one filter call, one with SAO off in every CTU: the stand-alone kernels and k_extend serve both"""
    import libhm_amd
    w, h, bd, log2_ctu = 72, 72, 10, 6
    a1, b = _pair(w, h, bd, log2_ctu)
    a2, _ = _pair(w, h, bd, log2_ctu, seed=1, sao=False)
    assert (a2.sao_raw[:, :, 0] == abi.SAO_OFF).all()
    _assert_every_margin_is_read(b, "mixed batch")
    ref0 = synth.noise_planes(w, h, bd, 3)
    wants = [_wants(oracle, a, b, ref0) for a in (a1, a2)]
    with libhm_amd.Context(_seq(a1)) as ctx:
        h0, h1, h2, hb = (ctx.acquire() for _ in range(4))
        ctx.upload(h0, ref0)
        for hh, a in ((h1, a1), (h2, a2)):
            ctx.upload(hh, [np.zeros_like(x) for x in ref0])
        ctx.decompress_pictures([(hh, [a.slice], a.meta, a.coeffs) for hh, a in ((h1, a1), (h2, a2))])
        ctx.set_profiling(True)
        ctx.filter_pictures([(hh, a.pp, abi.sao_array_from_raw(a.sao_raw)) for hh, a in ((h1, a1), (h2, a2))])
        ctx.sync()
        fused, extend = _fused_kernel_ran(ctx)
        ctx.set_profiling(False)
        assert fused == 0 and extend == 1, "the mixed batch takes the stand-alone route (%d fused, %d extension launches)" % (fused, extend)
        for k, hh in enumerate((h1, h2)):
            _same(ctx.download(hh), wants[k][0], "mixed batch: picture A%d" % k)
            _decode(ctx, hb, b, hh)
            _same(ctx.download(hb), wants[k][1], "mixed batch: picture B from A%d" % k)


@pytest.mark.parametrize("lanes", [1, 2])
def test_replayed_pictures_serve_as_references(oracle, lanes):
    """two pictures replayed twice (reconstruction and filters, stages 15) on one lane and on two: both are references like before"""
    import libhm_amd
    w, h, bd, log2_ctu = 136, 72, 10, 6
    a1, b = _pair(w, h, bd, log2_ctu)
    a2, _ = _pair(w, h, bd, log2_ctu, seed=1)
    _assert_every_margin_is_read(b, "replay")
    ref0 = synth.noise_planes(w, h, bd, 3)
    wants = [_wants(oracle, a, b, ref0) for a in (a1, a2)]
    with libhm_amd.Context(_seq(a1)) as ctx:
        h0, h1, h2, hb = (ctx.acquire() for _ in range(4))
        ctx.upload(h0, ref0)
        for hh in (h1, h2):
            ctx.upload(hh, [np.zeros_like(x) for x in ref0])
        ctx.decompress_pictures([(hh, [a.slice], a.meta, a.coeffs) for hh, a in ((h1, a1), (h2, a2))])
        ctx.filter_pictures([(hh, a.pp, abi.sao_array_from_raw(a.sao_raw)) for hh, a in ((h1, a1), (h2, a2))])
        ctx.set_streams(lanes)
        ctx.replay([h1, h2], 15, 2)
        ctx.set_streams(1)
        for k, hh in enumerate((h1, h2)):
            _same(ctx.download(hh), wants[k][0], "replay on %d lane(s): picture A%d" % (lanes, k))
            _decode(ctx, hb, b, hh)
            _same(ctx.download(hb), wants[k][1], "replay on %d lane(s): picture B from A%d" % (lanes, k))


def test_a_reused_handle_keeps_no_stale_margins(oracle):
    """A filtered in a handle, then a different A' decoded into the same handle and filtered: B' sees the margins of A'"""
    import libhm_amd
    w, h, bd, log2_ctu = 72, 72, 8, 4
    a1, b = _pair(w, h, bd, log2_ctu)
    a2, _ = _pair(w, h, bd, log2_ctu, seed=1)
    _assert_every_margin_is_read(b, "handle reuse")
    ref0 = synth.noise_planes(w, h, bd, 3)
    wants = [_wants(oracle, a, b, ref0) for a in (a1, a2)]
    for c in range(3):                                    # the two pictures differ along every border
        for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
            assert not np.array_equal(wants[0][0][c][edge], wants[1][0][c][edge])
    with libhm_amd.Context(_seq(a1)) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        for k, a in enumerate((a1, a2)):
            _decode(ctx, ha, a, h0)
            ctx.filter_picture(ha, a.pp, a.sao_raw)
            _decode(ctx, hb, b, ha)
            _same(ctx.download(hb), wants[k][1], "handle reuse: picture B from A%s" % ("'" if k else ""))


@pytest.mark.parametrize("w,h,log2_ctu,nf", [(64, 64, 6, False), (72, 72, 4, False), (136, 72, 6, True), (64, 200, 5, False)])
def test_region_equals_the_one_of_filter_then_extend(w, h, log2_ctu, nf):
    """the whole device region of a picture (planes, margins, spare lines: what a transfer carries) after the fused kernel equals the
    region of the same picture filtered stage by stage, where k_extend writes the margins"""
    import torch
    import libhm_amd
    from libhm_amd import frame_parallel as fp
    bd = 10
    a, _ = _pair(w, h, bd, log2_ctu, nf=nf)
    ref0 = synth.noise_planes(w, h, bd, 3)
    with libhm_amd.Context(_seq(a)) as ctx:
        h0, h1, h2 = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        _decode(ctx, h1, a, h0)
        ctx.filter_picture(h1, a.pp, a.sao_raw)
        _decode(ctx, h2, a, h0)
        ctx.filter_picture(h2, a.pp, a.sao_raw, stages=3)
        ctx.filter_picture(h2, a.pp, a.sao_raw, stages=4)
        ctx.sync()
        with torch.cuda.stream(torch.cuda.ExternalStream(ctx.stream_handle())):
            r1, r2 = fp.region_tensor(ctx, h1).cpu(), fp.region_tensor(ctx, h2).cpu()
        assert r1.numel() == r2.numel() and r1.numel() > 2 * w * h
        diff = torch.nonzero(r1 != r2)
        assert diff.numel() == 0, "%d bytes of the region differ, first at byte %d" % (diff.shape[0], int(diff[0]))
