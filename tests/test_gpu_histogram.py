"""Picture histograms on the GPU (hmgpu_pictures_histogram, k_histogram.hip) behind Context.histogram: every count and every field of
every record against the numpy model (tests/histogram_ref.py), exactly.  Pictures are 416x240 -- partial CTUs, and partial 256 x 8
tiles, on both borders -- written with Context.upload."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, histogram
from tests import export_ref
from tests import histogram_ref as href
from tests import synth
from tests.test_gpu_motion import _hip

pytestmark = pytest.mark.gpu

W, H = 416, 240
ALL = ("y", "cb", "cr", "maxrgb")


def _torch():
    import torch
    return torch


def make_seq(fmt=1, bd=10, bdc=None, w=W, h=H, max_pictures=8):
    seq = abi.make_seq(w, h, bd, bd if bdc is None else bdc, log2_ctu=6, max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def depths(seq):
    return (seq.bit_depth_luma, seq.bit_depth_chroma)


def source(seq, seed, amp_div=6):
    """smooth_planes plus uniform noise of about maxv / amp_div, clipped to the coding range: hundreds of occupied bins"""
    rng = np.random.RandomState(1000 + seed)
    out = []
    for k, p in enumerate(synth.smooth_planes(seq.width, seq.height, seq.bit_depth_luma, seed, seq.chroma_format, seq.bit_depth_chroma)):
        maxv = (1 << depths(seq)[1 if k else 0]) - 1
        amp = max(1, maxv // amp_div)
        out.append(np.clip(p.astype(np.int64) + rng.randint(-amp, amp + 1, size=p.shape), 0, maxv).astype(np.int16))
    return out


def coef_of(seq, matrix=1, full_range=0, rgb_bit_depth=0):
    return list(libhm_amd.histogram_plan(seq, ("maxrgb",), matrix=matrix, full_range=full_range, rgb_bit_depth=rgb_bit_depth).coef)


def upload_all(ctx, planes_list):
    hs = []
    for p in planes_list:
        h = ctx.acquire()
        ctx.upload(h, p)
        hs.append(h)
    return hs


def check(out, want, where="", with_hist=True):
    """out: a result of Context.histogram; want: per picture the model's four channels.  Returns (records, histograms) as numpy"""
    rec = histogram.records(out).cpu().numpy()
    assert rec.shape == (len(want), 4, 8) and rec.dtype == np.int64
    hists = {}
    for c, name in enumerate(href.NAMES):
        ch = out[name]
        on = want[0][c]["samples"] > 0
        assert ("hist" in ch) == (on and with_hist), (where, name)
        if "hist" in ch:
            hists[name] = ch["hist"].cpu().numpy()
            assert hists[name].dtype == np.int32 and hists[name].shape == (len(want), 1 << want[0][c]["log2_bins"]), (where, name)
        for i, chans in enumerate(want):
            w = chans[c]
            got = {"samples": int(rec[i, c, 0]), "sum": int(rec[i, c, 1]), "sum_sq": int(rec[i, c, 2]),
                   "min": int(rec[i, c, 3]) & 0xffffffff, "max": (int(rec[i, c, 3]) >> 32) & 0xffffffff}
            for f in href.FIELDS:
                assert got[f] == w[f], (where, i, name, f, got[f], w[f])
                assert int(ch[f][i]) == w[f], (where, i, name, f)
            assert not rec[i, c, 4:].any(), (where, i, name)              # the reserved words, the ticket among them
            if "hist" in ch:
                assert np.array_equal(hists[name][i].astype(np.int64), w["hist"]), (where, i, name)
    return rec, hists


# ------------------------------------------------------------------------------------------------ 1. formats, depths, batch sizes
@pytest.mark.parametrize("bd", [(8, 8), (10, 10), (12, 12), (10, 8)], ids=lambda d: "bd%d_%d" % d)
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_formats_depths_and_batch_sizes(fmt, bd):
    seq = make_seq(fmt, bd[0], bd[1], max_pictures=18)
    pics = [source(seq, 10 + i) for i in range(16)]
    coef = coef_of(seq)
    want = [href.picture(p, fmt, bd, (0, 1, 2, 3), coef=coef) for p in pics]
    for c in range(4):                                                  # natural-like content: hundreds of bins are occupied
        if want[0][c]["samples"]:
            assert int((want[0][c]["hist"] > 0).sum()) >= (100 if min(bd) == 8 else 200), (c, int((want[0][c]["hist"] > 0).sum()))
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        for n in (1, 3, 16):
            out = ctx.histogram(hs[:n], channels=ALL)
            rec, hists = check(out, want[:n], (fmt, bd, n))
            again = ctx.histogram(hs[:n], channels=ALL)
            assert histogram.records(again).cpu().numpy().tobytes() == rec.tobytes()        # two calls: byte-identical
            for name, h in hists.items():
                assert again[name]["hist"].cpu().numpy().tobytes() == h.tobytes()
            if fmt == 0:
                assert not rec[:, 1:3, :].any()                         # channels the format lacks: all zero


# ------------------------------------------------------------------------------------------------ 2. crops
@pytest.mark.parametrize("fmt,crop", [(1, (6, 4, 2, 8)), (3, (3, 1, 5, 7)), (1, (0, 6, 0, 2)), (2, (2, 0, 1, 0))],
                         ids=["420_unaligned", "444_odd", "420_right_edge", "422_left"])
def test_crops_with_unaligned_starts_and_partial_groups(fmt, crop):
    """starts off the 8- and 16-byte groups (every load of the picture sample by sample), widths that are no multiple of 4 (the last
    group of a row cut short, after whole loads where the start is aligned)"""
    seq = make_seq(fmt)
    pics = [source(seq, 20 + i) for i in range(2)]
    coef = coef_of(seq)
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        out = ctx.histogram(hs, channels=ALL, crop=crop)
        want = [href.picture(p, fmt, depths(seq), (0, 1, 2, 3), crop=crop, coef=coef) for p in pics]
        check(out, want, (fmt, crop))
    assert want[0][0]["samples"] == (W - crop[0] - crop[1]) * (H - crop[2] - crop[3])


# ------------------------------------------------------------------------------------------------ 3. extremes
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_extremes_and_a_minimum_above_the_zeroed_record(bd):
    """picture 0: value 0 at sample (0, 0) and 2^D - 1 at the last sample of every plane, everything else strictly between; picture 1:
    no sample below 64, so a min that stayed at the zero the record starts from would show"""
    seq = make_seq(1, bd)
    top = (1 << bd) - 1
    rng = np.random.RandomState(bd)
    a = [rng.randint(1, top, size=p.shape).astype(np.int16) for p in source(seq, 1)]
    for p in a:
        p[0, 0], p[-1, -1] = 0, top
    b = [np.maximum(p, 64 + k).astype(np.int16) for k, p in enumerate(source(seq, 2))]
    for k, p in enumerate(b):
        p[5, 7] = 64 + k
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, [a, b])
        out = ctx.histogram(hs, channels=ALL)
        want = [href.picture(p, 1, (bd, bd), (0, 1, 2, 3), coef=coef_of(seq)) for p in (a, b)]
        rec, hists = check(out, want, bd)
    for c, name in enumerate(("y", "cb", "cr")):
        assert (want[0][c]["min"], want[0][c]["max"]) == (0, top)
        assert hists[name][0][0] == 1 and hists[name][0][top] == 1        # both end bins
        assert want[1][c]["min"] == 64 + c and int(out[name]["min"][1]) == 64 + c
        assert not hists[name][1][:64].any()


# ------------------------------------------------------------------------------------------------ 4. flat pictures
@pytest.mark.parametrize("bd", [8, 10])
def test_flat_pictures_put_every_sample_into_one_bin(bd):
    """every sample equal, the chroma pair included: all 64 lanes of every wave add to one LDS word"""
    seq = make_seq(1, bd, max_pictures=18)
    vals = [(37 * i + 3) % (1 << bd) for i in range(16)]
    pics = [[np.full(p.shape, v, dtype=np.int16) for p in source(seq, 0)] for v in vals]
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        out = ctx.histogram(hs, channels=ALL)
        want = [href.picture(p, 1, (bd, bd), (0, 1, 2, 3), coef=coef_of(seq)) for p in pics]
        rec, hists = check(out, want, bd)
    for i, v in enumerate(vals):
        for name, samples in (("y", W * H), ("cb", W * H // 4), ("cr", W * H // 4)):
            assert hists[name][i][v] == samples and int((hists[name][i] > 0).sum()) == 1
        assert int((hists["maxrgb"][i] > 0).sum()) == 1 and hists["maxrgb"][i].max() == W * H


# ------------------------------------------------------------------------------------------------ 5. several tiles per workgroup
def test_runs_of_several_tiles_and_runs_that_cross_pictures():
    """832x240, sixteen pictures: 120 luma and 30 chroma tiles per picture, 2400 in all, so every workgroup walks three -- with one
    tile per workgroup no lane keeps sums across tiles and no run crosses from one (picture, class) to the next, which is where the
    bins are flushed and zeroed in the middle of a run (tests/test_gpu_metrics.py, the first-difference test, for the same reason)"""
    w, h, n = 832, 240, 16
    seq = make_seq(1, 10, w=w, h=h, max_pictures=n + 2)
    pics = [source(seq, 40 + i) for i in range(n)]
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        out = ctx.histogram(hs, channels=ALL)
        want = [href.picture(p, 1, (10, 10), (0, 1, 2, 3), coef=coef_of(seq)) for p in pics]
        check(out, want)


# ------------------------------------------------------------------------------------------------ 6. reduced bins, records only
@pytest.mark.parametrize("bd,bins", [(10, 256), (8, 16), (12, 4096), (10, 4096)], ids=["10bit_256", "8bit_16", "12bit_4096", "10bit_4096"])
def test_reduced_bins_and_records_only(bd, bins):
    seq = make_seq(2, bd)
    pics = [source(seq, 50 + i) for i in range(3)]
    log2 = bins.bit_length() - 1
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        out = ctx.histogram(hs, channels=ALL, bins=bins)
        want = [href.picture(p, 2, (bd, bd), (0, 1, 2, 3), log2_bins=log2, coef=coef_of(seq)) for p in pics]
        rec, hists = check(out, want, (bd, bins))
        assert hists["y"].shape[1] == min(bins, 1 << bd)
        full = ctx.histogram(hs, channels=ALL)
        assert histogram.records(full).cpu().numpy().tobytes() == rec.tobytes()                 # the records are over the values, not the bins
        b = min(log2, bd)
        for name in ALL:
            assert np.array_equal(full[name]["hist"].cpu().numpy().reshape(3, 1 << b, -1).sum(2), hists[name])
        only = ctx.histogram(hs, channels=ALL, bins=bins, histogram=False)
        check(only, want, (bd, bins, "records only"), with_hist=False)
        assert histogram.records(only).cpu().numpy().tobytes() == rec.tobytes()


# ------------------------------------------------------------------------------------------------ 7. channel subsets
def test_channel_subsets_leave_the_other_records_zero_and_the_gaps_alone():
    torch = _torch()
    seq = make_seq()
    pics = [source(seq, 60 + i) for i in range(2)]
    coef = coef_of(seq)
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        full, _ = check(ctx.histogram(hs, channels=ALL), [href.picture(p, 1, (10, 10), (0, 1, 2, 3), coef=coef) for p in pics])
        for chans in (("cb",), ("y", "maxrgb"), ("cr", "y"), ("maxrgb",), (2, 1)):
            idx = [href.NAMES.index(c) if isinstance(c, str) else c for c in chans]
            out = ctx.histogram(hs, channels=chans)
            rec, _ = check(out, [href.picture(p, 1, (10, 10), idx, coef=coef) for p in pics], chans)
            for c in range(4):
                assert np.array_equal(rec[:, c], full[:, c] if c in idx else np.zeros_like(full[:, c])), (chans, c)
        # the caller's own memory with padded strides: what lies between the histograms and between the records is left alone
        CAN = 0x5A5A5A5A
        hist = torch.full((2, 1024 + 8), CAN, dtype=torch.int32, device="cuda")
        unused = torch.full((2, 1024), CAN, dtype=torch.int32, device="cuda")
        rec = torch.full((2, 33), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        desc = histogram.describe(("cb",))
        ctx.histogram_into(hs, desc, rec.data_ptr(), 33 * 8, [None, hist.data_ptr(), None, None], [0, (1024 + 8) * 4, 0, 0], 1,
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got, r = hist.cpu().numpy(), rec.cpu().numpy()
        for i, p in enumerate(pics):
            assert np.array_equal(got[i, :1024].astype(np.int64), href.channel(p[1], 10)["hist"])
        assert (got[:, 1024:] == CAN).all() and (unused.cpu().numpy() == CAN).all() and (r[:, 32] == 0x5A5A5A5A5A5A5A5A).all()
        assert np.array_equal(r[:, :32].reshape(2, 4, 8), rec_of(ctx, hs, ("cb",)))


def rec_of(ctx, hs, chans):
    return histogram.records(ctx.histogram(hs, channels=chans, histogram=False)).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 8. maxRGB
def _export_max(ctx, hs, D, matrix, full_range, crop=(0, 0, 0, 0)):
    """max(R, G, B) per pixel of the device's own RGB export at D bits, int64 [n, H, W]"""
    torch = _torch()
    t = ctx.export_batch(hs, layout="rgb", bit_depth=D, matrix=matrix, full_range=full_range, crop=crop)
    v = t.long() if t.element_size() == 1 else t.view(torch.int16).long() & 0xffff
    return v.amax(1)


@pytest.mark.parametrize("fmt,matrix,full_range,rgb_depth",
                         [(f, m, r, (0, 8)[(f + m + r) & 1]) for f in (0, 1, 2, 3) for m in (1, 9) for r in (0, 1)] + [(3, 0, 0, 0), (3, 0, 0, 8), (1, 1, 0, 12)],
                         ids=lambda v: str(v))
def test_maxrgb_against_the_model_and_against_the_rgb_export(fmt, matrix, full_range, rgb_depth):
    """two independent checks: the model (export_ref.export_rgb with the plan's coef), and torch.bincount over the device's own RGB
    export of the same handles.  Picture 0 is uniform noise over the whole coding range -- saturated chroma against luma extremes --
    and picture 1 natural-like; the assertions on the model's sums before the clip say that each of R, G, B is the strict maximum
    somewhere and that the clip acts at both bounds.  (4:0:0 has R = G = B, no strict maximum, and at full range nothing to clip;
    the identity has no sums.)"""
    torch = _torch()
    seq = make_seq(fmt, 10, 10 if fmt != 2 else 8)                       # 4:2:2: unequal depths as well
    bd = depths(seq)
    D = rgb_depth or bd[0]
    pics = [synth.noise_planes(W, H, bd[0], 5, fmt, bd[1]), source(seq, 70)]
    coef = coef_of(seq, matrix, full_range, rgb_depth)
    crop = (2, 4, 6, 8) if fmt in (1, 3) else (0, 0, 0, 0)
    if matrix:
        cp = export_ref.crop_planes(pics[0], fmt, (0, 0, 0, 0))
        sx, sy = export_ref.chroma_shift(fmt)
        ry, rx = np.arange(H) >> sy, np.arange(W) >> sx
        u, v = (cp[k].astype(np.int64)[ry][:, rx] if fmt else np.full((H, W), 1 << (bd[1] - 1)) for k in (1, 2))
        clipped, sums = export_ref.rgb_int(cp[0].ravel(), u.ravel(), v.ravel(), coef)
        if fmt:
            for k in range(3):
                others = [j for j in range(3) if j != k]
                assert (clipped[k] > np.maximum(clipped[others[0]], clipped[others[1]])).any(), k
        if fmt or not full_range:
            assert ((sums >> coef[0]) < 0).any() and ((sums >> coef[0]) > coef[9]).any()
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        for cr in ((0, 0, 0, 0), crop):
            out = ctx.histogram(hs, channels=("y", "maxrgb"), crop=cr, matrix=matrix, full_range=full_range, rgb_bit_depth=rgb_depth)
            want = [href.picture(p, fmt, bd, (0, 3), crop=cr, coef=coef, rgb_bit_depth=rgb_depth) for p in pics]
            rec, hists = check(out, want, (fmt, matrix, full_range, rgb_depth, cr))
            assert hists["maxrgb"].shape[1] == 1 << D
            m = _export_max(ctx, hs, D, matrix, full_range, cr)
            for i in range(2):
                dev = torch.bincount(m[i].reshape(-1), minlength=1 << D)
                assert torch.equal(dev, out["maxrgb"]["hist"][i].long()), (fmt, matrix, full_range, rgb_depth, cr, i)
                assert int(m[i].sum()) == int(out["maxrgb"]["sum"][i]) and int(m[i].max()) == int(out["maxrgb"]["max"][i])


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refused_calls_leave_the_destinations_untouched():
    """the histograms and the records are allocations of their own (hipMalloc), exactly as large as a valid call needs"""
    torch = _torch()
    hip = _hip()
    seq = make_seq()
    pics = [source(seq, 80 + i) for i in range(2)]
    hist_bytes, rec_bytes = 2 * 4096, 2 * 256
    bufs = [C.c_void_p() for _ in range(3)]                            # Y histograms, Cb histograms, records
    sizes = [hist_bytes, hist_bytes, rec_bytes]
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        stale = upload_all(ctx, pics[:1])[0]
        ctx.release(stale)
        for b, s in zip(bufs, sizes):
            assert hip.hipMalloc(C.byref(b), s) == 0
        try:
            for b, s in zip(bufs, sizes):
                assert hip.hipMemset(b, 0x5A, s) == 0
            y, cb, rec = (b.value for b in bufs)
            desc = histogram.describe(("y", "cb"))
            only = histogram.describe(("y", "cb"), histogram=False)
            ptrs, strides = [y, cb, None, None], [4096, 4096, 0, 0]
            stream = torch.cuda.current_stream().cuda_stream
            cases = [
                ("stale handle", dict(pics=[hs[0], stale])),
                ("negative handle", dict(pics=[hs[0], -1])),
                ("hist NULL for a selected channel", dict(ptrs=[y, None, None, None])),
                ("hist for a channel that is not selected", dict(ptrs=[y, cb, cb, None], strides=[4096, 4096, 4096, 0])),
                ("hist in a records-only call", dict(desc=only)),
                ("no hist at all", dict(ptrs=None, strides=None)),
                ("stride below hist_bytes", dict(strides=[4092, 4096, 0, 0])),
                ("stride no multiple of 4", dict(ptrs=[y, cb, None, None], strides=[4096, 4098, 0, 0])),
                ("a span that leaves its allocation", dict(strides=[4096, 4100, 0, 0])),
                ("a start that leaves its allocation", dict(ptrs=[y + 4, cb, None, None])),
                ("misaligned histogram", dict(ptrs=[y + 2, cb, None, None])),
                ("misaligned records", dict(records=rec + 4)),
                ("records stride below 256", dict(stride=248)),
                ("records outside their allocation", dict(stride=264)),
                ("null records", dict(records=0)),
                ("host memory for the records", dict(records=np.zeros(64, np.int64).ctypes.data)),
                ("n = 0", dict(pics=[])),
                ("n = 17", dict(pics=[hs[0]] * 17)),
            ]
            for why, kw in cases:
                kw = dict(kw)
                p, d = kw.pop("pics", hs), kw.pop("desc", desc)
                records, stride = kw.pop("records", rec), kw.pop("stride", 256)
                pp, ss = kw.pop("ptrs", ptrs), kw.pop("strides", strides)
                assert ctx.histogram_status(p, d, records, stride, pp, ss) == abi.HMGPU_EINVAL, why
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    ctx.histogram_into(p, d, records, stride, pp, ss, on_stream=1, stream=stream)
                assert e.value.status == abi.HMGPU_EINVAL, why
            with pytest.raises(libhm_amd.HmgpuError):
                ctx.histogram_into(hs, desc, rec, 256, ptrs, strides, on_stream=2)
            ctx.sync()
            torch.cuda.synchronize()
            for b, s in zip(bufs, sizes):
                got = np.zeros(s, np.uint8)
                assert hip.hipMemcpy(got.ctypes.data, b, s, 2) == 0 and (got == 0x5A).all()
            # the accepted calls: records only without any hist argument, then the histograms
            assert ctx.histogram_status(hs, only, rec, 256) == abi.HMGPU_OK
            assert ctx.histogram_status(hs, desc, rec, 256, ptrs, strides) == abi.HMGPU_OK
            ctx.histogram_into(hs, desc, rec, 256, ptrs, strides, on_stream=1, stream=stream)
            torch.cuda.synchronize()
            got = [np.zeros(s // 4, np.int32) for s in sizes[:2]] + [np.zeros(rec_bytes // 8, np.int64)]
            for g, b, s in zip(got, bufs, sizes):
                assert hip.hipMemcpy(g.ctypes.data, b, s, 2) == 0
        finally:
            ctx.sync()
            for b in bufs:
                hip.hipFree(b)
    for i, p in enumerate(pics):
        for c in range(2):
            w = href.channel(p[c], 10)
            assert np.array_equal(got[c].reshape(2, 1024)[i].astype(np.int64), w["hist"])
            r = got[2].reshape(2, 4, 8)[i, c]
            assert (int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 0xffffffff, int(r[3]) >> 32) == tuple(w[f] for f in href.FIELDS)
        assert not got[2].reshape(2, 4, 8)[i, 2:].any()


# ------------------------------------------------------------------------------------------------ 10. the caller's stream
def test_a_dependent_op_on_the_callers_stream_sees_the_counts():
    torch = _torch()
    seq = make_seq()
    pics = [source(seq, 90 + i) for i in range(4)]
    with libhm_amd.Context(seq) as ctx:
        hs = upload_all(ctx, pics)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            out = ctx.histogram(hs, on_stream=True)
            total = out["y"]["hist"].long().sum(1) + out["cb"]["hist"].long().sum(1) + out["cr"]["hist"].long().sum(1)
            mean = histogram.mean(out["y"])
        side.synchronize()
        assert total.tolist() == [W * H * 3 // 2] * 4
        assert [abs(m - p[0].astype(np.float64).mean()) < 1e-9 for m, p in zip(mean.tolist(), pics)] == [True] * 4
        check(out, [href.picture(p, 1, (10, 10)) for p in pics])
