"""Picture metrics on the GPU (hmgpu_pictures_metrics, k_metrics.hip) behind Context.metrics: every field of every record against the
numpy model (tests/metrics_ref.py), exactly -- ssim_q32 within metrics_ref.tolerance(), whose docstring derives the bound.  Pictures are
416x240 -- partial CTUs, and partial 64 x 32 tiles, on both borders -- written with Context.upload."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, metrics
from tests import metrics_ref as mref
from tests import synth
from tests.test_gpu_motion import _hip

pytestmark = pytest.mark.gpu

W, H = 416, 240
NAMES = ("y", "cb", "cr")


def _torch():
    import torch
    return torch


def make_seq(fmt=1, bd=10, log2_ctu=6, max_pictures=8, bdc=None):
    seq = abi.make_seq(W, H, bd, bd if bdc is None else bdc, log2_ctu=log2_ctu, max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def depths(seq):
    return (seq.bit_depth_luma, seq.bit_depth_chroma)


def disturbed(planes, seq, seed, amp_div=8):
    """the planes plus uniform noise of amplitude about maxv / amp_div (a different one per seed), clipped to the coding range"""
    rng = np.random.RandomState(seed)
    out = []
    for k, p in enumerate(planes):
        maxv = (1 << depths(seq)[1 if k else 0]) - 1
        amp = max(1, int(maxv / amp_div * (0.25 + 1.5 * rng.rand())))
        out.append(np.clip(p.astype(np.int64) + rng.randint(-amp, amp + 1, size=p.shape), 0, maxv).astype(np.int16))
    return out


def source(seq, seed):
    return synth.smooth_planes(W, H, seq.bit_depth_luma, seed, seq.chroma_format, seq.bit_depth_chroma)


def check(out, want, where=""):
    """out: a result of Context.metrics; want: per picture the model's three records"""
    rec = metrics.records(out).cpu().numpy()
    assert rec.shape == (len(want), 3, 8) and rec.dtype == np.int64
    for i, recs in enumerate(want):
        for k in range(3):
            for f, name in enumerate(mref.FIELDS):
                got, exp = int(rec[i, k, f]), recs[k][name]
                assert int(out[NAMES[k]][name][i]) == got
                if name == "ssim_q32":
                    assert abs(got - exp) <= mref.tolerance(recs[k]["ssim_windows"]), (where, i, k, name, got, exp)
                else:
                    assert got == exp, (where, i, k, name, got, exp)
    return rec


def upload_all(ctx, planes_list):
    hs = []
    for p in planes_list:
        h = ctx.acquire()
        ctx.upload(h, p)
        hs.append(h)
    return hs


# ------------------------------------------------------------------------------------------------ 1. picture against picture
@pytest.mark.parametrize("n", [1, 3, 16])
def test_picture_against_picture_420_10bit(n):
    seq = make_seq(max_pictures=2 * n + 2)
    a = [source(seq, 10 + i) for i in range(n)]
    b = [disturbed(a[i], seq, 100 + i) for i in range(n)]
    if n >= 3:
        b[1] = [p.copy() for p in a[1]]                                # identical planes in another handle
        for k in range(3):                                             # exactly one sample: the last of the plane ...
            b[2][k] = a[2][k].copy()
            b[2][k][-1, -1] ^= 5
    if n >= 16:
        for k in range(3):                                             # ... and the first
            b[3][k] = a[3][k].copy()
            b[3][k][0, 0] ^= 64
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        if n >= 16:
            hb[4], b[4] = ha[4], a[4]                                    # a picture compared with itself
        out = ctx.metrics(ha, ref_pics=hb)
        want = [mref.picture(a[i], b[i], 1, depths(seq)) for i in range(n)]
        rec = check(out, want, "n=%d" % n)
        again = metrics.records(ctx.metrics(ha, ref_pics=hb)).cpu().numpy()
        assert again.tobytes() == rec.tobytes()                        # two calls: byte-identical
    if n >= 3:
        for k in range(3):
            w = want[1][k]
            assert (w["sse"], w["differing"], w["first_diff"], w["ssim_q32"]) == (0, 0, -1, w["ssim_windows"] << 32) and w["ssim_windows"] > 0
            assert int(rec[1, k, 5]) == w["ssim_windows"] << 32        # identical planes: exact
            assert want[2][k]["differing"] == 1 and want[2][k]["first_diff"] == want[2][k]["samples"] - 1
    if n >= 16:
        assert all(want[3][k]["first_diff"] == 0 and want[3][k]["differing"] == 1 for k in range(3))
        assert all(int(rec[4, k, 5]) == want[4][k]["ssim_windows"] << 32 for k in range(3))
    # the SSIM values spread: the amplitudes differ per picture
    vals = [metrics.ssim(out["y"])[i] for i in range(n) if want[i][0]["differing"] > 1]
    assert all(-1.0 < v < 0.999 for v in vals), vals
    ps = metrics.psnr(out["y"], 10)
    assert all(abs(ps[i] - mref.psnr(want[i][0]["samples"], want[i][0]["sse"], 10)) < 1e-9 for i in range(n))


@pytest.mark.parametrize("ssim", [False, True], ids=["plain", "ssim"])
def test_first_diff_is_the_least_index_not_the_first_one_a_lane_meets(ssim):
    """A lane does not meet its samples in index order: within a tile it covers several rows (r and r + 4 of a 256 x 8 tile, several
    block rows of a 64 x 32 one), then it moves one tile to the right, to rows above the ones it has just seen.  Here every picture
    differs in rows 4 .. 31 of the columns left of x0, rows 0 .. 3 there are equal, and one sample (x0, 0) differs: first_diff is x0.
    832x240, sixteen pictures: 2400 and 2112 tiles, so every workgroup walks 3 (without SSIM, a run of tiles 0 .. 2 of a row of four) or
    2 (with) neighbouring tiles -- with one tile per workgroup no lane sees two -- and x0 moves over the tiles from picture to picture,
    so that some tile that holds (x0, 0) follows its left neighbour in a run whatever the runs' phase."""
    w, h, n = 832, 240, 16
    seq = abi.make_seq(w, h, 10, 10, log2_ctu=6, max_pictures=n + 2)
    seq.chroma_format = 1
    a = synth.smooth_planes(w, h, 10, 70, 1, 10)
    b, x0s = [], []
    for i in range(n):
        planes, xs = [], []
        for p in a:
            q = p.copy()
            x0 = 64 * (1 + i % (p.shape[1] // 64 - 1)) + 6
            q[4:32, :x0 - 6] ^= 1
            q[0, x0] ^= 2
            planes.append(q)
            xs.append(x0)
        b.append(planes)
        x0s.append(xs)
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, [a]), upload_all(ctx, b)
        out = ctx.metrics(ha * n, ref_pics=hb, ssim=ssim)
        want = [mref.picture(a, b[i], 1, (10, 10), ssim=ssim) for i in range(n)]
        assert [[want[i][k]["first_diff"] for k in range(3)] for i in range(n)] == x0s
        check(out, want, "ssim=%d" % ssim)


# ------------------------------------------------------------------------------------------------ 2. crops
@pytest.mark.parametrize("crop", [(6, 10, 2, 14), (100, 304, 100, 128), (64, 0, 32, 0), (0, 288, 0, 176), (346, 2, 196, 4)],
                         ids=lambda c: "crop%d_%d_%d_%d" % c)
def test_crops_off_the_tile_grid_and_small_planes(crop):
    """window edges off the 64 x 32 tile grid and off the groups of 4 samples; the 12x12 luma crop leaves 6x6 chroma planes without a
    window; 128x64: exactly two tiles by two, the apron of the last ones outside the plane"""
    seq = make_seq()
    a = [source(seq, 20 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 200 + i, 8) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        for ssim in (True, False):
            out = ctx.metrics(ha, ref_pics=hb, crop=crop, ssim=ssim)
            want = [mref.picture(a[i], b[i], 1, depths(seq), crop=crop, ssim=ssim) for i in range(2)]
            check(out, want, crop)
    if crop == (100, 304, 100, 128):
        assert want[0][0]["samples"] == 144 and want[0][1]["samples"] == 36
        assert mref.picture(a[0], b[0], 1, depths(seq), crop=crop)[1]["ssim_windows"] == 0


# ------------------------------------------------------------------------------------------------ 3. formats and depths
@pytest.mark.parametrize("log2_ctu", [4, 6])
@pytest.mark.parametrize("bd", [8, 12])
@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_formats_and_depths(fmt, bd, log2_ctu):
    seq = make_seq(fmt, bd, log2_ctu)
    crop = {0: (3, 5, 1, 7), 2: (2, 6, 1, 3), 3: (1, 3, 5, 7)}[fmt]
    a = [source(seq, 30 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 300 + i) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        for cr in ((0, 0, 0, 0), crop):
            out = ctx.metrics(ha, ref_pics=hb, crop=cr)
            want = [mref.picture(a[i], b[i], fmt, depths(seq), crop=cr) for i in range(2)]
            rec = check(out, want, (fmt, bd, log2_ctu, cr))
            if fmt == 0:
                assert not rec[:, 1:, :].any()                         # components the format lacks: all zero


# ------------------------------------------------------------------------------------------------ 4. caller's planes
def padded_reference(planes_list, dtype, col0, extra_cols, extra_rows, canary):
    """per component one canary-filled tensor [n, h + extra_rows, col0 + w + extra_cols] and the view that holds the planes"""
    torch = _torch()
    full, views = [], []
    for k in range(3):
        stack = np.stack([p[k] for p in planes_list]).astype(np.int64)
        n, h, w = stack.shape
        host = np.full((n, h + extra_rows, col0 + w + extra_cols), canary, dtype=np.int64)
        host[:, 1:1 + h, col0:col0 + w] = stack
        host = host.astype(np.uint8 if dtype == "u8" else np.uint16)
        t = torch.from_numpy(host.view(np.uint8 if dtype == "u8" else np.int16)).cuda()
        full.append((t, host))
        views.append(t[:, 1:1 + h, col0:col0 + w])
    return full, views


@pytest.mark.parametrize("dtype,col0", [("u8", 4), ("u8", 3), ("u16", 4), ("u16", 1)], ids=["u8_aligned", "u8_odd", "u16_aligned", "u16_odd"])
def test_reference_planes_with_pitch_stride_and_canaries(dtype, col0):
    """the reference in the middle of a larger canary-filled allocation: pitch above the least pitch, a padded batch stride, the first
    column aligned for whole loads or not.  A canary read as a sample would show in the sums; none is changed."""
    torch = _torch()
    seq = make_seq(bd=8 if dtype == "u8" else 10)
    crop = (4, 8, 2, 6)
    n = 3
    a = [source(seq, 40 + i) for i in range(n)]
    b = [mref.crop_planes(disturbed(a[i], seq, 400 + i), crop, 1) for i in range(n)]
    canary = 0xA5 if dtype == "u8" else 0xA5A5
    full, views = padded_reference(b, dtype, col0, 5, 3, canary)
    with libhm_amd.Context(seq) as ctx:
        ha = upload_all(ctx, a)
        for ssim in (True, False):
            out = ctx.metrics(ha, ref=views, crop=crop, ssim=ssim)
            want = [[mref.plane(mref.crop_planes(a[i], crop, 1)[k], b[i][k], depths(seq)[1 if k else 0], ssim) for k in range(3)] for i in range(n)]
            check(out, want, (dtype, col0, ssim))
        torch.cuda.synchronize()
    for t, host in full:
        assert np.array_equal(t.cpu().numpy().view(host.dtype), host)


def test_uint16_reference_at_full_range():
    """65535 against samples of 0: max_abs and sse at the top of their range (65535^2 per sample), SSIM sums with the largest s2"""
    torch = _torch()
    seq = make_seq(bd=12)
    zero = [np.zeros_like(p) for p in source(seq, 1)]
    top = [np.full(p.shape, 65535, dtype=np.int64) for p in zero]
    ref = [torch.from_numpy(p.astype(np.uint16).view(np.int16)[None].copy()).cuda() for p in top]
    with libhm_amd.Context(seq) as ctx:
        h = upload_all(ctx, [zero])
        out = ctx.metrics(h, ref=ref)
        want = [[mref.plane(zero[k], top[k], 12) for k in range(3)]]
        check(out, want)
    assert want[0][0]["max_abs"] == 65535 and want[0][0]["sse"] == 65535 ** 2 * W * H and want[0][0]["first_diff"] == 0


# ------------------------------------------------------------------------------------------------ 5. subsets, no SSIM
@pytest.mark.parametrize("planes", [False, True], ids=["pictures", "planes"])
def test_component_subsets_and_distortion_only(planes):
    torch = _torch()
    seq = make_seq()
    a = [source(seq, 50 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 500 + i) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        full = None
        for comps in ((0, 1, 2), (0,), (1,), (2,), (0, 2), (1, 2)):
            if planes:
                ref = [torch.from_numpy(np.stack([b[i][k] for i in range(2)])).cuda() if k in comps else None for k in range(3)]
                kw = dict(ref=ref)
            else:
                kw = dict(ref_pics=hb)
            out = ctx.metrics(ha, components=comps, **kw)
            want = [mref.picture(a[i], b[i], 1, depths(seq), components=comps) for i in range(2)]
            rec = check(out, want, comps)
            for k in range(3):
                if k not in comps:
                    assert not rec[:, k, :].any()                      # not selected: all zero
            if full is None:
                full = rec
            else:
                for k in comps:
                    assert np.array_equal(rec[:, k, :], full[:, k, :])
            plain = metrics.records(ctx.metrics(ha, components=comps, ssim=False, **kw)).cpu().numpy()
            assert not plain[:, :, 5:7].any()                          # ssim_q32, ssim_windows
            keep = [0, 1, 2, 3, 4, 7]
            assert np.array_equal(plain[:, :, keep], rec[:, :, keep])


# ------------------------------------------------------------------------------------------------ 6. the final plane set
def test_a_picture_that_went_through_sao_is_read_from_its_final_planes():
    seq = make_seq(max_pictures=8)
    p = synth.make_picture(W, H, 10, seed=7, bi=False, intra_frac=0.0, num_refs=2, ref_handles=([0, 1], [1]), sao=True)
    with libhm_amd.Context(seq) as ctx:
        upload_all(ctx, [synth.noise_planes(W, H, 10, 5 + k) for k in range(2)])
        h, plain = ctx.acquire(), ctx.acquire()
        sao = abi.sao_array_from_raw(p.sao_raw)
        ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs), (plain, p.slices, p.meta, p.coeffs)])
        ctx.filter_pictures([(h, p.pp, sao)])
        ctx.filter_picture(plain, p.pp, p.sao_raw, stages=abi.STAGE_DEBLOCK_VER | abi.STAGE_DEBLOCK_HOR)
        final = ctx.download(h)
        copy = upload_all(ctx, [final])[0]
        out = ctx.metrics([h, h], ref_pics=[copy, plain])
        rec = check(out, [mref.picture(final, final, 1, (10, 10)), mref.picture(final, ctx.download(plain), 1, (10, 10))])
    assert not rec[0, :, 1:4].any() and (rec[0, :, 4] == -1).all()    # against the upload of its own download: no difference
    assert rec[1, 0, 3] > 0                                            # SAO changed samples: the deblocked planes are another picture


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_calls_leave_the_results_untouched():
    """the results and the Cr reference are allocations of their own (hipMalloc), exactly as large as a valid call needs"""
    torch = _torch()
    hip = _hip()
    seq = make_seq()
    a = [source(seq, 60 + i) for i in range(2)]
    CAN = 0x5A5A5A5A5A5A5A5A
    res_bytes, cr_bytes = 200 + 192, 2 * (H // 2) * (W // 2) * 2
    res, cr = C.c_void_p(), C.c_void_p()
    with libhm_amd.Context(seq) as ctx, libhm_amd.Context(seq) as other:
        ha = upload_all(ctx, a)
        upload_all(other, a + a)                                       # handles 0 .. 3 exist there, 2 and 3 not here
        assert hip.hipMalloc(C.byref(res), res_bytes) == 0 and hip.hipMalloc(C.byref(cr), cr_bytes) == 0
        try:
            assert hip.hipMemset(res, 0x5A, res_bytes) == 0 and hip.hipMemset(cr, 0, cr_bytes) == 0
            ref16 = [torch.zeros((2, H >> (1 if k else 0), W >> (1 if k else 0)), dtype=torch.int16, device="cuda") for k in range(2)]
            pic_desc = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
            pl_desc = abi.make_metrics_desc(abi.METRICS_REF_PLANES, 7, 1, 2)
            ptrs = [t.data_ptr() for t in ref16] + [cr.value]
            pitches = [W * 2, W, W]
            bstrides = [W * H * 2, W * H // 2, W * H // 2]
            stream = torch.cuda.current_stream().cuda_stream
            EINVAL = abi.HMGPU_EINVAL
            cases = [
                ("foreign handle", dict(pics=[0, 3], desc=pic_desc, ref_pics=ha)),
                ("foreign reference handle", dict(pics=ha, desc=pic_desc, ref_pics=[0, 2])),
                ("negative handle", dict(pics=[0, -1], desc=pic_desc, ref_pics=ha)),
                ("both references", dict(pics=ha, desc=pic_desc, ref_pics=ha, ptrs=ptrs, pitches=pitches, bstrides=bstrides)),
                ("neither reference", dict(pics=ha, desc=pic_desc)),
                ("planes wanted, pictures given", dict(pics=ha, desc=pl_desc, ref_pics=ha)),
                ("both references, planes", dict(pics=ha, desc=pl_desc, ref_pics=ha, ptrs=ptrs, pitches=pitches, bstrides=bstrides)),
                ("reference outside its allocation", dict(pics=ha, desc=pl_desc, ptrs=ptrs, pitches=pitches, bstrides=bstrides[:2] + [bstrides[2] + 2])),
                ("reference pitch outside its allocation", dict(pics=ha, desc=pl_desc, ptrs=ptrs, pitches=pitches[:2] + [W + 2], bstrides=bstrides)),
                ("pitch below the row", dict(pics=ha, desc=pl_desc, ptrs=ptrs, pitches=[pitches[0] - 2] + pitches[1:], bstrides=bstrides)),
                ("batch stride below the plane", dict(pics=ha, desc=pl_desc, ptrs=ptrs, pitches=pitches, bstrides=[bstrides[0] - 2] + bstrides[1:])),
                ("odd reference address", dict(pics=ha, desc=pl_desc, ptrs=[ptrs[0] + 1] + ptrs[1:], pitches=pitches, bstrides=bstrides)),
                ("a selected plane missing", dict(pics=ha, desc=pl_desc, ptrs=[ptrs[0], None, ptrs[2]], pitches=pitches, bstrides=bstrides)),
                ("a plane that is not compared", dict(pics=ha, desc=abi.make_metrics_desc(abi.METRICS_REF_PLANES, 1, 1, 2), ptrs=ptrs,
                                                      pitches=pitches, bstrides=bstrides)),
                ("uint8 planes at 10 bits", dict(pics=ha, desc=abi.make_metrics_desc(abi.METRICS_REF_PLANES, 7, 1, 1), ptrs=ptrs,
                                                 pitches=pitches, bstrides=bstrides)),
                ("misaligned results", dict(pics=ha, desc=pic_desc, ref_pics=ha, results=res.value + 4)),
                ("results stride below a picture's records", dict(pics=ha, desc=pic_desc, ref_pics=ha, stride=184)),
                ("results stride no multiple of 8", dict(pics=ha, desc=pic_desc, ref_pics=ha, stride=196)),
                ("results outside their allocation", dict(pics=ha, desc=pic_desc, ref_pics=ha, results=res.value + 16)),
                ("results stride outside their allocation", dict(pics=ha, desc=pic_desc, ref_pics=ha, stride=208)),
                ("host memory for the results", dict(pics=ha, desc=pic_desc, ref_pics=ha, results=np.zeros(64, np.int64).ctypes.data)),
                ("null results", dict(pics=ha, desc=pic_desc, ref_pics=ha, results=0)),
                ("17 pictures", dict(pics=[0] * 17, desc=pic_desc, ref_pics=[0] * 17)),
                ("no picture", dict(pics=[], desc=pic_desc, ref_pics=[])),
            ]
            for why, kw in cases:
                kw = dict(kw)
                pics, desc = kw.pop("pics"), kw.pop("desc")
                results, stride = kw.pop("results", res.value), kw.pop("stride", 192)
                assert ctx.metrics_status(pics, desc, results, stride, **kw) == EINVAL, why
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    ctx.metrics_into(pics, desc, results, stride, on_stream=1, stream=stream, **kw)
                assert e.value.status == EINVAL, why
            with pytest.raises(libhm_amd.HmgpuError):
                ctx.metrics_into(ha, pic_desc, res.value, 192, ref_pics=ha, on_stream=2)
            ctx.sync()
            torch.cuda.synchronize()
            got = np.zeros(res_bytes // 8, np.int64)
            assert hip.hipMemcpy(got.ctypes.data, res, res_bytes, 2) == 0 and (got == CAN).all()
            # the valid calls: the planes as they are; pictures with a padded results stride, whose gap is left alone
            assert ctx.metrics_status(ha, pl_desc, res.value, 192, ptrs=ptrs, pitches=pitches, bstrides=bstrides) == abi.HMGPU_OK
            assert ctx.metrics_status(ha, pic_desc, res.value, 200, ref_pics=ha) == abi.HMGPU_OK
            ctx.metrics_into(ha, pic_desc, res.value, 200, ref_pics=list(reversed(ha)), on_stream=1, stream=stream)
            torch.cuda.synchronize()
            assert hip.hipMemcpy(got.ctypes.data, res, res_bytes, 2) == 0
        finally:
            ctx.sync()
            hip.hipFree(res)
            hip.hipFree(cr)
    want = [mref.picture(a[i], a[1 - i], 1, (10, 10)) for i in range(2)]
    for i in range(2):
        for k in range(3):
            r = got[25 * i + 8 * k:25 * i + 8 * k + 8]
            for f, name in enumerate(mref.FIELDS):
                if name == "ssim_q32":
                    assert abs(int(r[f]) - want[i][k][name]) <= mref.tolerance(want[i][k]["ssim_windows"]), (i, k)
                else:
                    assert int(r[f]) == want[i][k][name], (i, k, name)
    assert got[24] == CAN
