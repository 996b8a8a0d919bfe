"""Picture metric maps on the GPU (hmgpu_pictures_metrics_map, k_metrics_map.hip) behind Context.metrics_map: every element of every map
against the numpy model (tests/metrics_map_ref.py), exactly -- ssim_q32 within metrics_ref.tolerance() of the windows in the block per
element, and of the windows of the plane for the sum over a map (the bound tests/metrics_ref.py derives).  Pictures are 416x240 --
partial blocks at 32 and 64, none at 16, partial 64 x 64 regions on both borders -- written with Context.upload."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, metrics
from tests import metrics_map_ref as mmap
from tests import metrics_ref as mref
from tests import synth
from tests.test_gpu_motion import _hip
from tests.test_gpu_metrics import W, H, NAMES, depths, disturbed, make_seq, padded_reference, source, upload_all

pytestmark = pytest.mark.gpu

BLOCKS = (8, 16, 32, 64)
CAN = 0x5A5A5A5A5A5A5A5A


def _torch():
    import torch
    return torch


def compare(got, want, where=""):
    """got, want: [n, 3, F, Hb, Wb] int64"""
    assert got.shape == want.shape and got.dtype == np.int64, (where, got.shape, want.shape)
    for f, name in enumerate(mmap.FIELDS[:want.shape[2]]):
        if name != "ssim_q32":
            bad = np.argwhere(got[:, :, f] != want[:, :, f])
            assert not len(bad), (where, name, bad[:4].tolist(), [(int(got[i, k, f, y, x]), int(want[i, k, f, y, x])) for i, k, y, x in bad[:4]])
    if want.shape[2] == 6:
        delta = got[:, :, 4] - want[:, :, 4]
        assert (np.abs(delta) <= mmap.block_tolerance(want)).all(), (where, "ssim_q32", int(np.abs(delta).max()))
        total, windows = delta.sum(axis=(2, 3)), want[:, :, 5].sum(axis=(2, 3))
        assert (np.abs(total) <= 1 + windows // 1024).all(), (where, "ssim_q32 summed", total.tolist())


def check(out, want, where=""):
    """out: a result of Context.metrics_map"""
    got = metrics.maps(out).cpu().numpy()
    compare(got, want, where)
    for k in range(3):
        for f, name in enumerate(mmap.FIELDS[:want.shape[2]]):
            assert out[NAMES[k]][name].shape == want.shape[:1] + want.shape[3:]
            assert np.array_equal(out[NAMES[k]][name].cpu().numpy(), got[:, k, f])
    return got


def model(a, b, fmt, bds, B, **kw):
    return np.stack([mmap.picture(a[i], b[i], fmt, bds, B, **kw) for i in range(len(a))])


# ------------------------------------------------------------------------------------------------ 1. sizes, the sum rule, repeats
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("n", [1, 3, 16])
def test_picture_against_picture_420_10bit(n, B):
    seq = make_seq(max_pictures=2 * n + 2)
    a = [source(seq, 10 + i) for i in range(n)]
    b = [disturbed(a[i], seq, 100 + i) for i in range(n)]
    if n >= 3:
        b[1] = [p.copy() for p in a[1]]                                # identical planes in another handle
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        out = ctx.metrics_map(ha, ref_pics=hb, block=B)
        want = model(a, b, 1, depths(seq), B)
        got = check(out, want, (n, B))
        again = metrics.maps(ctx.metrics_map(ha, ref_pics=hb, block=B)).cpu().numpy()
        assert again.tobytes() == got.tobytes()                        # two calls: byte-identical
        # the sum rule on the device: the map summed in torch against Context.metrics of the same call
        rec = ctx.metrics(ha, ref_pics=hb)
        for name in NAMES:
            for f in ("sse", "sad", "differing", "ssim_windows"):
                assert bool((out[name][f].sum(dim=(1, 2)) == rec[name][f]).all()), (name, f)
            assert bool((out[name]["max_abs"].amax(dim=(1, 2)) == rec[name]["max_abs"]).all())
            d = (out[name]["ssim_q32"].sum(dim=(1, 2)) - rec[name]["ssim_q32"]).abs().tolist()
            assert all(v <= mref.tolerance(w) for v, w in zip(d, rec[name]["ssim_windows"].tolist())), (name, d)
    assert got.shape == (n, 3, 6, -(-H // B), -(-W // B))
    if n >= 3:
        assert not got[1, :, :4].any() and np.array_equal(got[1, :, 4], got[1, :, 5] << 32) and got[1, :, 5].sum() > 0
    assert got[0, :, 2].sum() > 0


# ------------------------------------------------------------------------------------------------ 2. single samples
def test_a_single_differing_sample_at_8_8():
    seq = make_seq()
    a = source(seq, 3)
    b = [p.copy() for p in a]
    for p in b:
        p[8, 8] ^= 256
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, [a]), upload_all(ctx, [b])
        out = ctx.metrics_map(ha, ref_pics=hb, block=8)
        got = check(out, model([a], [b], 1, depths(seq), 8), "single")[0]
    # luma: 8x8 blocks, the sample is the first of block (1, 1); chroma: 4x4 blocks, block (2, 2)
    for k, (by, bx) in enumerate(((1, 1), (2, 2), (2, 2))):
        want = np.zeros(got.shape[2:], np.int64)
        want[by, bx] = 1
        assert np.array_equal(got[k, 2], want) and np.array_equal(got[k, 0], want * 65536) and np.array_equal(got[k, 3], want * 256)
        below = got[k, 4] < (got[k, 5] << 32)
        hit = np.zeros(got.shape[2:], bool)
        if k == 0:
            hit[0:2, 0:2] = True                                       # windows at 0 .. 8: blocks (0, 0), (1, 0), (0, 1), (1, 1)
        else:
            hit[1:3, 1:3] = True                                       # windows at 4 and 8: one per 4x4 block
        assert np.array_equal(below, hit), k
        assert np.array_equal(got[k, 4][~hit], got[k, 5][~hit] << 32)


@pytest.mark.parametrize("B", BLOCKS)
def test_region_borders_the_apron_and_the_last_partial_block(B):
    """832x240, sixteen pictures, each with one differing sample: at luma (63, 31), (64, 32), (64, 63) and at the last sample of the
    plane (the chroma sample under it likewise) -- either side of a region's right and bottom border, whose windows start in the
    neighbouring region's blocks and read this region's apron; 240 = 3 * 64 + 48: the last block row is partial at 32 and 64"""
    w, h, n = 832, 240, 16
    seq = abi.make_seq(w, h, 10, 10, log2_ctu=6, max_pictures=n + 2)
    seq.chroma_format = 1
    a = synth.smooth_planes(w, h, 10, 70, 1, 10)
    spots = [(63, 31), (64, 32), (64, 63), (w - 1, h - 1)]
    b = []
    for i in range(n):
        x, y = spots[i % 4]
        planes = [p.copy() for p in a]
        planes[0][y, x] ^= 1 << (i % 9)
        for k in (1, 2):
            planes[k][y >> 1, x >> 1] ^= 1 << ((i + k) % 9)
        b.append(planes)
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, [a]), upload_all(ctx, b)
        out = ctx.metrics_map(ha * n, ref_pics=hb, block=B)
        got = check(out, model([a] * n, b, 1, (10, 10), B), B)
    for i in range(n):
        x, y = spots[i % 4]
        want = np.zeros(got.shape[3:], np.int64)
        want[y // B, x // B] = 1
        assert all(np.array_equal(got[i, k, 2], want) for k in range(3)), i


# ------------------------------------------------------------------------------------------------ 3. crops
@pytest.mark.parametrize("crop", [(6, 10, 2, 14), (2, 6, 2, 4), (100, 304, 100, 128), (64, 0, 32, 0), (0, 288, 0, 176), (346, 2, 196, 4)],
                         ids=lambda c: "crop%d_%d_%d_%d" % c)
def test_crops_off_the_block_grid_and_off_the_window_grid(crop):
    """the grid starts at the crop's top-left sample; (100, 304, 100, 128): 12x12 luma samples, 6x6 chroma planes without a window"""
    seq = make_seq()
    a = [source(seq, 20 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 200 + i, 8) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        for B in BLOCKS:
            for ssim in (True, False):
                out = ctx.metrics_map(ha, ref_pics=hb, block=B, crop=crop, ssim=ssim)
                got = check(out, model(a, b, 1, depths(seq), B, crop=crop, ssim=ssim), (crop, B, ssim))
                if crop == (100, 304, 100, 128) and ssim:
                    assert not got[:, 1:, 4:].any() and got[:, 0, 5].sum() == 8


# ------------------------------------------------------------------------------------------------ 4. formats and depths
@pytest.mark.parametrize("bd", [8, 12])
@pytest.mark.parametrize("fmt", [0, 2, 3])
def test_formats_and_depths(fmt, bd):
    seq = make_seq(fmt, bd)
    crop = {0: (3, 5, 1, 7), 2: (2, 6, 1, 3), 3: (1, 3, 5, 7)}[fmt]
    a = [source(seq, 30 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 300 + i) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        for cr in ((0, 0, 0, 0), crop):
            for B in BLOCKS:
                out = ctx.metrics_map(ha, ref_pics=hb, block=B, crop=cr)
                got = check(out, model(a, b, fmt, depths(seq), B, crop=cr), (fmt, bd, cr, B))
                if fmt == 0:
                    assert not got[:, 1:].any()                        # components the format lacks: zeroed from Python
    if fmt == 2:
        assert mmap.block_size(2, 8, 1) == (4, 8)


# ------------------------------------------------------------------------------------------------ 5. caller's planes
@pytest.mark.parametrize("dtype,col0", [("u8", 4), ("u8", 3), ("u16", 4), ("u16", 1)], ids=["u8_aligned", "u8_odd", "u16_aligned", "u16_odd"])
def test_reference_planes_with_pitch_stride_and_canaries(dtype, col0):
    """the reference in the middle of a larger canary-filled allocation, the first column aligned for whole loads or not.  A canary
    read as a sample would show in some block; none is changed."""
    torch = _torch()
    seq = make_seq(bd=8 if dtype == "u8" else 10)
    crop = (4, 8, 2, 6)
    n = 3
    a = [source(seq, 40 + i) for i in range(n)]
    b = [mref.crop_planes(disturbed(a[i], seq, 400 + i), crop, 1) for i in range(n)]
    full, views = padded_reference(b, dtype, col0, 5, 3, 0xA5 if dtype == "u8" else 0xA5A5)
    with libhm_amd.Context(seq) as ctx:
        ha = upload_all(ctx, a)
        for B in (8, 64):
            for ssim in (True, False):
                out = ctx.metrics_map(ha, ref=views, block=B, crop=crop, ssim=ssim)
                want = np.stack([mmap.cropped(mref.crop_planes(a[i], crop, 1), b[i], 1, depths(seq), B, W - 12, H - 8, ssim=ssim) for i in range(n)])
                check(out, want, (dtype, col0, B, ssim))
        torch.cuda.synchronize()
    for t, host in full:
        assert np.array_equal(t.cpu().numpy().view(host.dtype), host)


def test_uint16_reference_at_full_range():
    """65535 against samples of 0: sse at the top of its range (65535^2 per sample, 2^44 per 64 x 64 block)"""
    torch = _torch()
    seq = make_seq(bd=12)
    zero = [np.zeros_like(p) for p in source(seq, 1)]
    top = [np.full(p.shape, 65535, dtype=np.int64) for p in zero]
    ref = [torch.from_numpy(p.astype(np.uint16).view(np.int16)[None].copy()).cuda() for p in top]
    with libhm_amd.Context(seq) as ctx:
        h = upload_all(ctx, [zero])
        for B in (8, 64):
            out = ctx.metrics_map(h, ref=ref, block=B)
            got = check(out, model([zero], [top], 1, depths(seq), B), B)
            assert got[0, 0, 0, 0, 0] == 65535 ** 2 * B * B and got[0, 0, 3].min() == 65535 and got[0, 1, 2, 0, 0] == B * B // 4


# ------------------------------------------------------------------------------------------------ 6. the destination
def raw_call(ctx, pics, ref_pics, B, comps, ssim, buf, base, pitch, fstride, bstride, given=None, check_only=False):
    """hmgpu_pictures_metrics_map into the int64 tensor `buf`: component k's maps start at element base[k]; strides in elements.
    given: the components whose maps[c] is not NULL (default: comps)"""
    torch = _torch()
    desc = abi.make_metrics_desc(abi.METRICS_REF_PICTURES, sum(1 << k for k in comps), 1 if ssim else 0, 0)
    md = abi.make_metrics_map_desc(B)
    maps = [buf.data_ptr() + 8 * base[k] if k in (comps if given is None else given) else None for k in range(3)]
    args = (pics, desc, md, maps, [8 * pitch] * 3, [8 * fstride] * 3, [8 * bstride] * 3)
    if check_only:
        return ctx.metrics_map_status(*args, ref_pics=ref_pics)
    ctx.metrics_map_into(*args, ref_pics=ref_pics, on_stream=1, stream=torch.cuda.current_stream().cuda_stream)


def test_padded_destination_inside_canaries():
    """pitch, field stride and batch stride above the least ones: every byte outside the map elements stays as it was"""
    torch = _torch()
    seq = make_seq()
    n, B = 3, 32
    nbx, nby = mmap.grid(W, H, B)
    a = [source(seq, 60 + i) for i in range(n)]
    b = [disturbed(a[i], seq, 600 + i) for i in range(n)]
    pitch, fstride = nbx + 3, (nbx + 3) * nby + 5
    bstride = fstride * 6 + 7
    per = 11 + n * bstride
    base = [11 + k * per for k in range(3)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        buf = torch.full((3 * per + 11,), CAN, dtype=torch.int64, device="cuda")
        raw_call(ctx, ha, hb, B, (0, 1, 2), True, buf, base, pitch, fstride, bstride)
        host = buf.cpu().numpy()
    want = model(a, b, 1, depths(seq), B)
    got = np.zeros_like(want)
    written = np.zeros(host.shape, bool)
    for k in range(3):
        for i in range(n):
            for f in range(6):
                for y in range(nby):
                    s = base[k] + i * bstride + f * fstride + y * pitch
                    got[i, k, f, y] = host[s:s + nbx]
                    written[s:s + nbx] = True
    compare(got, want, "padded")
    assert (host[~written] == CAN).all() and written.sum() == want.size


def test_component_subsets_and_distortion_only():
    """maps[c] is NULL for the components left out, and nothing is written for them; without SSIM a six-field buffer keeps its
    fields 4 and 5"""
    torch = _torch()
    seq = make_seq()
    B = 16
    nbx, nby = mmap.grid(W, H, B)
    a = [source(seq, 50 + i) for i in range(2)]
    b = [disturbed(a[i], seq, 500 + i) for i in range(2)]
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        full = model(a, b, 1, depths(seq), B)
        for comps in ((0, 1, 2), (0,), (1,), (2,), (0, 2), (1, 2)):
            out = ctx.metrics_map(ha, ref_pics=hb, block=B, components=comps)
            got = check(out, model(a, b, 1, depths(seq), B, components=comps), comps)
            for k in range(3):
                assert np.array_equal(got[:, k, :4], full[:, k, :4]) if k in comps else not got[:, k].any()
            plain = ctx.metrics_map(ha, ref_pics=hb, block=B, components=comps, ssim=False)
            assert sorted(plain["y"]) == sorted(mmap.FIELDS[:4])
            assert np.array_equal(metrics.maps(plain).cpu().numpy(), got[:, :, :4])
            # the same into one canary-filled [3, n, 6, nby, nbx] buffer: a NULL map per component left out, four fields written
            buf = torch.full((3, 2, 6, nby, nbx), CAN, dtype=torch.int64, device="cuda")
            raw_call(ctx, ha, hb, B, comps, False, buf.view(-1), [k * buf.stride(0) for k in range(3)], nbx, nbx * nby, 6 * nbx * nby)
            host = buf.cpu().numpy()
            for k in range(3):
                if k in comps:
                    assert np.array_equal(host[k, :, :4], full[:, k, :4]) and (host[k, :, 4:] == CAN).all()
                else:
                    assert (host[k] == CAN).all()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refused_calls_leave_the_maps_untouched():
    """the three maps are allocations of their own (hipMalloc), exactly as large as the valid call needs"""
    torch = _torch()
    hip = _hip()
    seq = make_seq()
    B = 16
    nbx, nby = mmap.grid(W, H, B)
    plane = nbx * nby
    a = [source(seq, 60 + i) for i in range(2)]
    EINVAL = abi.HMGPU_EINVAL
    with libhm_amd.Context(seq) as ctx, libhm_amd.Context(seq) as other:
        ha = upload_all(ctx, a)
        upload_all(other, a + a)                                       # handles 0 .. 3 exist there, 2 and 3 not here
        nbytes = 2 * 6 * plane * 8
        bufs = [C.c_void_p() for _ in range(3)]
        for p in bufs:
            assert hip.hipMalloc(C.byref(p), nbytes) == 0 and hip.hipMemset(p, 0x5A, nbytes) == 0
        ptrs = [p.value for p in bufs]

        def download():
            got = [np.zeros(nbytes // 8, np.int64) for _ in range(3)]
            for g, p in zip(got, bufs):
                assert hip.hipMemcpy(g.ctypes.data, p, nbytes, 2) == 0
            return got
        stream = torch.cuda.current_stream().cuda_stream
        pic = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
        md = abi.make_metrics_map_desc(B)
        ok = dict(pics=ha, desc=pic, md=md, maps=ptrs, pitch=[nbx * 8] * 3, fs=[plane * 8] * 3, bs=[6 * plane * 8] * 3, ref_pics=ha)
        bad_md = abi.make_metrics_map_desc(B)
        bad_md.reserved[3] = 1
        ref16 = [torch.zeros((2, H >> (1 if k else 0), W >> (1 if k else 0)), dtype=torch.int16, device="cuda") for k in range(3)]
        planes_kw = dict(desc=abi.make_metrics_desc(abi.METRICS_REF_PLANES, 7, 1, 2), ref_pics=None, ptrs=[t.data_ptr() for t in ref16],
                         pitches=[W * 2, W, W], bstrides=[W * H * 2, W * H // 2, W * H // 2])
        cases = [
            ("foreign handle", dict(pics=[0, 3])),
            ("foreign reference handle", dict(ref_pics=[0, 2])),
            ("neither reference", dict(ref_pics=None)),
            ("17 pictures", dict(pics=[0] * 17, ref_pics=[0] * 17)),
            ("no picture", dict(pics=[], ref_pics=[])),
            ("a bad metrics description", dict(desc=abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 2))),
            ("a crop of half a chroma sample", dict(desc=abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (1, 0, 0, 0)))),
            ("block of 4", dict(md=abi.make_metrics_map_desc(4))),
            ("block of 128", dict(md=abi.make_metrics_map_desc(128))),
            ("block of 24", dict(md=abi.make_metrics_map_desc(24))),
            ("reserved word", dict(md=bad_md)),
            ("no map description", dict(md=None)),
            ("a map of a component the call does not select", dict(desc=abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 5))),
            ("a selected map missing", dict(maps=[ptrs[0], None, ptrs[2]])),
            ("no maps", dict(maps=None)),
            ("no strides", dict(bs=None)),
            ("misaligned map", dict(maps=[ptrs[0] + 4] + ptrs[1:])),
            ("pitch below the row", dict(pitch=[nbx * 8 - 8] * 3)),
            ("pitch no multiple of 8", dict(pitch=[nbx * 8 + 4] * 3)),
            ("field stride below the plane", dict(fs=[plane * 8 - 8] * 3)),
            ("batch stride below the fields", dict(bs=[6 * plane * 8 - 8] * 3)),
            ("map outside its allocation", dict(maps=[ptrs[0], ptrs[1] + 8, ptrs[2]])),
            ("batch stride outside the allocation", dict(bs=[6 * plane * 8 + 8] * 3)),
            ("host memory for a map", dict(maps=[np.zeros(2 * 6 * plane, np.int64).ctypes.data] + ptrs[1:])),
            ("planes: a missing reference", dict(planes_kw, ptrs=[planes_kw["ptrs"][0], None, planes_kw["ptrs"][2]])),
            ("planes: pitch below the row", dict(planes_kw, pitches=[W * 2 - 2, W, W])),
            ("planes and pictures", dict(planes_kw, ref_pics=ha)),
        ]
        for why, kw in cases:
            q = dict(ok)
            q.update(kw)
            args = (q["pics"], q["desc"], q["md"], q["maps"], q["pitch"], q["fs"], q["bs"])
            ref = dict(ref_pics=q["ref_pics"], ptrs=q.get("ptrs"), pitches=q.get("pitches"), bstrides=q.get("bstrides"))
            assert ctx.metrics_map_status(*args, **ref) == EINVAL, why
            with pytest.raises(libhm_amd.HmgpuError) as e:
                ctx.metrics_map_into(*args, on_stream=1, stream=stream, **ref)
            assert e.value.status == EINVAL, why
        with pytest.raises(libhm_amd.HmgpuError):
            ctx.metrics_map_into(ha, pic, md, ptrs, ok["pitch"], ok["fs"], ok["bs"], ref_pics=ha, on_stream=2)
        ctx.sync()
        torch.cuda.synchronize()
        assert all((g == CAN).all() for g in download())
        # the valid calls: pictures, and planes
        assert ctx.metrics_map_status(ha, pic, md, ptrs, ok["pitch"], ok["fs"], ok["bs"], ref_pics=ha) == abi.HMGPU_OK
        assert ctx.metrics_map_status(ha, planes_kw["desc"], md, ptrs, ok["pitch"], ok["fs"], ok["bs"], ptrs=planes_kw["ptrs"],
                                      pitches=planes_kw["pitches"], bstrides=planes_kw["bstrides"]) == abi.HMGPU_OK
        ctx.metrics_map_into(ha, pic, md, ptrs, ok["pitch"], ok["fs"], ok["bs"], ref_pics=list(reversed(ha)), on_stream=1, stream=stream)
        torch.cuda.synchronize()
        got = np.stack([g.reshape(2, 6, nby, nbx) for g in download()], axis=1)
        ctx.sync()
        for p in bufs:
            hip.hipFree(p)
    compare(got, model(a, a[::-1], 1, depths(seq), B), "valid")


# ------------------------------------------------------------------------------------------------ 8. the Python helpers
def test_python_helpers_against_the_model():
    torch = _torch()
    seq = make_seq()
    B = 32
    a = [source(seq, 80 + i) for i in range(3)]
    b = [disturbed(a[i], seq, 800 + i) for i in range(3)]
    b[1] = [p.copy() for p in a[1]]
    b[1][0][100, 200] ^= 1                                             # one sample of one picture: luma block (3, 6), no chroma
    b[2][1] = a[2][1].copy()
    b[2][1][:16, :16] ^= 1                                             # Cb of the third: block (0, 0) alone
    crop = (2, 6, 2, 4)                                                # the sample at (198, 98) of the crop
    with libhm_amd.Context(seq) as ctx:
        ha, hb = upload_all(ctx, a), upload_all(ctx, b)
        out = ctx.metrics_map(ha, ref_pics=hb, block=B, crop=crop)
        plan = libhm_amd.metrics_map_plan(seq, B, crop=crop)
        want = model(a, b, 1, depths(seq), B, crop=crop)
        for k, name in enumerate(NAMES):
            samples = metrics.map_samples(plan, k, device="cuda")
            assert np.array_equal(samples.cpu().numpy(), mmap.samples(W - 8, H - 6, 1, B, k))
            ps = metrics.map_psnr(out[name], samples, 10).cpu().numpy()
            ss = metrics.map_ssim(out[name]).cpu().numpy()
            assert ps.shape == ss.shape == want[:, k, 0].shape and ps.dtype == ss.dtype == np.float64
            sn = samples.cpu().numpy()
            for i, y, x in np.ndindex(*ps.shape):
                exp = mref.psnr(int(sn[y, x]), int(want[i, k, 0, y, x]), 10)
                assert abs(ps[i, y, x] - exp) <= 1e-9 * abs(exp), (k, i, y, x)
                wn = int(want[i, k, 5, y, x])
                if wn:
                    assert abs(ss[i, y, x] - want[i, k, 4, y, x] / 4294967296.0 / wn) < 1e-8
                else:
                    assert np.isnan(ss[i, y, x])
            idx = metrics.mismatch_blocks(out[name])
            assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), np.argwhere(want[:, k, 2] > 0))
        assert metrics.mismatch_blocks(out["y"])[(metrics.mismatch_blocks(out["y"])[:, 0] == 1)].tolist() == [[1, 98 // B, 198 // B]]
        assert metrics.mismatch_blocks(out["cb"])[(metrics.mismatch_blocks(out["cb"])[:, 0] >= 1)].tolist() == [[2, 0, 0]]
        assert float(metrics.map_psnr(out["cb"], metrics.map_samples(plan, 1), 10)[1].min()) == 999.99
    # the last block row of the cropped chroma plane (117 rows, blocks of 16) starts at 112: its windows would need rows up to 119
    assert np.isnan(metrics.map_ssim(out["cb"]).cpu().numpy()[:, -1]).all()
