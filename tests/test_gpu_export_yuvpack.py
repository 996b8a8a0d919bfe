"""Packed YUV export on the GPU: hmgpu_pictures_export_yuvpack behind yuv= of Context.export_batch and Context.export.  The feature
adds no arithmetic, so every check is an equality of bytes against code that exists: the planar hmgpu_pictures_export_format of the
same pictures, crop or windows, flips and conversion at the words' chroma format and depth (held against numpy by
tests/test_gpu_export_format.py), laid out by the numpy model tests/yuvpack_ref.py, which is written from the header's table."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from libhm_amd import export as hexport
from tests import yuvpack_ref as yref
from tests.test_gpu_export_format import NAMES, Source, bits

pytestmark = pytest.mark.gpu

W, H = 72, 40
CROP = (0, 2, 0, 2)            # 70x38: 17.5 groups of four pairs, 11 2/3 groups of six pixels
CANARY = 0xA5
SOURCES = (0, 1, 2, 3)
OFFSETS = (2, 6)               # window left edges: pairs that are not 8-byte aligned
WIDTHS = (46, 50, 2)           # v210 tails of 4 and 2 pixels; a window narrower than one lane's unit
EINVAL, EUNSUPPORTED = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def sources():
    cache = {}

    def get(fmt, bd=8, w=W, h=H):
        key = (fmt, bd, w, h)
        if key not in cache:
            cache[key] = Source(fmt, w, h, bd, 70 + len(cache))
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def conversions(src, cf):
    """(chroma, chroma_down, chroma_loc) of every conversion the pair of formats tells apart: both up filters and the six sample
    locations where an axis gains samples next to a 4:2:0 side, both down rules where one loses them"""
    if src == 1:
        return [("replicate", "drop", 0)] + [("linear", "drop", loc) for loc in range(6)]
    if src == 2 and cf == 3:
        return [("replicate", "drop", 0), ("linear", "drop", 0)]
    if src == 3 and cf == 2:
        return [("linear", "drop", 0), ("linear", "linear", 0)]
    return [("linear", "linear", 3)]


def same_bytes(a, b):
    """equal shapes and bytes (16-bit unsigned tensors have few operators of their own)"""
    torch = _torch()
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def raw_rows(t, n):
    """a tensor of words [N, H, ...] as numpy bytes [N, H, bytes of a row]"""
    torch = _torch()
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(n, t.shape[1], -1)


def planar(s, fmt, pics, conv, **kw):
    """the planes the words must hold, per picture (y, cb, cr) as integers: the existing planar format export"""
    cf, d = yref.CHROMA[fmt], yref.DEPTH[fmt]
    got = s.ctx.export_batch(pics, "planar", d, chroma_format=NAMES[cf], chroma=conv[0], chroma_down=conv[1], chroma_loc=conv[2], **kw)
    p = [got[:, k] for k in range(3)] if cf == 3 else list(got)
    p = [bits(t) for t in p]
    return [(p[0][i], p[1][i], p[2][i]) for i in range(len(pics))]


def check(s, fmt, pics, conv, alpha=None, row_align=1, **kw):
    torch = _torch()
    got = s.ctx.export_batch(pics, yuv=fmt, alpha=alpha, chroma=conv[0], chroma_down=conv[1], chroma_loc=conv[2], row_align=row_align, **kw)
    want = planar(s, fmt, pics, conv, **kw)
    h, w = want[0][0].shape
    rb = yref.row_bytes(fmt, w)
    es = yref.ELEMENT[fmt]
    assert got.dtype == (torch.int32 if es == 4 else hexport.torch_dtype(es))
    shape = {"uyvy": (h, w, 2), "yuy2": (h, w, 2), "y210": (h, w, 2), "y216": (h, w, 2), "ayuv": (h, w, 4), "y416": (h, w, 4), "y410": (h, w),
             "v210": (h, -(-rb // max(row_align, 4)) * max(row_align, 4) // 4)}[fmt]
    assert tuple(got.shape) == (len(pics),) + shape
    rows = raw_rows(got, len(pics))
    for i, (y, cb, cr) in enumerate(want):
        assert np.array_equal(rows[i][:, :rb], yref.pack(fmt, y, cb, cr, alpha or 0)), (fmt, s.fmt, s.bd, conv, sorted(kw), i)
    return got


# ------------------------------------------------------------------------------------------------ every format, every source, every conversion
@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_against_the_planar_format_export(sources, fmt):
    for src in SOURCES:
        for bd in (8, 10):
            s = sources(src, bd)
            for conv in conversions(src, yref.CHROMA[fmt]):
                check(s, fmt, s.pics, conv, alpha=yref.ALPHA_MAX[fmt] // 2 + 1 if yref.ALPHA_MAX[fmt] else None)
                check(s, fmt, s.pics, conv, crop=CROP)


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_windows_and_mirrors(sources, fmt):
    """windows at offsets 2 and 6 of widths 46, 50 and 2, plain and mirrored in one batch; whole pictures and the crop mirrored"""
    for src, bd in ((1, 8), (2, 10), (3, 8), (0, 10)):
        s = sources(src, bd)
        conv = conversions(src, yref.CHROMA[fmt])[-1]
        for w in WIDTHS:
            wins = [(OFFSETS[0], 6, w, 26), (OFFSETS[1], 2, w, 26), (20, 12, w, 26)]
            for flip in (None, [True, False, True], [False, True, True]):
                check(s, fmt, s.pics, conv, windows=wins, flip=flip)
        check(s, fmt, s.pics, conv, flip=[True, True, False])
        check(s, fmt, s.pics, conv, crop=CROP, flip=[False, True, True])
    if yref.CHROMA[fmt] == 3:                                    # odd edges: a 4:4:4 source into 4:4:4 words
        s = sources(3, 10)
        check(s, fmt, s.pics, ("replicate", "drop", 0), windows=[(1, 1, 45, 25), (3, 0, 45, 25), (26, 15, 45, 25)], flip=[True, False, True])


@pytest.mark.parametrize("n", [1, 3, 16])
def test_batches(sources, n):
    s = sources(1, 10)
    pics = [s.pics[i % 3] for i in range(n)]
    for fmt in ("uyvy", "v210", "y410"):
        got = check(s, fmt, pics, ("linear", "drop", 2), crop=CROP, flip=[bool(i & 1) for i in range(n)])
        if n == 3:                                               # the repeated handle: slot 2 is slot 0 again; slot 1 was mirrored
            again = check(s, fmt, pics, ("linear", "drop", 2), crop=CROP, flip=[False, False, False])
            assert same_bytes(again[0], again[2]) and same_bytes(got[0], again[0]) and not same_bytes(got[1], again[1])
    one = s.ctx.export(s.pics[1], yuv="y210", chroma="linear", chroma_loc=2)
    assert one.shape == (H, W, 2) and same_bytes(one, s.ctx.export_batch(s.pics[1:2], yuv="y210", chroma="linear", chroma_loc=2)[0])


def test_the_depth_rule_both_ways(sources):
    """12-bit sources into the 8-, 10- and 16-bit words"""
    for src in (1, 3):
        s = sources(src, 12)
        for fmt in yref.FORMATS:
            check(s, fmt, s.pics, conversions(src, yref.CHROMA[fmt])[-1], crop=CROP, flip=[False, True, False])


def test_more_than_one_v210_line_per_row(sources):
    """264x200: five and a half 128-byte lines of 48 pixels a row"""
    s = sources(1, 10, 264, 200)
    check(s, "v210", s.pics, ("linear", "drop", 1), row_align=128)
    check(s, "v210", s.pics, ("linear", "drop", 1), windows=[(2, 6, 250, 180), (6, 2, 250, 180), (14, 20, 250, 180)], flip=[True, False, True])
    check(s, "y416", s.pics, ("linear", "drop", 1))
    check(s, "uyvy", s.pics, ("replicate", "drop", 0), flip=[True, False, True])


# ------------------------------------------------------------------------------------------------ destinations
def into(s, fmt, conv, off, pitch_extra, stride_extra, on_stream, crop=CROP, flip=None, n=3):
    """the entry itself into a buffer of canaries: (buffer bytes, expected bytes), the whole buffer"""
    torch = _torch()
    code = abi.YUVPACKS[fmt]
    d = yref.DEPTH[fmt]
    win = hexport.make_windows(s.seq, crop, None, flip, n)
    desc = abi.make_export_desc(abi.EXPORT_PLANAR, (d, d), 1 if d <= 8 else 2, 0, crop if win is None else (0, 0, 0, 0))
    f = abi.make_export_format(yref.CHROMA[fmt], conv[0], conv[1], conv[2])
    pk = abi.make_export_yuvpack(code, yref.ALPHA_MAX[fmt])
    st, plan = libhm_amd.export_yuvpack_status(s.seq, desc, None, win, f, pk)
    assert st == abi.HMGPU_OK
    h, w, rb = plan.height[0], plan.width[0], plan.row_bytes[0]
    pitch = rb + pitch_extra
    bstride = pitch * (h - 1) + rb + stride_extra
    size = 64 + off + (n - 1) * bstride + pitch * (h - 1) + rb + 64
    buf = torch.full((size + 256,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + (-buf.data_ptr() % 256) + 64 + off          # 64 + off beyond a 256-byte boundary
    lead = base - buf.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream if on_stream else 0
    s.ctx.export_yuvpack_into(s.pics[:n], desc, f, pk, base, pitch, bstride, 1 if on_stream else 0, stream, windows=win)
    if on_stream:
        torch.cuda.current_stream().synchronize()
    else:
        s.ctx.sync()
    kw = dict(crop=crop) if flip is None else dict(crop=crop, flip=flip)
    want = np.full((buf.numel(),), CANARY, np.uint8)
    for i, (y, cb, cr) in enumerate(planar(s, fmt, s.pics[:n], conv, **kw)):
        img = yref.pack(fmt, y, cb, cr, yref.ALPHA_MAX[fmt], pitch, canary=CANARY).reshape(-1)[:pitch * (h - 1) + rb]
        want[lead + i * bstride:lead + i * bstride + img.size] = img
    return buf.cpu().numpy(), want


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_pitch_stride_and_alignment_inside_canaries(sources, fmt):
    """a pitch and a batch stride beyond the least, addresses on and off 16-byte alignment (the format's own alignment, then 4 and 8
    bytes), both stream modes: the rows hold the words, every other byte of the buffer its canary"""
    es = yref.ELEMENT[fmt]
    for src, bd in ((1, 8), (3, 10)):
        s = sources(src, bd)
        conv = conversions(src, yref.CHROMA[fmt])[-1]
        for k, (off, pe, se) in enumerate(((0, 0, 0), (0, 32, 48), (es, 4 * es, 12 * es), (4, 12, 20), (8, 8, 24), (3 * es, 0, es))):
            got, want = into(s, fmt, conv, off, pe, se, on_stream=bool(k & 1), flip=[False, True, False] if k & 2 else None)
            assert np.array_equal(got, want), (fmt, src, off, pe, se)


def test_row_align_and_out(sources):
    """row_align=128 for v210 (the rows' tails stay unwritten), and out= views with rows and batch entries apart"""
    torch = _torch()
    s = sources(2, 10)
    conv = ("linear", "linear", 3)
    got = check(s, "v210", s.pics, conv, row_align=128)
    assert got.shape == (3, H, 64)                                # 72 pixels: 12 groups = 192 bytes -> 256
    rb = yref.row_bytes("v210", 70)
    big = torch.full((4, H, 96), -1, dtype=torch.int32, device="cuda")
    view = big[1:, 1:39, 8:8 + 64]                               # 70x38 into rows of 256 bytes, 32 bytes into a row of 384
    ret = s.ctx.export_batch(s.pics, yuv="v210", crop=CROP, out=view, row_align=128, chroma=conv[0], chroma_down=conv[1], chroma_loc=conv[2])
    assert ret is view
    torch.cuda.synchronize()
    want = planar(s, "v210", s.pics, conv, crop=CROP)
    rows = big.view(torch.uint8).cpu().numpy().reshape(4, H, 384)
    expect = np.full_like(rows, 0xFF)
    for i, (y, cb, cr) in enumerate(want):
        expect[1 + i, 1:39, 32:32 + rb] = yref.pack("v210", y, cb, cr)
    assert np.array_equal(rows, expect)
    for fmt in ("yuy2", "y416", "y410"):
        shape, dt, _ = hexport.yuvpack_shape(abi.YUVPACKS[fmt], libhm_amd.export_yuvpack_plan(
            s.seq, abi.make_export_desc(abi.EXPORT_PLANAR, 0, 0), None, None, abi.make_export_format(yref.CHROMA[fmt]), abi.make_export_yuvpack(fmt)))
        dt = torch.int16 if dt not in (torch.uint8, torch.int32) else dt           # (16-bit words: int16 holds the same bits)
        wide = torch.zeros((3, H + 2) + (shape[1] + 3,) + shape[2:], dtype=dt, device="cuda")
        view = wide[:, 1:H + 1, 2:2 + shape[1]]
        s.ctx.export_batch(s.pics, yuv=fmt, out=view, chroma="linear", chroma_down="linear")
        torch.cuda.synchronize()
        assert same_bytes(view, s.ctx.export_batch(s.pics, yuv=fmt, chroma="linear", chroma_down="linear"))
        assert (wide[:, 0] == 0).all() and (wide[:, -1] == 0).all() and (wide[:, :, :2] == 0).all() and (wide[:, :, -1] == 0).all()
    with pytest.raises(ValueError):
        s.ctx.export_batch(s.pics, yuv="uyvy", row_align=128)
    with pytest.raises(ValueError):
        s.ctx.export_batch(s.pics, yuv="nv16")


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_leave_the_destination_untouched(sources):
    torch = _torch()
    s = sources(3, 10)
    buf = torch.full((3 * H * W * 8 + 512,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + (-buf.data_ptr() % 256) + 64
    odd = [abi.make_export_window((1, W - 47, 0, H - 26))] * 3

    def run(fmt, desc="good", f="good", pk="good", ptrs=None, pitch=None, bstride=None, pics=None, **kw):
        d = yref.DEPTH[fmt]
        desc = abi.make_export_desc(abi.EXPORT_PLANAR, (d, d), 1 if d <= 8 else 2) if desc == "good" else desc
        f = abi.make_export_format(yref.CHROMA[fmt], 1, 1, 2) if f == "good" else f
        pk = abi.make_export_yuvpack(fmt) if pk == "good" else pk
        rb = yref.row_bytes(fmt, 46 if "windows" in kw else W)
        hh = 26 if "windows" in kw else H
        pitch = rb if pitch is None else pitch
        bstride = pitch * (hh - 1) + rb if bstride is None else bstride
        ptrs = [base] if ptrs is None else ptrs
        pics = s.pics if pics is None else pics
        st = s.ctx.export_yuvpack_status(pics, desc, f, pk, ptrs, [pitch], [bstride], **kw)
        if pics is s.pics:
            assert s.ctx.export_yuvpack_destination_status(3, desc, f, pk, ptrs, [pitch], [bstride], **kw) == st
        return st

    reserved = abi.make_export_yuvpack("uyvy")
    reserved.reserved[2] = 7
    for fmt in yref.FORMATS:
        d, cf, es = yref.DEPTH[fmt], yref.CHROMA[fmt], yref.ELEMENT[fmt]
        rb = yref.row_bytes(fmt, W)
        assert run(fmt, pk=None) == EINVAL and run(fmt, pk=reserved) == EINVAL
        assert run(fmt, pk=abi.make_export_yuvpack(8)) == EUNSUPPORTED and run(fmt, pk=abi.make_export_yuvpack(-1)) == EUNSUPPORTED
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_SEMIPLANAR, (d, d), 1 if d <= 8 else 2)) == EINVAL
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_RGB, (d, d), 1 if d <= 8 else 2)) == EINVAL
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_PLANAR, (d, 12 if d != 12 else 9), 1 if d <= 8 else 2)) == EINVAL
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_PLANAR, (d, d), 2 if d <= 8 else 1)) == EINVAL
        if d > 8:
            assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_PLANAR, (d, d), 2, 1)) == EINVAL
        assert run(fmt, f=None) == EINVAL and run(fmt, f=abi.make_export_format(5 - cf)) == EINVAL and run(fmt, f=abi.make_export_format(1)) == EINVAL
        assert run(fmt, pk=abi.make_export_yuvpack(fmt, yref.ALPHA_MAX[fmt] + 1)) == EINVAL and run(fmt, pk=abi.make_export_yuvpack(fmt, -1)) == EINVAL
        assert run(fmt, scale=abi.make_export_scale(36, 20)) == EUNSUPPORTED
        assert run(fmt, tensor=abi.make_export_tensor(abi.SAMPLE_F16)) == EUNSUPPORTED
        assert run(fmt, f=abi.make_export_format(cf, up=2)) == EUNSUPPORTED and run(fmt, f=abi.make_export_format(cf, loc=6)) == EINVAL
        if cf == 2:
            assert run(fmt, windows=odd) == EINVAL
        # the stated order: the format before the layout; the layout before a float tensor; a float tensor before the windows
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_RGB, (d, d), 2), pk=abi.make_export_yuvpack(9)) == EUNSUPPORTED
        assert run(fmt, desc=abi.make_export_desc(abi.EXPORT_RGB, (d, d), 2), tensor=abi.make_export_tensor(abi.SAMPLE_F32)) == EINVAL
        assert run(fmt, tensor=abi.make_export_tensor(abi.SAMPLE_F32), windows=[odd[0], odd[0], abi.make_export_window((0, 0, 0, 0))]) == EUNSUPPORTED
        # the destination
        assert run(fmt, ptrs=[base, base]) == EINVAL and run(fmt, ptrs=[base, None, base]) == EINVAL and run(fmt, ptrs=[None]) == EINVAL
        assert run(fmt, pitch=rb - es) == EINVAL and run(fmt, bstride=rb * H - es) == EINVAL
        if es > 1:
            assert run(fmt, ptrs=[base + es // 2]) == EINVAL and run(fmt, pitch=rb + es // 2) == EINVAL and run(fmt, bstride=rb * H + es // 2) == EINVAL
        assert run(fmt, bstride=1 << 40) == EINVAL                                        # the second picture leaves the allocation
        assert run(fmt, pics=s.pics[:2] + [99]) == EINVAL
    s.ctx.sync()
    torch.cuda.synchronize()
    assert (buf == CANARY).all()
    assert run("y416", windows=odd, tensor=abi.make_export_tensor(abi.SAMPLE_UINT)) == abi.HMGPU_OK      # odd edges: 4:4:4 into 4:4:4
    s.ctx.sync()
    assert not (buf == CANARY).all()
    for kw in (dict(size=(20, 36)), dict(dtype=torch.float32), dict(pixel="rgb"), dict(chroma_format="422"), dict(msb_aligned=True)):
        with pytest.raises(ValueError):
            s.ctx.export_batch(s.pics, yuv="uyvy", **kw)
