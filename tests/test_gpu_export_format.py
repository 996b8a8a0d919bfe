"""The format export on the GPU: hmgpu_pictures_export_format behind chroma_format= of Context.export_batch and Context.export.
Every result is integer arithmetic that include/hmgpu.h states in full, so every comparison is an equality of bit patterns.  Two
yardsticks:
  1. independent: tests/export_format_ref.py (numpy) converts Cb and Cr, tests/export_ref.py applies the depth rule and the layout,
     tests/export_batch_ref.py the float map;
  2. for the call forms: a context of the OUTPUT format that holds the same luma and the model-converted chroma.  Its existing
     planar / semi-planar export (held against numpy by the existing tests) is what the new export must write, byte for byte."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from libhm_amd import export as hexport
from tests import export_batch_ref as bref
from tests import export_format_ref as fref
from tests import export_ref as ref
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

W, H = 72, 40                  # the coded picture (a context takes multiples of 8)
SIZES = [(72, 40), (70, 38)]   # chroma groups of 4: 72 -> 18 / 9 full groups; 70 -> 17.5 / 8.75: an odd number, and a last partial group
CROPS = {(72, 40): (0, 0, 0, 0), (70, 38): (0, 2, 0, 2)}       # 70x38 is the 72x40 picture without its last two columns and rows
BW, BH = 264, 200              # the scaled kernel's picture
CANARY = 0xA5
FORMATS = (0, 1, 2, 3)
NAMES = {0: "400", 1: "420", 2: "422", 3: "444"}
PAIRS = [(s, o) for s in FORMATS for o in FORMATS]
WINDOWS = [(2, 6, 44, 26), (6, 2, 44, 26), (24, 12, 44, 26)]     # left / top 2 and 6: chroma groups that are not 8-byte aligned


def _torch():
    import torch
    return torch


def raw(t):
    return t.contiguous().view(_torch().uint8)


def same(a, b):
    torch = _torch()
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return not isinstance(b, (tuple, list)) and a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def bits(t):
    """a tensor's elements as non-negative integers (their bit patterns for float types)"""
    torch = _torch()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().astype(np.int64) & ((1 << (8 * t.element_size())) - 1)


def planted_planes(fmt, w, h, bd, seed):
    """planes of random samples with, in chroma: the first and the last two columns and rows alternating between the extremes (a
    tap that is not clamped, or clamped one sample off, shows), and a checkerboard of 0 and the maximum in the middle (each weight
    product moves the result by many code values): what tests/test_gpu_export_chroma.py plants"""
    rng = np.random.default_rng(seed)
    m = (1 << bd) - 1
    p = [rng.integers(0, m + 1, (h, w)).astype(np.int16)]
    if fmt == 0:
        return p
    sx, sy = fref.shifts(fmt)
    for k in range(2):
        c = rng.integers(0, m + 1, (h >> sy, w >> sx)).astype(np.int16)
        lo, hi = (0, m) if k == 0 else (m, 0)
        c[:, 0], c[:, 1], c[:, -1], c[:, -2] = lo, hi, hi, lo
        c[0, :], c[1, :], c[-1, :], c[-2, :] = hi, lo, lo, hi
        c[0, 0], c[0, -1], c[-1, 0], c[-1, -1] = lo, lo, hi, hi
        yy, xx = np.mgrid[6:14, 8:24]
        c[6:14, 8:24] = np.where((yy + xx + k) & 1, m, 0)
        p.append(c)
    return p


class Source:
    """a context of one format, size and depth with two planted pictures (and the first again as a third handle), and on demand
    twins: contexts of another format that hold the same luma and the model-converted chroma"""

    def __init__(self, fmt, w, h, bd, seed):
        self.fmt, self.w, self.h, self.bd = fmt, w, h, bd
        self.seq = self.make_seq(fmt)
        self.ctx = libhm_amd.Context(self.seq)
        self.planes = [planted_planes(fmt, w, h, bd, 1000 * seed + 10 * fmt + i) for i in range(2)]
        self.pics = []
        for p in self.planes:
            self.pics.append(self.ctx.acquire())
            self.ctx.upload(self.pics[-1], p if fmt else p + [np.zeros((h // 2, w // 2), np.int16)] * 2)
        self.pics.append(self.pics[0])
        self.planes.append(self.planes[0])
        self.models, self.twins = {}, {}

    def make_seq(self, fmt):
        seq = abi.make_seq(self.w, self.h, self.bd, self.bd, max_pictures=8)
        seq.chroma_format = fmt
        return seq

    def model(self, out, up=0, down=0, loc=0):
        """the converted planes of every picture at the coding depth, computed once per conversion and never written again"""
        if self.fmt == 0 or out == 0 or out == self.fmt:
            key = (out, 0, 0, 0)
        else:
            gain = fref.shifts(self.fmt)[0] + fref.shifts(self.fmt)[1] > fref.shifts(out)[0] + fref.shifts(out)[1]
            key = (out, up if gain else 0, 0 if gain else down, loc if 1 in (self.fmt, out) else 0)
        if key not in self.models:
            self.models[key] = [fref.convert_planes(p, self.fmt, key[0], key[1], key[2], key[3], self.bd) for p in self.planes[:2]]
            self.models[key].append(self.models[key][0])
        return self.models[key]

    def twin(self, out, up=0, down=0, loc=0):
        """(context, handles) of the output format holding model(out, ...)"""
        m = self.model(out, up, down, loc)
        key = id(m)
        if key not in self.twins:
            ctx = libhm_amd.Context(self.make_seq(out))
            pics = []
            for p in m[:2]:
                pics.append(ctx.acquire())
                ctx.upload(pics[-1], p if out else p + [np.zeros((self.h // 2, self.w // 2), np.int16)] * 2)
            self.twins[key] = (ctx, pics + [pics[0]])
        return self.twins[key]

    def close(self):
        self.ctx.close()
        for ctx, _ in self.twins.values():
            ctx.close()


@pytest.fixture(scope="module")
def sources():
    cache = {}

    def get(fmt, size=SIZES[0], bd=8):
        key = (fmt, bd)                 # (size: the crop the caller exports, CROPS)
        if key not in cache:
            cache[key] = Source(fmt, W, H, bd, len(cache) + 1)
        return cache[key]
    yield get
    for s in cache.values():
        s.close()


def planes_of(out, layout, got):
    """the export's result as a list of per-plane tensors [N, ...]: the stacked [N, 3, H, W] of planar 4:4:4 split"""
    if layout == "planar" and out == 3:
        assert not isinstance(got, (tuple, list)) and got.dim() == 4 and got.shape[1] == 3
        return [got[:, k] for k in range(3)]
    assert isinstance(got, tuple)
    return list(got)


def expected(src, model, out, layout, out_bd, msb=False, crop=(0, 0, 0, 0)):
    """tests/export_ref.py on the model planes.  A 4:0:0 source: the model's constant is already at the chroma output depth"""
    bd = (src.bd, out_bd[1] if src.fmt == 0 else src.bd)
    return ref.export_yuv(model, out, bd, out_bd, ref.PLANAR if layout == "planar" else ref.SEMIPLANAR, crop, msb)


# ------------------------------------------------------------------------------------------------ yardstick 1: the numpy model
@pytest.mark.parametrize("src_fmt,out", PAIRS)
def test_against_the_model(sources, src_fmt, out):
    """all 16 format pairs x six sample locations x both up x both down x planar and semi-planar x both sizes, uint8 at 8 bits and
    uint16 at 10 (plain and msb_aligned)"""
    torch = _torch()
    for size in SIZES:
        for bd in (8, 10):
            s = sources(src_fmt, size, bd)
            converts = src_fmt != 0 and out != 0 and out != src_fmt
            for loc in (range(6) if converts else (0, 5)):
                for up, down in ((("replicate", "drop"), ("linear", "linear"), ("replicate", "linear"), ("linear", "drop")) if converts
                                 else (("linear", "linear"),)):
                    m = s.model(out, abi.CHROMA_FILTERS[up], abi.DOWN_FILTERS[down], loc)
                    for layout in ("planar", "semiplanar"):
                        for msb in ((False,) if bd == 8 else (False, True)):
                            got = s.ctx.export_batch(s.pics, layout, bd, CROPS[size], msb_aligned=msb, chroma_format=NAMES[out], chroma=up,
                                                     chroma_down=down, chroma_loc=loc)
                            got = planes_of(out, layout, got)
                            assert got[0].dtype == (torch.uint8 if bd == 8 else hexport.torch_dtype(2))
                            for i in range(3):
                                want = expected(s, m[i], out, layout, (bd, bd), msb, CROPS[size])
                                assert len(got) == len(want)
                                for k, wp in enumerate(want):
                                    assert np.array_equal(bits(got[k][i]), wp), (size, bd, loc, up, down, layout, msb, i, k)


def test_the_planted_content_tells_the_conversions_apart(sources):
    """the six types and the two filters give different planes, in both directions"""
    for src_fmt, out in ((1, 3), (3, 1)):
        s = sources(src_fmt, SIZES[0], 10)
        outs = [s.ctx.export_batch(s.pics[:1], "planar", 10, chroma_format=out, chroma="linear", chroma_down="linear", chroma_loc=k) for k in range(6)]
        outs.append(s.ctx.export_batch(s.pics[:1], "planar", 10, chroma_format=out))
        assert all(not same(outs[a], outs[b]) for a in range(7) for b in range(a)), (src_fmt, out)


@pytest.mark.parametrize("src_fmt,out", [(1, 3), (3, 1), (2, 1), (1, 2), (2, 3), (3, 2), (0, 3), (3, 0)])
def test_float_elements(sources, src_fmt, out):
    """float16 / bfloat16 / float32, per-plane mean and std: numpy's float32 multiply, add and astype on the model's integers"""
    torch = _torch()
    for size, bd in ((SIZES[0], 10), (SIZES[1], 8)):
        s = sources(src_fmt, size, bd)
        m = s.model(out, 1, 1, 3)
        for dtype, st in ((torch.float16, abi.SAMPLE_F16), (torch.bfloat16, abi.SAMPLE_BF16), (torch.float32, abi.SAMPLE_F32)):
            got = s.ctx.export_batch(s.pics, "planar", bd, CROPS[size], chroma_format=out, chroma="linear", chroma_down="linear", chroma_loc=3,
                                     dtype=dtype, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            got = planes_of(out, "planar", got)
            sc, bi = hexport.affine((bd,) * 3, bref.IMAGENET_MEAN, bref.IMAGENET_STD)
            t = abi.make_export_tensor(st, sc, bi)
            for i in range(3):
                want = bref.tensor_bits(expected(s, m[i], out, "planar", (bd, bd), False, CROPS[size]), t)
                assert len(got) == len(want) and all(g.dtype == dtype for g in got)
                for k, wp in enumerate(want):
                    assert np.array_equal(bits(got[k][i]), wp.astype(np.int64)), (size, bd, dtype, i, k)


def test_other_output_depths(sources):
    """the converted sample takes the decoded one's place in front of the bit-depth rule: 10 -> 8 rounds and clips, 8 -> 12 shifts;
    a 4:0:0 source writes 1 << (D - 1) of the chroma OUTPUT depth"""
    for src_fmt, out, bd, out_bd in ((1, 3, 10, (8, 8)), (3, 1, 10, (10, 8)), (2, 1, 8, (12, 12)), (0, 2, 8, (8, 12)), (0, 1, 10, (8, 8))):
        s = sources(src_fmt, SIZES[1], bd)
        m = s.model(out, 1, 1, 2) if src_fmt else [fref.convert_planes(p, 0, out, depth_chroma=out_bd[1]) for p in s.planes]
        for layout in ("planar", "semiplanar"):
            got = planes_of(out, layout, s.ctx.export_batch(s.pics, layout, out_bd, CROPS[SIZES[1]], chroma_format=out, chroma="linear",
                                                            chroma_down="linear", chroma_loc=2))
            for i in range(3):
                for k, wp in enumerate(expected(s, m[i], out, layout, out_bd, False, CROPS[SIZES[1]])):
                    assert np.array_equal(bits(got[k][i]), wp), (src_fmt, out, layout, i, k)


# ------------------------------------------------------------------------------------------------ yardstick 2: the twin of the output format
CALLS = [(1, 3, "linear", "drop", 3), (1, 3, "replicate", "drop", 0), (3, 1, "replicate", "linear", 0), (3, 1, "replicate", "linear", 5),
         (3, 1, "replicate", "drop", 0), (3, 2, "replicate", "linear", 1), (2, 1, "replicate", "linear", 2), (1, 2, "linear", "drop", 4),
         (2, 3, "linear", "drop", 0), (0, 1, "replicate", "drop", 0), (2, 0, "replicate", "drop", 0)]


def both(s, call, layout, idx=None, bit_depth=None, **kw):
    """(the format export of the source's pictures, the existing export of the twin's) with the same arguments; the stacked tensor
    of planar 4:4:4 as the tuple of planes the twin returns"""
    src_fmt, out, up, down, loc = call
    ctx, pics = s.twin(out, abi.CHROMA_FILTERS[up], abi.DOWN_FILTERS[down], loc)
    idx = range(3) if idx is None else idx
    bd = s.bd if bit_depth is None else bit_depth
    got = s.ctx.export_batch([s.pics[i] for i in idx], layout, bd, chroma_format=out, chroma=up, chroma_down=down, chroma_loc=loc, **kw)
    want = ctx.export_batch([pics[i] for i in idx], layout, bd, **{k: v for k, v in kw.items() if k != "out"})
    _torch().cuda.synchronize()
    if layout == "planar" and out == 3:
        got = tuple(got[:, k] for k in range(3))
    return got, want


@pytest.mark.parametrize("call", CALLS)
def test_windows_mirrors_and_batches(sources, call):
    """windows at offsets 2 and 6, mirrors, a batch of 3 with a repeated handle, at both sizes and depths, both layouts"""
    for size, bd in ((SIZES[0], 8), (SIZES[1], 10)):
        s = sources(call[0], size, bd)
        crop = CROPS[size]
        for layout in ("planar", "semiplanar"):
            got, want = both(s, call, layout, crop=crop)
            assert same(got, want), (size, layout)
            for flips in ([False, False, False], [True, False, True]):
                got, want = both(s, call, layout, crop=crop, windows=WINDOWS, flip=flips)
                assert same(got, want), (size, layout, flips)
            got, want = both(s, call, layout, idx=[1], crop=(4, 2, 2, 4), flip=[True])
            assert same(got, want), (size, layout, "crop")
            if bd == 10:
                got, want = both(s, call, layout, crop=crop, msb_aligned=True, windows=WINDOWS, flip=[False, True, False])
                assert same(got, want), (size, layout, "msb")
        got, want = both(s, call, "planar", crop=crop, windows=WINDOWS, flip=[True, False, False], dtype=_torch().float16, mean=bref.IMAGENET_MEAN,
                         std=bref.IMAGENET_STD)
        assert same(got, want), (size, "float16")


def test_window_of_the_export_is_the_export_of_the_window(sources):
    """taps outside the window but inside the decoded plane count"""
    for call in CALLS[:8]:
        src_fmt, out, up, down, loc = call
        s = sources(src_fmt, SIZES[0], 10)
        osx, osy = fref.shifts(out)
        kw = dict(chroma_format=out, chroma=up, chroma_down=down, chroma_loc=loc)
        full = planes_of(out, "planar", s.ctx.export_batch(s.pics, "planar", 10, **kw))
        part = planes_of(out, "planar", s.ctx.export_batch(s.pics, "planar", 10, windows=WINDOWS, **kw))
        for i, (x, y, w, h) in enumerate(WINDOWS):
            assert same(part[0][i], full[0][i, y:y + h, x:x + w])
            for k in (1, 2):
                assert same(part[k][i], full[k][i, y >> osy:(y + h) >> osy, x >> osx:(x + w) >> osx]), (call, i, k)


@pytest.mark.parametrize("on_stream", [True, False])
def test_stream_modes(sources, on_stream):
    torch = _torch()
    side = torch.cuda.Stream()
    for call in (CALLS[0], CALLS[3]):
        s = sources(call[0], SIZES[0], 10)
        ctx, _ = s.twin(call[1], abi.CHROMA_FILTERS[call[2]], abi.DOWN_FILTERS[call[3]], call[4])
        with torch.cuda.stream(side):
            got, want = both(s, call, "semiplanar", on_stream=on_stream)
            got2, want2 = both(s, call, "planar", on_stream=on_stream, windows=WINDOWS, flip=[False, True, True])
        if not on_stream:
            s.ctx.sync()
            ctx.sync()
        torch.cuda.synchronize()
        assert same(got, want) and same(got2, want2)


def test_strided_out_and_single_picture(sources):
    """out= in both forms: one [N, 3, H, W] view for planar 4:4:4, a tuple of plane views otherwise; rows, planes and batch entries
    further apart than dense, the canaries around them kept"""
    torch = _torch()
    s = sources(1, SIZES[0], 10)
    call = CALLS[0]
    ctx444, pics444 = s.twin(3, 1, 0, 3)
    store = torch.full((3, 4, 30, 50), 77, dtype=torch.int16, device="cuda")
    out = store[:, :3, 2:28, 3:47]
    ret = s.ctx.export_batch(s.pics, "planar", 10, windows=WINDOWS, chroma_format="444", chroma="linear", chroma_loc=3, out=out)
    want = ctx444.export_batch(pics444, "planar", 10, windows=WINDOWS)
    torch.cuda.synchronize()
    assert ret is out and all(torch.equal(out[:, k], want[k].view(torch.int16)) for k in range(3))
    assert (store[:, 3] == 77).all() and (store[:, :, :2] == 77).all() and (store[:, :, 28:] == 77).all() and (store[..., :3] == 77).all()
    with pytest.raises(ValueError):
        s.ctx.export_batch(s.pics, "planar", 10, chroma_format="444", out=tuple(out[:, k] for k in range(3)))
    # NV12-shaped views from a 4:4:4 source
    s3 = sources(3, SIZES[1], 8)
    ctx420, pics420 = s3.twin(1, 0, 1, 0)
    ys = torch.full((3, 40, 80), 77, dtype=torch.uint8, device="cuda")
    cs = torch.full((3, 21, 40, 2), 77, dtype=torch.uint8, device="cuda")
    s3.ctx.export_batch(s3.pics, "nv12", 8, CROPS[SIZES[1]], chroma_format="420", chroma_down="linear", out=(ys[:, 1:39, 5:75], cs[:, 1:20, 2:37]))
    want = ctx420.export_batch(pics420, "nv12", 8, CROPS[SIZES[1]])
    torch.cuda.synchronize()
    assert torch.equal(ys[:, 1:39, 5:75], want[0]) and torch.equal(cs[:, 1:20, 2:37], want[1])
    assert (ys[:, 0] == 77).all() and (ys[..., :5] == 77).all() and (cs[:, 20] == 77).all() and (cs[:, :, 37:] == 77).all() and (cs[:, :, :2] == 77).all()
    # Context.export: one picture, no batch dimension
    one = s.ctx.export(s.pics[1], "planar", 10, chroma_format="444", chroma="linear", chroma_loc=3)
    assert one.shape == (3, 40, 72) and all(same(one[k], w) for k, w in zip(range(3), ctx444.export(pics444[1], "planar", 10)))
    y, c = s3.ctx.export(s3.pics[1], "nv12", 8, chroma_format=1, chroma_down="linear", size=(20, 36))
    assert y.shape == (20, 36) and c.shape == (10, 18, 2)
    with pytest.raises(ValueError):
        s.ctx.export_batch(s.pics, "planar", 10, chroma_format="411")
    with pytest.raises(ValueError):
        s.ctx.export_batch(s.pics, "planar", 10, chroma_down="linear")


def test_unaligned_destinations_keep_their_canaries(sources):
    """destinations at odd byte offsets (no vector stores) inside canaries"""
    torch = _torch()
    for call, bd, layout in ((CALLS[0], 8, "semiplanar"), (CALLS[3], 10, "semiplanar"), (CALLS[6], 8, "planar"), (CALLS[7], 10, "planar")):
        s = sources(call[0], SIZES[1], bd)
        es, dt = (1, torch.uint8) if bd == 8 else (2, torch.int16)
        got, want = both(s, call, layout, crop=CROPS[SIZES[1]])
        for off in (es, 3 * es):
            bufs, outs = [], []
            for p in want:
                n = int(np.prod(p.shape))
                buf = torch.full((n * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
                bufs.append(buf)
                outs.append(buf[off:off + n * es].view(dt).view(p.shape))
            s.ctx.export_batch(s.pics, layout, bd, CROPS[SIZES[1]], chroma_format=call[1], chroma=call[2], chroma_down=call[3], chroma_loc=call[4],
                               out=tuple(outs))
            torch.cuda.synchronize()
            for buf, o, p in zip(bufs, outs, want):
                n = int(np.prod(p.shape)) * es
                assert torch.equal(raw(o), raw(p)) and (buf[:off] == CANARY).all() and (buf[off + n:] == CANARY).all(), (call, off)


# ------------------------------------------------------------------------------------------------ fixed properties
@pytest.mark.parametrize("fmt", FORMATS)
def test_output_equal_to_the_source_is_the_existing_call(sources, fmt):
    torch = _torch()
    s = sources(fmt, SIZES[1], 10)
    for layout in ("planar", "semiplanar"):
        for kw in ({}, dict(windows=WINDOWS, flip=[True, False, True]), dict(size=(24, 36), filter="bicubic"), dict(msb_aligned=True)):
            kw["crop"] = CROPS[SIZES[1]]
            got = s.ctx.export_batch(s.pics, layout, 10, chroma_format=fmt, chroma="linear", chroma_down="linear", chroma_loc=4, **kw)
            want = s.ctx.export_batch(s.pics, layout, 10, **kw)
            if layout == "planar" and fmt == 3:
                got = tuple(got[:, k] for k in range(3))
            assert same(got, want), (fmt, layout, kw)
    # through the entry itself, into canaries: the same bytes
    desc = abi.make_export_desc(abi.EXPORT_PLANAR, 10, 2, crop=CROPS[SIZES[1]])
    plan = libhm_amd.export_plan(s.seq, desc)
    bufs = []
    for use_new in (True, False):
        buf = torch.full((3 * 3 * 38 * 70 * 2 + 64,), CANARY, dtype=torch.uint8, device="cuda")
        ptrs = [buf.data_ptr() + 32 + k * 3 * 38 * 70 * 2 for k in range(3)]
        pitches = [plan.row_bytes[k] for k in range(3)]
        bs = [plan.row_bytes[k] * plan.height[k] for k in range(3)]
        if use_new:
            s.ctx.export_format_into(s.pics, desc, abi.make_export_format(fmt, 1, 1, 2), ptrs, pitches, bs)
        else:
            s.ctx.export_batch_into(s.pics, desc, ptrs, pitches, bs)
        bufs.append(buf)
    s.ctx.sync()
    assert torch.equal(bufs[0], bufs[1]) and not (bufs[0][32:-32] == CANARY).all()


# ------------------------------------------------------------------------------------------------ scaled
FILTERS = {"nearest": abi.SCALE_NEAREST, "bilinear": abi.SCALE_BILINEAR, "bicubic": abi.SCALE_BICUBIC, "area": abi.SCALE_AREA}


@pytest.fixture(scope="module")
def big():
    made = {}

    def get(fmt, w=BW, h=BH):
        if (fmt, w, h) not in made:
            made[fmt, w, h] = Source(fmt, w, h, 10, 50 + len(made))
        return made[fmt, w, h]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("size", [(64, 96), (232, 300)])
@pytest.mark.parametrize("src_fmt,out", [(1, 3), (3, 1)])
def test_scaled(big, src_fmt, out, size, filt):
    """264x200 -> 96x64 and -> 300x232.  Yardstick: the tables of hmgpu_export_format_scale_taps applied in numpy by scale_ref's
    rule; and for the chroma planes a context that already holds the source chroma planes as planes of the output geometry -- a
    4:4:4 picture of the source chroma size, a 4:2:0 picture of twice the source chroma size -- whose existing scaled export
    resamples them from the same size to the same size"""
    s = big(src_fmt)
    for layout in ("planar", "semiplanar"):
        d = abi.make_export_desc(abi.EXPORT_PLANAR if layout == "planar" else abi.EXPORT_SEMIPLANAR, 10, 2)
        sc = sref.scale_of(size, FILTERS[filt])
        f = abi.make_export_format(out, 1, 1, 2)
        plan = libhm_amd.export_format_plan(s.seq, d, sc, None, None, f)
        tabs = {(k, ax): libhm_amd.export_format_scale_taps(s.seq, d, sc, f, k, ax) for k in (0, 1) for ax in (0, 1)}
        got = planes_of(out, layout, s.ctx.export_batch(s.pics, layout, 10, size=size, filter=filt, chroma_format=out, chroma="linear",
                                                        chroma_down="linear", chroma_loc=2))
        for i in range(3):
            want = sref.export_scaled(s.planes[i], src_fmt, (10, 10), d, plan, tabs)
            assert len(got) == len(want)
            for k, wp in enumerate(want):
                assert np.array_equal(bits(got[k][i]), wp), (layout, i, k)
    # the twin geometry: chroma planes only (its luma is another picture)
    cw, ch = BW >> fref.shifts(src_fmt)[0], BH >> fref.shifts(src_fmt)[1]
    tw, th = (cw, ch) if out == 3 else (2 * cw, 2 * ch)
    pw, ph = -tw % 8, -th % 8                                   # (a context takes multiples of 8: the rest is cropped away again)
    t = big(out, tw + pw, th + ph)
    pic = t.ctx.acquire()
    t.ctx.upload(pic, [np.zeros((th + ph, tw + pw), np.int16)] + [np.pad(s.planes[1][k], ((0, ph), (0, pw))) for k in (1, 2)])
    want = t.ctx.export_batch([pic], "planar", 10, (0, pw, 0, ph), size=size, filter=filt)
    got = planes_of(out, "planar", s.ctx.export_batch([s.pics[1]], "planar", 10, size=size, filter=filt, chroma_format=out))
    t.ctx.release(pic)
    assert same(got[1], want[1]) and same(got[2], want[2])


def test_scaled_windows_crops_and_constants(big, sources):
    """windows that differ (per-picture tables), one crop for all (the table slot), float elements, the mirror; a 4:0:0 source keeps
    the constant, output 4:0:0 is the luma of the existing call"""
    torch = _torch()
    s = big(1)
    f = abi.make_export_format(3, 0, 0, 0)
    wins = [(2, 6, 200, 150), (6, 2, 258, 198), (0, 0, 264, 200)]
    for kw in (dict(windows=wins, flip=[True, False, False]), dict(crop=(6, 2, 2, 4))):
        got = s.ctx.export_batch(s.pics, "planar", 10, size=(64, 96), filter="bicubic", chroma_format="444", **kw)
        for i in range(3):
            x, y, w, h = wins[i] if "windows" in kw else (6, 2, 256, 194)
            d = abi.make_export_desc(abi.EXPORT_PLANAR, 10, 2, crop=(x, BW - x - w, y, BH - y - h))
            sc = abi.make_export_scale(96, 64, abi.SCALE_BICUBIC)
            plan = libhm_amd.export_format_plan(s.seq, d, sc, None, None, f)
            tabs = {(k, ax): libhm_amd.export_format_scale_taps(s.seq, d, sc, f, k, ax) for k in (0, 1) for ax in (0, 1)}
            want = sref.export_scaled(s.planes[i], 1, (10, 10), d, plan, tabs)
            for k in range(3):
                wp = want[k][:, ::-1] if "windows" in kw and kw["flip"][i] else want[k]
                assert np.array_equal(bits(got[i, k]), wp), (sorted(kw), i, k)
    m = sources(0, SIZES[0], 10)
    got = m.ctx.export_batch(m.pics, "semiplanar", (10, 8), size=(30, 52), chroma_format="420")
    want = m.ctx.export_batch(m.pics, "planar", (10, 8), size=(30, 52))
    assert same(got[0], want[0]) and got[1].shape == (3, 15, 26, 2) and (bits(got[1]) == 128).all()
    c = sources(2, SIZES[0], 10)
    got = c.ctx.export_batch(c.pics, "planar", 10, size=(30, 52), chroma_format="400", dtype=torch.float32)
    want = c.ctx.export_batch(c.pics, "planar", 10, size=(30, 52), dtype=torch.float32)
    assert len(got) == 1 and same(got[0], want[0])


# ------------------------------------------------------------------------------------------------ refusals
def destination(n, h, w, es):
    torch = _torch()
    buf = torch.full((n * 3 * h * w * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 32
    return buf, [base + k * n * h * w * es for k in range(3)], [w * es] * 3, [h * w * es] * 3


def test_refused_calls_leave_the_destination_untouched(sources):
    s = sources(3, SIZES[0], 10)
    W, H = SIZES[0]
    good = abi.make_export_desc(abi.EXPORT_PLANAR, 10, 2)
    fmt = abi.make_export_format(1, 1, 1, 2)
    reserved = abi.make_export_format(1, 1, 1, 2)
    reserved.reserved[0] = 1
    buf, ptrs, pitches, bs = destination(3, H, W, 2)
    EINVAL, EUNSUPPORTED = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    odd = [abi.make_export_window((1, W - 45, 0, H - 26))] * 3
    cases = [(abi.make_export_desc(abi.EXPORT_RGB, 10, 2), fmt, {}, EINVAL), (good, None, {}, EINVAL), (good, reserved, {}, EINVAL),
             (good, abi.make_export_format(4), {}, EINVAL), (good, abi.make_export_format(-1), {}, EINVAL),
             (good, abi.make_export_format(1, loc=6), {}, EINVAL), (good, abi.make_export_format(1, loc=-1), {}, EINVAL),
             (good, abi.make_export_format(1, up=2), {}, EUNSUPPORTED), (good, abi.make_export_format(1, down=2), {}, EUNSUPPORTED),
             (good, fmt, dict(windows=odd), EINVAL), (abi.make_export_desc(abi.EXPORT_PLANAR, 10, 2, crop=(0, 0, 1, 1)), fmt, {}, EINVAL),
             (good, fmt, dict(scale=abi.make_export_scale(31, 20)), EINVAL),
             (good, fmt, dict(scale=abi.make_export_scale(1, 1, abi.SCALE_AREA)), EUNSUPPORTED),
             (abi.make_export_desc(abi.EXPORT_SEMIPLANAR, 10, 2), fmt, dict(tensor=abi.make_export_tensor(abi.SAMPLE_F16)), EUNSUPPORTED),
             # the matching call's refusals come first, the format's own in their order
             (abi.make_export_desc(abi.EXPORT_PLANAR, 10, 1), abi.make_export_format(1, up=2), {}, EINVAL),
             (abi.make_export_desc(abi.EXPORT_RGB, 10, 2), abi.make_export_format(1, up=2), {}, EINVAL),
             (good, abi.make_export_format(5, up=2), {}, EINVAL), (good, abi.make_export_format(1, up=2), dict(windows=odd), EUNSUPPORTED)]
    for desc, f, kw, status in cases:
        with pytest.raises(libhm_amd.HmgpuError) as e:
            s.ctx.export_format_into(s.pics, desc, f, ptrs, pitches, bs, **kw)
        assert e.value.status == status, (status, e.value.status)
        assert s.ctx.export_format_destination_status(3, desc, f, ptrs, pitches, bs, **kw) == status
    # the destination against the plan of the OUTPUT format: the 4:2:0 chroma planes fit strides a quarter of the luma's ...
    small = [bs[0], bs[0] // 4, bs[0] // 4]
    half = [pitches[0], pitches[0] // 2, pitches[0] // 2]
    assert s.ctx.export_format_destination_status(3, good, fmt, ptrs, half, small) == abi.HMGPU_OK
    # ... which the picture's own format does not; one byte short is refused; a handle that is no picture
    assert s.ctx.export_format_destination_status(3, good, abi.make_export_format(3), ptrs, half, small) == EINVAL
    short = list(small)
    short[2] -= 1
    for bad_bs, pics in ((short, s.pics), (small, s.pics[:2] + [99])):
        with pytest.raises(libhm_amd.HmgpuError) as e:
            s.ctx.export_format_into(pics, good, fmt, ptrs, half, bad_bs)
        assert e.value.status == EINVAL
    s.ctx.sync()
    assert (buf == CANARY).all()
    s.ctx.export_format_into(s.pics, good, fmt, ptrs, half, small)
    s.ctx.sync()
    assert not (buf[32:-32] == CANARY).all() and (buf[:32] == CANARY).all() and (buf[-32:] == CANARY).all()
    with pytest.raises(libhm_amd.HmgpuError):
        s.ctx.export_batch(s.pics, "rgb", 10, chroma_format="420")
