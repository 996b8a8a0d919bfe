"""The chroma stage of the RGB exports on the GPU: hmgpu_pictures_export_chroma behind chroma="linear" of Context.export_batch and
Context.export.  Every result is integer arithmetic that include/hmgpu.h states in full, so every comparison is an equality of bit
patterns.  Two yardsticks:
  1. independent: tests/export_chroma_ref.py (numpy) upsamples Cb and Cr, tests/export_ref.py applies the published coef;
  2. for the combinations: a 4:4:4 context of the same size and depths whose pictures hold the same luma and the reference-upsampled
     chroma.  Its existing export (held against numpy by the existing tests) is what the new export of the 4:2:0 picture must write,
     byte for byte, in every form the export has."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import export_batch_ref as bref
from tests import export_chroma_ref as chref
from tests import export_ref as ref

pytestmark = pytest.mark.gpu

W, H = 72, 40              # 36 x 20 chroma samples: several groups of 4 per row, the last group of a row partial (72 = 18 * 4)
BW, BH = 264, 200          # the scaled kernel's picture
CANARY = 0xA5
LOCS = range(6)
FORMS = [None, "rgb", "bgr", "rgba", "bgra", "argb", "abgr", "cl"]


def _torch():
    import torch
    return torch


def raw(t):
    """a tensor's bytes in logical order"""
    torch = _torch()
    return t.contiguous().view(torch.uint8)


def same(a, b):
    torch = _torch()
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def planted_planes(w, h, bd, seed):
    """4:2:0 planes of random samples with, in chroma: the first and the last two columns and rows alternating between the extremes
    (each differs strongly from its neighbour, so a tap that is not clamped, or clamped one sample off, shows), and a checkerboard
    of 0 and the maximum in the middle (neighbouring samples differ by the full range, so each of the sixteen weight products moves
    the result by many code values)"""
    rng = np.random.default_rng(seed)
    m = (1 << bd) - 1
    p = [rng.integers(0, m + 1, (h, w)).astype(np.int16)] + [rng.integers(0, m + 1, (h // 2, w // 2)).astype(np.int16) for _ in range(2)]
    for k, c in enumerate(p[1:]):
        lo, hi = (0, m) if k == 0 else (m, 0)
        c[:, 0], c[:, 1], c[:, -1], c[:, -2] = lo, hi, hi, lo
        c[0, :], c[1, :], c[-1, :], c[-2, :] = hi, lo, lo, hi
        c[0, 0], c[0, -1], c[-1, 0], c[-1, -1] = lo, lo, hi, hi
        yy, xx = np.mgrid[6:14, 8:24]
        c[6:14, 8:24] = np.where((yy + xx + k) & 1, m, 0)
    return p


class Pair:
    """a 4:2:0 context and a 4:4:4 context of one size and depth; picture i of the first with chroma_sample_loc_type `loc` is
    picture (i, loc) of the second"""

    def __init__(self, w, h, bd, count, locs, seed):
        self.w, self.h, self.bd = w, h, bd
        self.seq = abi.make_seq(w, h, bd, bd, max_pictures=16)
        self.seq444 = abi.make_seq(w, h, bd, bd, max_pictures=16)
        self.seq444.chroma_format = 3
        self.planes = [planted_planes(w, h, bd, 100 * seed + i) for i in range(count)]
        self.ctx, self.ctx444 = libhm_amd.Context(self.seq), libhm_amd.Context(self.seq444)
        self.pics, self.pics444, self.up = [], {}, {}
        for p in self.planes:
            self.pics.append(self.ctx.acquire())
            self.ctx.upload(self.pics[-1], p)
        for loc in locs:
            for i, p in enumerate(self.planes):
                self.up[i, loc] = chref.upsample_planes(p, 1, loc)        # computed once, shared, never written again
                self.pics444[i, loc] = self.ctx444.acquire()
                self.ctx444.upload(self.pics444[i, loc], self.up[i, loc])
        # a third slot for the batches: the first picture again (a handle may repeat), so that six types fit sixteen pictures
        self.pics.append(self.pics[0])
        for loc in locs:
            self.up[count, loc], self.pics444[count, loc] = self.up[0, loc], self.pics444[0, loc]

    def close(self):
        self.ctx.close()
        self.ctx444.close()

    def both(self, loc, idx=None, **kw):
        """(the linear export of the 4:2:0 pictures, the existing export of the 4:4:4 pictures) with the same arguments"""
        idx = range(len(self.pics)) if idx is None else idx
        kw.setdefault("bit_depth", self.bd)
        got = self.ctx.export_batch([self.pics[i] for i in idx], "rgb", chroma="linear", chroma_loc=loc, **kw)
        want = self.ctx444.export_batch([self.pics444[i, loc] for i in idx], "rgb", **kw)
        _torch().cuda.synchronize()
        return got, want


@pytest.fixture(scope="module", params=[8, 10])
def pair(request):
    p = Pair(W, H, request.param, 2, LOCS, request.param)
    yield p
    p.close()


@pytest.fixture(scope="module")
def big():
    p = Pair(BW, BH, 10, 2, (1, 2), 7)
    p.pics.pop()                                             # two slots
    yield p
    p.close()


def form_kw(form):
    if form == "cl":
        return dict(memory_format=_torch().channels_last)
    return {} if form is None else dict(pixel=form, alpha=None if form in ("rgb", "bgr", "rgba", "bgra") else 5)


# ------------------------------------------------------------------------------------------------ yardstick 1: numpy
@pytest.mark.parametrize("loc", LOCS)
def test_against_numpy(pair, loc):
    """plain unsigned planes, matrix 1 and 9, limited and full range: the numpy upsample, then the published coef arithmetic"""
    for matrix in (1, 9):
        for full in (0, 1):
            desc = abi.make_export_desc(abi.EXPORT_RGB, pair.bd, 1 if pair.bd == 8 else 2, 0, (0, 0, 0, 0), matrix, full)
            coef = list(libhm_amd.export_plan(pair.seq, desc).coef)
            got = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, matrix=matrix, full_range=full, chroma="linear", chroma_loc=loc)
            got = got.cpu().numpy().astype(np.int64) & 0xffff
            for i in range(len(pair.pics)):
                want = ref.export_rgb(pair.up[i, loc], 3, (pair.bd, pair.bd), pair.bd, coef)
                assert np.array_equal(got[i], want), (loc, matrix, full, i)
    # the planted content does what it is there for: the six types give six different pictures, and none is the replicated one
    outs = [pair.ctx.export_batch(pair.pics[:1], "rgb", pair.bd, chroma="linear", chroma_loc=k) for k in LOCS]
    outs.append(pair.ctx.export_batch(pair.pics[:1], "rgb", pair.bd))
    assert all(not same(outs[a], outs[b]) for a in range(7) for b in range(a))


def test_single_picture_export(pair):
    one = pair.ctx.export(pair.pics[1], "rgb", pair.bd, chroma="linear", chroma_loc=3)
    assert same(one, pair.ctx444.export(pair.pics444[1, 3], "rgb", pair.bd))
    px = pair.ctx.export(pair.pics[1], "rgb", pair.bd, chroma="linear", chroma_loc=3, pixel="bgra", size=(30, 50))
    assert same(px, pair.ctx444.export(pair.pics444[1, 3], "rgb", pair.bd, pixel="bgra", size=(30, 50)))
    assert same(pair.ctx.export(pair.pics[1], "rgb", pair.bd, chroma="linear"), pair.ctx444.export(pair.pics444[1, 0], "rgb", pair.bd))


# ------------------------------------------------------------------------------------------------ yardstick 2: the 4:4:4 twin
@pytest.mark.parametrize("loc", [0, 3, 4])
def test_forms(pair, loc):
    """three planes, every packed order, channels-last; unsigned at the coding depth, and 2-byte msb-aligned at 10 bits"""
    for form in FORMS:
        got, want = pair.both(loc, **form_kw(form))
        assert same(got, want), (loc, form)
    if pair.bd == 10:
        for form in (None, "rgba"):
            got, want = pair.both(loc, msb_aligned=True, **form_kw(form))
            assert same(got, want), (loc, form, "msb")
    got, want = pair.both(loc, bit_depth=8, **form_kw("bgr"))               # another output depth than the coding depth
    assert same(got, want)


@pytest.mark.parametrize("loc", [1, 2])
def test_float_elements(pair, loc):
    torch = _torch()
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        for form in (None, "argb", "cl"):
            got, want = pair.both(loc, dtype=dtype, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD, **form_kw(form))
            assert got.dtype == dtype and same(got, want), (loc, dtype, form)
    # the scaled kernel: every element, planes and both pixel sizes, two pictures with the second mirrored, from a window whose
    # chroma offset is odd and whose width is no multiple of 4
    geo = dict(idx=[0, 1], windows=[(2, 6, 42, 26)] * 2, flip=[False, True], size=(20, 30))
    for dtype in (None, torch.float16, torch.bfloat16, torch.float32):
        kw = dict(geo) if dtype is None else dict(geo, dtype=dtype, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
        for form in (None, "bgr", "argb"):
            got, want = pair.both(loc, **kw, **form_kw(form))
            assert same(got, want), (loc, dtype, form, "scaled")


@pytest.mark.parametrize("shaper", [False, True])
def test_colour_lut_behind_the_chroma_stage(pair, shaper):
    rng = np.random.default_rng(11)
    depth = pair.bd
    lattice = rng.integers(0, 1 << depth, (17, 17, 17, 3)).astype(np.uint16)
    sh = rng.integers(0, 65536, (3, 1 << depth)).astype(np.uint16) if shaper else None
    with pair.ctx.colour_lut(lattice, sh, depth) as a, pair.ctx444.colour_lut(lattice, sh, depth) as b:
        for loc, kw in ((2, {}), (5, form_kw("rgba")), (1, dict(size=(24, 40), filter="bicubic"))):
            got = pair.ctx.export_batch(pair.pics, "rgb", depth, chroma="linear", chroma_loc=loc, lut=a, **kw)
            want = pair.ctx444.export_batch([pair.pics444[i, loc] for i in range(3)], "rgb", depth, lut=b, **kw)
            plain = pair.ctx444.export_batch([pair.pics444[i, loc] for i in range(3)], "rgb", depth, **kw)
            assert same(got, want) and not same(got, plain), (loc, kw)
        # every element and form behind both stages, unscaled and scaled: two pictures, the second mirrored, from a window whose
        # chroma offset is odd and whose width is no multiple of 4
        torch = _torch()
        geo = dict(windows=[(2, 6, 42, 26)] * 2, flip=[False, True])
        for dtype in (None, torch.float16, torch.bfloat16, torch.float32):
            kw = dict(geo) if dtype is None else dict(geo, dtype=dtype, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            for form in (None, "bgr", "argb"):
                for size in (None, (20, 30)):
                    got = pair.ctx.export_batch(pair.pics[:2], "rgb", depth, chroma="linear", chroma_loc=3, lut=a, size=size, **kw, **form_kw(form))
                    want = pair.ctx444.export_batch([pair.pics444[i, 3] for i in range(2)], "rgb", depth, lut=b, size=size, **kw, **form_kw(form))
                    assert same(got, want), (dtype, form, size)


WINDOWS = [(2, 6, 44, 26), (6, 2, 44, 26), (28, 14, 44, 26)]      # left / top 2 and 6: odd chroma offsets, groups not 8-byte aligned


@pytest.mark.parametrize("loc", [1, 2, 5])
def test_windows_mirrors_and_strided_out(pair, loc):
    torch = _torch()
    for flips in ([False, False, False], [True, False, True]):
        for form in (None, "bgr", "abgr"):
            got, want = pair.both(loc, windows=WINDOWS, flip=flips, **form_kw(form))
            assert same(got, want), (loc, flips, form)
    # windows resized, each from its own source window
    got, want = pair.both(loc, windows=[(2, 6, 44, 26), (6, 2, 60, 30), (0, 0, 72, 40)], flip=[True, False, False], size=(24, 36))
    assert same(got, want)
    # out=: rows, planes and batch entries further apart than dense
    dt = torch.uint8 if pair.bd == 8 else torch.int16
    store = [torch.full((3, 4, 30, 50), 77, dtype=dt, device="cuda") for _ in range(2)]
    outs = [s[:, :3, 2:28, 3:47] for s in store]
    got = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, windows=WINDOWS, chroma="linear", chroma_loc=loc, out=outs[0])
    want = pair.ctx444.export_batch([pair.pics444[i, loc] for i in range(3)], "rgb", pair.bd, windows=WINDOWS, out=outs[1])
    torch.cuda.synchronize()
    assert torch.equal(store[0], store[1]) and (store[0][:, 3] == 77).all() and (store[0][:, :, :2] == 77).all()


def test_window_of_the_export_is_the_export_of_the_window(pair):
    """taps outside the window but inside the decoded plane count: the linear export of a window is the window of the whole export"""
    for loc in (0, 3, 4):
        full = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, chroma="linear", chroma_loc=loc)
        part = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, chroma="linear", chroma_loc=loc, windows=WINDOWS)
        for i, (x, y, w, h) in enumerate(WINDOWS):
            assert same(part[i], full[i, :, y:y + h, x:x + w]), (loc, i)
        crop = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, chroma="linear", chroma_loc=loc, crop=(6, 2, 2, 4), pixel="rgb")
        whole = pair.ctx.export_batch(pair.pics, "rgb", pair.bd, chroma="linear", chroma_loc=loc, pixel="rgb")
        assert same(crop, whole[:, 2:H - 4, 6:W - 2])


@pytest.mark.parametrize("on_stream", [True, False])
def test_stream_modes(pair, on_stream):
    torch = _torch()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, want = pair.both(2, on_stream=on_stream, **form_kw("rgb"))
        got2, want2 = pair.both(2, on_stream=on_stream, size=(20, 36))
    if not on_stream:
        pair.ctx.sync()
        pair.ctx444.sync()
    torch.cuda.synchronize()
    assert same(got, want) and same(got2, want2)


def test_unaligned_destinations_keep_their_canaries(pair):
    """destinations at odd byte offsets (no vector stores) inside canaries, planes and packed pixels"""
    torch = _torch()
    es = 1 if pair.bd == 8 else 2
    dt = torch.uint8 if pair.bd == 8 else torch.int16
    for form, shape in ((None, (3, 3, H, W)), ("rgb", (3, H, W, 3)), ("rgba", (3, H, W, 4))):
        n = int(np.prod(shape))
        for off in (es, 3 * es):
            bufs = []
            for ctx, pics in ((pair.ctx, dict(chroma="linear", chroma_loc=3)), (pair.ctx444, {})):
                buf = torch.full((n * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
                out = buf[off:off + n * es].view(dt).view(shape)
                handles = pair.pics if pics else [pair.pics444[i, 3] for i in range(3)]
                ctx.export_batch(handles, "rgb", pair.bd, out=out, **pics, **form_kw(form))
                bufs.append(buf)
            torch.cuda.synchronize()
            assert torch.equal(bufs[0], bufs[1]), (form, off)
            assert (bufs[0][:off] == CANARY).all() and (bufs[0][off + n * es:] == CANARY).all()


# ------------------------------------------------------------------------------------------------ the scaled kernel
def tiles_of(out_w, out_h, n, taps_x, taps_y, x0=0):
    """the tiling the host chooses for an RGB scaled export (scale_tile_start and scale_tiles of hmgpu_export.hip, restated):
    (tiles_x, tiles_y, the most LDS passes a tile makes)"""
    tw = 128
    while tw > 4 and tw // 2 >= out_w:
        tw //= 2
    th = 1024 // tw
    while th > 1 and th // 2 >= out_h:
        th //= 2
    blocks = lambda: -(-out_w // tw) * -(-out_h // th)
    while blocks() * n < 1024 and tw * th > 64:
        if th >= tw // 4 and th > 2:
            th //= 2
        elif tw > 16:
            tw //= 2
        else:
            break
    fx, cx = taps_x
    fy, cy = taps_y
    while True:
        cap = 0
        for i0 in range(0, out_w, tw):
            lo, hi = min(fx[i0:i0 + tw]), max(f + c for f, c in zip(fx[i0:i0 + tw], cx[i0:i0 + tw]))
            cap = max(cap, ((x0 + hi + 7) & ~7) - ((x0 + lo) & ~7))
        cap = (cap + 7) & ~7
        rows = min(1024 // tw, 40960 // (3 * (2 * cap + 4 * tw)))
        if (rows >= 4 or tw <= 16) and rows >= 1:
            break
        tw //= 2
    passes = 0
    for i0 in range(0, out_h, th):
        lo, hi = min(fy[i0:i0 + th]), max(f + c for f, c in zip(fy[i0:i0 + th], cy[i0:i0 + th]))
        passes = max(passes, -(-(hi - lo) // rows))
    return -(-out_w // tw), -(-out_h // th), passes


SIZES = [(8, 64), (152, 200), (300, 400)]                  # (height, width): 25x / 4x down, 1.3x down, 1.5x up
FILTERS = {"nearest": abi.SCALE_NEAREST, "bilinear": abi.SCALE_BILINEAR, "bicubic": abi.SCALE_BICUBIC, "area": abi.SCALE_AREA}


def test_scaled_grid_has_several_tiles_and_passes(big):
    """what the scaled cases below rest on: every one runs several tiles in both directions, and the strong reductions walk their
    source rows in more than one pass through LDS"""
    desc = abi.make_export_desc(abi.EXPORT_RGB, 10, 2)
    for (h, w) in SIZES:
        for name, filt in FILTERS.items():
            sc = abi.make_export_scale(w, h, filt)
            tx, ty = (libhm_amd.export_scale_taps(big.seq, desc, sc, 0, ax) for ax in (0, 1))
            t = tiles_of(w, h, 2, (list(tx[0]), list(tx[1])), (list(ty[0]), list(ty[1])))
            assert t[0] > 1 and t[1] > 1, (h, w, name, t)
            if (h, w) == SIZES[0] and name != "nearest":
                assert t[2] > 1, (name, t)


@pytest.mark.parametrize("filt", sorted(FILTERS))
@pytest.mark.parametrize("size", SIZES)
def test_scaled(big, filt, size):
    torch = _torch()
    for loc in (1, 2):
        got, want = big.both(loc, size=size, filter=filt)
        assert same(got, want), (loc, size, filt)
    got, want = big.both(2, size=size, filter=filt, dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD, **form_kw("bgra"))
    assert same(got, want)
    wins = [(2, 6, 200, 150), (6, 2, 258, 198)]
    got, want = big.both(1, size=size, filter=filt, windows=wins, flip=[True, False], bit_depth=8)
    assert same(got, want)
    got, want = big.both(1, size=size, filter=filt, crop=(6, 2, 2, 4))       # one crop for all: the table slot of the shape
    assert same(got, want)


# ------------------------------------------------------------------------------------------------ the other chroma formats
def context_of(fmt, bd, planes):
    seq = abi.make_seq(W, H, bd, bd, max_pictures=8)
    seq.chroma_format = fmt
    ctx = libhm_amd.Context(seq)
    pic = ctx.acquire()
    ctx.upload(pic, planes)
    return seq, ctx, pic


def test_422_only_the_horizontal_rule_acts():
    rng = np.random.default_rng(3)
    m = 1023
    p = [rng.integers(0, m + 1, (H, W)).astype(np.int16)] + [rng.integers(0, m + 1, (H, W // 2)).astype(np.int16) for _ in range(2)]
    for c in p[1:]:
        c[:, 0], c[:, 1], c[:, -1], c[:, -2] = 0, m, m, 0
        c[::2, 8:24:2], c[1::2, 9:24:2] = m, 0
    seq, ctx, pic = context_of(2, 10, p)
    up = chref.upsample_planes(p, 2, 0)
    assert np.array_equal(up[1][:, 0::2], p[1]) and not np.array_equal(up[1][:, 1::2], p[1])
    seq444, ctx444, pic444 = context_of(3, 10, up)
    try:
        desc = abi.make_export_desc(abi.EXPORT_RGB, 10, 2, 0, (0, 0, 0, 0), 1, 0)
        want = ref.export_rgb(up, 3, (10, 10), 10, list(libhm_amd.export_plan(seq, desc).coef))
        outs = [ctx.export_batch([pic], "rgb", 10, chroma="linear", chroma_loc=loc) for loc in LOCS]
        assert np.array_equal(outs[0][0].cpu().numpy().astype(np.int64), want)
        assert all(same(o, outs[0]) for o in outs)                           # loc has no effect
        assert not same(outs[0], ctx.export_batch([pic], "rgb", 10))
        for kw in (form_kw("bgra"), dict(size=(30, 50), filter="bicubic"), dict(windows=[(6, 3, 40, 21)], flip=[True])):
            got = ctx.export_batch([pic], "rgb", 10, chroma="linear", chroma_loc=4, **kw)
            assert same(got, ctx444.export_batch([pic444], "rgb", 10, **kw)), kw
    finally:
        ctx.close()
        ctx444.close()


@pytest.mark.parametrize("fmt", [0, 3])
def test_444_and_400_are_untouched(fmt):
    rng = np.random.default_rng(fmt)
    sx, sy = ref.chroma_shift(fmt)
    p = [rng.integers(0, 256, (H, W)).astype(np.int16)] + [rng.integers(0, 256, (H >> sy, W >> sx)).astype(np.int16) for _ in range(2)]
    seq, ctx, pic = context_of(fmt, 8, p)
    try:
        for loc in (0, 5):
            for kw in ({}, form_kw("argb"), dict(size=(30, 50)), dict(windows=[(6, 2, 40, 20)], flip=[True], dtype=_torch().float32)):
                got = ctx.export_batch([pic], "rgb", 8, chroma="linear", chroma_loc=loc, **kw)
                assert same(got, ctx.export_batch([pic], "rgb", 8, **kw)), (fmt, loc, kw)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ the entry itself
def planar_destination(n, h, w, es=1):
    torch = _torch()
    buf = torch.full((n * 3 * h * w * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 32
    return buf, [base + k * h * w * es for k in range(3)], [w * es] * 3, [3 * h * w * es] * 3


def test_replicate_through_the_new_entry_is_the_existing_call(pair):
    """HMGPU_CHROMA_REPLICATE: bit for bit what the matching existing call writes, for planes, windows, scaling and packed pixels"""
    torch = _torch()
    es = 1 if pair.bd == 8 else 2
    rep = abi.make_export_chroma(abi.CHROMA_REPLICATE, 4)
    desc = abi.make_export_desc(abi.EXPORT_RGB, pair.bd, es, 0, (0, 0, 0, 0), 9, 1)
    win = [abi.make_export_window((2, W - 46, 6, H - 32)), abi.make_export_window((6, W - 50, 2, H - 28), True),
           abi.make_export_window((0, W - 44, 0, H - 26))]
    sc = abi.make_export_scale(40, 24, abi.SCALE_BICUBIC)
    px = abi.make_export_pixel(abi.PIXEL_BGRA, 7)
    for windows, scale, h, w in ((None, None, H, W), (win, None, 26, 44), (win, sc, 24, 40), (None, sc, 24, 40)):
        a, ptrs, pitches, bs = planar_destination(3, h, w, es)
        pair.ctx.export_chroma_into(pair.pics, desc, rep, ptrs, pitches, bs, scale=scale, windows=windows)
        b, ptrs, pitches, bs = planar_destination(3, h, w, es)
        pair.ctx.export_batch_into(pair.pics, desc, ptrs, pitches, bs, scale=scale, windows=windows)
        pair.ctx.sync()
        assert torch.equal(a, b) and not (a[32:-32] == CANARY).all(), (windows is not None, scale is not None)
        a = torch.full((3 * h * w * 4 * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
        b = a.clone()
        pair.ctx.export_chroma_into(pair.pics, desc, rep, [a.data_ptr() + 32], [w * 4 * es], [h * w * 4 * es], scale=scale, windows=windows, pixel=px)
        pair.ctx.export_pixels_into(pair.pics, desc, px, b.data_ptr() + 32, w * 4 * es, h * w * 4 * es, scale=scale, windows=windows)
        pair.ctx.sync()
        assert torch.equal(a, b) and not (a[32:-32] == CANARY).all()


def test_refused_calls_leave_the_destination_untouched(pair):
    es = 1 if pair.bd == 8 else 2
    lin = abi.make_export_chroma(abi.CHROMA_LINEAR, 2)
    good = abi.make_export_desc(abi.EXPORT_RGB, pair.bd, es)
    yuv = abi.make_export_desc(abi.EXPORT_PLANAR, pair.bd, es)
    reserved = abi.make_export_chroma(abi.CHROMA_LINEAR, 2)
    reserved.reserved[5] = 1
    buf, ptrs, pitches, bs = planar_destination(3, H, W, es)
    cases = [(yuv, lin, {}, abi.HMGPU_EINVAL), (good, None, {}, abi.HMGPU_EINVAL), (good, reserved, {}, abi.HMGPU_EINVAL),
             (good, abi.make_export_chroma(abi.CHROMA_LINEAR, 6), {}, abi.HMGPU_EINVAL),
             (good, abi.make_export_chroma(abi.CHROMA_LINEAR, -1), {}, abi.HMGPU_EINVAL),
             (good, abi.make_export_chroma(2, 0), {}, abi.HMGPU_EUNSUPPORTED),
             # the matching call's refusals come first: an unknown matrix (EUNSUPPORTED) before a NULL descriptor (EINVAL),
             # a bad LUT handle (the colour call's rule) before an unknown filter
             (abi.make_export_desc(abi.EXPORT_RGB, pair.bd, es, matrix=7), None, {}, abi.HMGPU_EUNSUPPORTED),
             (good, abi.make_export_chroma(2, 0), dict(lut=12345), abi.HMGPU_EINVAL),
             (good, lin, dict(scale=abi.make_export_scale(1, 1, abi.SCALE_AREA)), abi.HMGPU_EUNSUPPORTED)]
    for desc, chroma, kw, status in cases:
        with pytest.raises(libhm_amd.HmgpuError) as e:
            pair.ctx.export_chroma_into(pair.pics, desc, chroma, ptrs, pitches, bs, **kw)
        assert e.value.status == status, (status, e.value.status)
        assert pair.ctx.export_chroma_destination_status(3, desc, chroma, ptrs, pitches, bs, **kw) == status
    # a batch stride one byte short of a plane, a handle that is no picture
    short = list(bs)
    short[2] = H * W * es - 1
    with pytest.raises(libhm_amd.HmgpuError) as e:
        pair.ctx.export_chroma_into(pair.pics, good, lin, ptrs, pitches, short)
    assert e.value.status == abi.HMGPU_EINVAL
    with pytest.raises(libhm_amd.HmgpuError) as e:
        pair.ctx.export_chroma_into(pair.pics[:2] + [99], good, lin, ptrs, pitches, bs)
    assert e.value.status == abi.HMGPU_EINVAL
    pair.ctx.sync()
    assert (buf == CANARY).all()
    assert pair.ctx.export_chroma_destination_status(3, good, lin, ptrs, pitches, bs) == abi.HMGPU_OK
    with pytest.raises(ValueError):
        pair.ctx.export_batch(pair.pics, "rgb", pair.bd, chroma="nearest")
    with pytest.raises(libhm_amd.HmgpuError):
        pair.ctx.export_batch(pair.pics, "planar", pair.bd, chroma="linear")
