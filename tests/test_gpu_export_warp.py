"""The affine warp export on the GPU: hmgpu_pictures_export_warp behind warp= of Context.export_batch and Context.export.  Every
result is integer arithmetic that include/hmgpu.h states in full, so every comparison but one is an equality of bit patterns.  Two
yardsticks:
  1. tests/export_warp_ref.py (numpy, int64) applied to S, the existing unscaled export of the same window (which the existing tests
     hold against numpy), or to S from tests/export_ref.py directly;
  2. the existing export itself: maps that are the identity, an orientation or a whole-sample shift must reproduce it, a slice of it,
     torch.rot90 / flip of it or a clamped take of it, in every form the export has.
The one exception is the sanity test of the helper's convention against torch's grid_sample, whose bound is computed from S."""
import math

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_batch_ref as bref
from tests import export_ref as ref
from tests import export_warp_ref as wref
from tests import synth

pytestmark = pytest.mark.gpu

W, H = 72, 40
OUTS = [(37, 61), (1, 1), (8, 224)]     # (height, width): odd (partial tiles, packed tails off dword alignment), one pixel, four tiles wide
CANARY = 0xA5
Q = 65536
ID = wref.IDENTITY
FORMS = [None, "rgb", "bgr", "rgba", "bgra", "argb", "abgr", "cl"]
# whole chroma samples of 4:2:0; left / top 2 and 6: odd chroma offsets
WINDOWS = [(0, 0, 72, 40), (2, 6, 44, 26), (6, 2, 60, 30), (28, 14, 44, 26), (10, 4, 20, 12)]
FILTERS, BORDERS = ("bilinear", "nearest"), ("edge", "fill")


def _torch():
    import torch
    return torch


def raw(t):
    """a tensor's bytes in logical order (a copy with standard strides: contiguous() keeps the strides of dimensions of size 1)"""
    torch = _torch()
    return torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t).view(torch.uint8)


def same(a, b):
    torch = _torch()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def bits(t):
    """a 2-byte unsigned export as int16 holding the same bits: flip, rot90 and comparisons exist for it in every torch"""
    torch = _torch()
    u16 = getattr(torch, "uint16", None)
    return t.view(torch.int16) if u16 is not None and t.dtype == u16 else t


def form_kw(form):
    if form == "cl":
        return dict(memory_format=_torch().channels_last)
    return {} if form is None else dict(pixel=form, alpha=None if form in ("rgb", "bgr", "rgba", "bgra") else 5)


def packed(form):
    return form not in (None, "cl")


def ints(t):
    """an unsigned export as int64 numpy"""
    return t.cpu().numpy().astype(np.int64) & 0xffff


class Box:
    """a context of one format and depth with a few uploaded pictures, and the S of (picture, window, chroma) computed once"""

    def __init__(self, fmt, bd, count, seed, matrix=1):
        self.fmt, self.bd, self.matrix = fmt, bd, matrix
        self.seq = abi.make_seq(W, H, bd, bd, max_pictures=8)
        self.seq.chroma_format = fmt
        sx, sy = ref.chroma_shift(fmt)
        rng = np.random.default_rng(seed)
        m = (1 << bd) - 1
        self.planes = [[rng.integers(0, m + 1, (H, W)).astype(np.int16)] + [rng.integers(0, m + 1, (H >> sy, W >> sx)).astype(np.int16) for _ in range(2)]
                       for _ in range(count)]
        self.ctx = libhm_amd.Context(self.seq)
        self.pics = []
        for p in self.planes:
            self.pics.append(self.ctx.acquire())
            self.ctx.upload(self.pics[-1], p)
        self.cache = {}

    def close(self):
        self.ctx.close()

    def existing(self, idx, **kw):
        kw.setdefault("bit_depth", self.bd)
        kw.setdefault("matrix", self.matrix)
        return self.ctx.export_batch([self.pics[i] for i in idx], "rgb", **kw)

    def warp(self, idx, maps, size, **kw):
        kw.setdefault("bit_depth", self.bd)
        kw.setdefault("matrix", self.matrix)
        return self.ctx.export_batch([self.pics[i] for i in idx], "rgb", warp=maps, size=size, **kw)

    def S(self, i, window=None, chroma="replicate", loc=0):
        key = (i, window, chroma, loc)
        if key not in self.cache:
            self.cache[key] = ints(self.existing([i], windows=None if window is None else [window], chroma=chroma, chroma_loc=loc)[0])
        return self.cache[key]


@pytest.fixture(scope="module", params=[8, 10])
def box(request):
    b = Box(1, request.param, 3, request.param)
    yield b
    b.close()


def random_map(rng, size, window):
    """rotation within 45 degrees, zoom 0.5 .. 2, shear, a sub-sample translation, onto a window (x, y, w, h)"""
    return export.affine_map(size, (window[3], window[2]), angle=rng.uniform(-45, 45), scale=rng.uniform(0.5, 2.0),
                             shear=(rng.uniform(-15, 15), rng.uniform(-10, 10)), translate=(rng.uniform(-6, 6), rng.uniform(-4, 4)))


# ------------------------------------------------------------------------------------------------ identities: the existing export
def test_identity_map_is_the_existing_export_in_every_form(box):
    torch = _torch()
    idx = [0, 1, 2]
    variants = [dict(), dict(flip=[True, False, True]), dict(chroma="linear", chroma_loc=3), dict(bit_depth=8),
                dict(dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD),
                dict(dtype=torch.bfloat16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD),
                dict(dtype=torch.float32, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD), dict(matrix=9, full_range=1)]
    if box.bd == 10:
        variants.append(dict(msb_aligned=True))
    # the chroma stage under every float element
    variants += [dict(chroma="linear", chroma_loc=2, dtype=t, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
                 for t in (torch.float16, torch.bfloat16, torch.float32)]
    for v, kw in enumerate(variants):
        for f, form in enumerate(FORMS):
            filt = FILTERS[(v + f) & 1]
            got = box.warp(idx, [ID] * 3, (H, W), filter=filt, **kw, **form_kw(form))
            want = box.existing(idx, **kw, **form_kw(form))
            assert same(got, want), (kw.keys(), form, filt)
    # windows of one size, mirrored: the window is the source
    wins = [WINDOWS[1], WINDOWS[3], (6, 2, 44, 26)]
    for form in (None, "bgr", "abgr"):
        kw = dict(windows=wins, flip=[False, True, True], **form_kw(form))
        assert same(box.warp(idx, [ID] * 3, (26, 44), **kw), box.existing(idx, **kw)), form


def test_identity_behind_a_colour_lut(box):
    rng = np.random.default_rng(11)
    lattice = rng.integers(0, 1 << box.bd, (17, 17, 17, 3)).astype(np.uint16)
    with box.ctx.colour_lut(lattice, None, box.bd) as lut:
        for form in (None, "rgba", "cl"):
            got = box.warp([0, 1], [ID] * 2, (H, W), lut=lut, chroma="linear", chroma_loc=1, **form_kw(form))
            want = box.existing([0, 1], lut=lut, chroma="linear", chroma_loc=1, **form_kw(form))
            assert same(got, want) and not same(got, box.existing([0, 1], chroma="linear", chroma_loc=1, **form_kw(form))), form
        # every element and form, without and with the chroma stage: two pictures, the second mirrored, from a window whose chroma
        # offset is odd and whose width is no multiple of 4
        torch = _torch()
        geo = dict(windows=[(2, 6, 42, 26)] * 2, flip=[False, True])
        for d, dtype in enumerate((None, torch.float16, torch.bfloat16, torch.float32)):
            kw = dict(geo) if dtype is None else dict(geo, dtype=dtype, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            for f, form in enumerate((None, "bgr", "argb")):
                for c, chroma in enumerate((dict(), dict(chroma="linear", chroma_loc=4))):
                    got = box.warp([0, 1], [ID] * 2, (26, 42), filter=FILTERS[(d + f + c) & 1], lut=lut, **kw, **chroma, **form_kw(form))
                    assert same(got, box.existing([0, 1], lut=lut, **kw, **chroma, **form_kw(form))), (dtype, form, chroma)


@pytest.mark.parametrize("size", OUTS)
def test_identity_at_another_size_is_a_slice_or_an_edge_replication(box, size):
    """the output size belongs to the warp: smaller than the window it is the top-left part of the existing export, larger it
    repeats the last column (edge) or shows the fill -- partial tiles, packed tails, 1 x 1 and several tiles in a row"""
    h, w = size
    fill = (3, (1 << box.bd) - 1, 7)
    for form in FORMS:
        full = bits(box.existing([0, 1, 2], **form_kw(form)))
        for border in BORDERS:
            got = bits(box.warp([0, 1, 2], [ID] * 3, size, border=border, fill=fill, filter="nearest" if form == "bgr" else "bilinear", **form_kw(form)))
            hh, ww = min(h, H), min(w, W)
            if packed(form):
                assert same(got[:, :hh, :ww], full[:, :hh, :ww]), (form, border, size)
            else:
                assert same(got[:, :, :hh, :ww], full[:, :, :hh, :ww]), (form, border, size)
            if w > W and form is None:
                tail = got[:, :, :, W:]
                if border == "edge":
                    assert (tail == full[:, :, :hh, W - 1:W]).all()
                else:
                    assert all((tail[:, c] == fill[c]).all() for c in range(3))


def test_all_eight_orientations(box):
    torch = _torch()
    idx = [0, 1, 2, 0]
    planes, pixels = bits(box.existing(idx)), bits(box.existing(idx, pixel="rgba"))
    n = 0
    for k in range(4):
        for vflip in (False, True):
            for hflip in (False, True):
                m, size = export.orientation_map(k, vflip, hflip, (H, W))
                filt, border = FILTERS[n & 1], BORDERS[(n >> 1) & 1]
                n += 1
                dims = [d for d, on in ((2, vflip), (3, hflip)) if on]
                want = torch.rot90(torch.flip(planes, dims) if dims else planes, k, (2, 3))
                got = bits(box.warp(idx, [m] * 4, size, filter=filt, border=border, fill=(1, 2, 3)))
                assert same(got, want), (k, vflip, hflip, filt, border)
                dims = [d for d, on in ((1, vflip), (2, hflip)) if on]
                want = torch.rot90(torch.flip(pixels, dims) if dims else pixels, k, (1, 2))
                got = bits(box.warp(idx, [m] * 4, size, filter=filt, border=border, fill=(1, 2, 3), pixel="rgba"))
                assert same(got, want), (k, vflip, hflip, filt, border, "rgba")


def test_whole_sample_translations_under_both_borders(box):
    S = np.stack([box.S(i) for i in range(3)])
    fill = (5, (1 << box.bd) - 2, 0)
    y, x = np.mgrid[0:H, 0:W]
    shifts = [(3, -2), (-5, 7), (80, 0), (0, -50), (-72, 40)]
    for s, (dx, dy) in enumerate(shifts):
        m = (Q, 0, dx * Q, 0, Q, dy * Q)
        edge = S[:, :, np.clip(y + dy, 0, H - 1), np.clip(x + dx, 0, W - 1)]
        inside = (x + dx >= 0) & (x + dx < W) & (y + dy >= 0) & (y + dy < H)
        filled = np.where(inside[None, None], edge, np.array(fill).reshape(1, 3, 1, 1))
        for filt in FILTERS:
            assert np.array_equal(ints(box.warp([0, 1, 2], [m] * 3, (H, W), filter=filt)), edge), (dx, dy, filt)
            assert np.array_equal(ints(box.warp([0, 1, 2], [m] * 3, (H, W), filter=filt, border="fill", fill=fill)), filled), (dx, dy, filt)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("n", [1, 5, 16])
def test_random_maps_against_the_reference(box, n):
    """each slot its own picture (handles repeat), window, map and mirror; both filters, both borders, every output size"""
    rng = np.random.default_rng(100 + n)
    idx = [i % 3 for i in range(n)]
    wins = [WINDOWS[(i + n) % len(WINDOWS)] for i in range(n)]
    flips = [bool((i * 7 + n) & 2) for i in range(n)]
    fill = ((1 << box.bd) - 1, 0, 77)
    for size in OUTS:
        maps = [random_map(rng, size, wins[i]) for i in range(n)]
        for filt in FILTERS:
            for border in BORDERS:
                got = ints(box.warp(idx, maps, size, windows=wins, flip=flips, filter=filt, border=border, fill=fill))
                for i in range(n):
                    want = wref.warp(box.S(idx[i], wins[i]), maps[i], size, filt, border, fill)
                    assert np.array_equal(got[i], want[:, :, ::-1] if flips[i] else want), (size, filt, border, i)


def test_chroma_stage_under_a_warp_against_the_reference(box):
    """HMGPU_CHROMA_LINEAR: S is the linear export of the window, whose chroma taps may lie outside the window"""
    rng = np.random.default_rng(5)
    idx, wins = [0, 1, 2, 1], [WINDOWS[1], WINDOWS[2], WINDOWS[4], WINDOWS[0]]
    for loc in (0, 3, 4):
        maps = [random_map(rng, OUTS[0], w) for w in wins]
        for filt in FILTERS:
            got = ints(box.warp(idx, maps, OUTS[0], windows=wins, filter=filt, border="fill", fill=(9, 8, 7), chroma="linear", chroma_loc=loc))
            for i in range(4):
                want = wref.warp(box.S(idx[i], wins[i], "linear", loc), maps[i], OUTS[0], filt, "fill", (9, 8, 7))
                assert np.array_equal(got[i], want), (loc, filt, i)
    assert not np.array_equal(box.S(0, WINDOWS[1], "linear", 3), box.S(0, WINDOWS[1]))


def test_reference_on_numpy_s_and_packed_forms(box):
    """S from tests/export_ref.py alone; the packed forms and float elements of a warped picture are those of its planes"""
    torch = _torch()
    rng = np.random.default_rng(9)
    desc = abi.make_export_desc(abi.EXPORT_RGB, box.bd, 1 if box.bd == 8 else 2, 0, (0, 0, 0, 0), 1, 0)
    coef = list(libhm_amd.export_plan(box.seq, desc).coef)
    size = OUTS[0]
    maps = [random_map(rng, size, WINDOWS[0]) for _ in range(3)]
    want = np.stack([wref.warp(ref.export_rgb(box.planes[i], 1, (box.bd, box.bd), box.bd, coef), maps[i], size) for i in range(3)])
    planes = bits(box.warp([0, 1, 2], maps, size))
    assert np.array_equal(ints(planes), want)
    assert same(bits(box.warp([0, 1, 2], maps, size, pixel="rgb")), planes.permute(0, 2, 3, 1))
    assert same(bits(box.warp([0, 1, 2], maps, size, pixel="bgr")), planes.flip(1).permute(0, 2, 3, 1))
    assert same(bits(box.warp([0, 1, 2], maps, size, memory_format=torch.channels_last)), planes)
    argb = bits(box.warp([0, 1, 2], maps, size, pixel="argb", alpha=5))
    assert same(argb[..., 1:], planes.permute(0, 2, 3, 1)) and (argb[..., 0] == 5).all()
    f32 = box.warp([0, 1, 2], maps, size, dtype=torch.float32, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0))
    assert np.array_equal(f32.cpu().numpy().astype(np.int64), want)
    one = bits(box.ctx.export(box.pics[1], "rgb", box.bd, warp=maps[1], size=size))
    assert same(one, planes[1])
    assert same(bits(box.ctx.export(box.pics[1], "rgb", box.bd, warp=[maps[1]], size=size, pixel="rgb")), planes[1].permute(1, 2, 0))


def test_extreme_maps_are_defined(box):
    """legal inputs with defined results: targets far outside the window on every side, where only a 64-bit clamp is right"""
    big, small = (1 << 31) - 1, -(1 << 31)
    maps = [(big, 0, small, 0, Q, 0), (Q, 0, 0, big, 0, small), (small, small, small, small, small, small), (big,) * 6,
            (big, big, 0, Q, 0, 0), (Q, big, small, small, Q, big), (-Q, 0, big, 0, -Q, big), (1, 1, small, 1, 1, small),
            (big, 0, -7 * Q, 0, big, -3 * Q)]
    n = len(maps)
    idx = [i % 3 for i in range(n)]
    fill = (1, (1 << box.bd) - 1, 2)
    for size in (OUTS[0], OUTS[2]):
        for filt in FILTERS:
            for border in BORDERS:
                got = ints(box.warp(idx, maps, size, filter=filt, border=border, fill=fill))
                for i in range(n):
                    assert np.array_equal(got[i], wref.warp(box.S(idx[i]), maps[i], size, filt, border, fill)), (size, filt, border, i)


# ------------------------------------------------------------------------------------------------ the other chroma formats
@pytest.mark.parametrize("fmt,bd,matrix", [(2, 10, 1), (3, 8, 1), (3, 10, 0), (0, 8, 1)])
def test_other_chroma_formats(fmt, bd, matrix):
    b = Box(fmt, bd, 2, 40 + fmt, matrix)
    try:
        rng = np.random.default_rng(fmt)
        wins = [(0, 0, 72, 40), (6, 3, 40, 21) if fmt != 0 else (6, 2, 40, 22)]
        size = OUTS[0]
        maps = [random_map(rng, size, w) for w in wins]
        for chroma in ("replicate", "linear"):
            assert same(b.warp([0, 1], [ID] * 2, (H, W), chroma=chroma, pixel="bgra"), b.existing([0, 1], chroma=chroma, pixel="bgra"))
            for filt in FILTERS:
                got = ints(b.warp([0, 1], maps, size, windows=wins, filter=filt, border="fill", fill=(1, 2, 3), chroma=chroma))
                for i in range(2):
                    want = wref.warp(b.S(i, wins[i], chroma), maps[i], size, filt, "fill", (1, 2, 3))
                    assert np.array_equal(got[i], want), (fmt, chroma, filt, i)
        if fmt == 2:
            assert not np.array_equal(b.S(0, None, "linear"), b.S(0))
    finally:
        b.close()


# ------------------------------------------------------------------------------------------------ destinations
def test_unaligned_destinations_keep_their_canaries(box):
    """destinations at odd byte offsets (no vector stores) inside canaries, planes and packed pixels, at an odd output size"""
    torch = _torch()
    es = 1 if box.bd == 8 else 2
    dt = torch.uint8 if box.bd == 8 else torch.int16
    rng = np.random.default_rng(2)
    h, w = OUTS[0]
    maps = [random_map(rng, OUTS[0], WINDOWS[0]) for _ in range(3)]
    for form, shape in ((None, (3, 3, h, w)), ("rgb", (3, h, w, 3)), ("rgba", (3, h, w, 4))):
        want = box.warp([0, 1, 2], maps, OUTS[0], flip=[False, True, False], **form_kw(form))
        n = int(np.prod(shape))
        for off in (0, es, 3 * es):
            buf = torch.full((n * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
            out = buf[32 + off:32 + off + n * es].view(dt).view(shape)
            box.warp([0, 1, 2], maps, OUTS[0], flip=[False, True, False], out=out, **form_kw(form))
            torch.cuda.synchronize()
            assert torch.equal(raw(out), raw(want)), (form, off)
            assert (buf[:32 + off] == CANARY).all() and (buf[32 + off + n * es:] == CANARY).all(), (form, off)
    # out=: rows, planes and batch entries further apart than dense
    store = torch.full((3, 4, h + 6, w + 9), 77, dtype=dt, device="cuda")
    box.warp([0, 1, 2], maps, OUTS[0], flip=[False, True, False], out=store[:, :3, 2:2 + h, 3:3 + w])
    torch.cuda.synchronize()
    assert same(store[:, :3, 2:2 + h, 3:3 + w], bits(box.warp([0, 1, 2], maps, OUTS[0], flip=[False, True, False])))
    assert (store[:, 3] == 77).all() and (store[:, :, :2] == 77).all() and (store[:, :, :, :3] == 77).all() and (store[:, :, :, 3 + w:] == 77).all()


@pytest.mark.parametrize("on_stream", [True, False])
def test_stream_modes_and_many_calls_through_the_ring(box, on_stream):
    """more calls in a row than the window ring has buffers, each with other maps, on a side stream or the context's own"""
    torch = _torch()
    rng = np.random.default_rng(3)
    side = torch.cuda.Stream()
    calls = []
    with torch.cuda.stream(side):
        for _ in range(7):
            maps = [random_map(rng, OUTS[0], WINDOWS[0]) for _ in range(2)]
            calls.append((maps, box.warp([0, 2], maps, OUTS[0], on_stream=on_stream)))
    if not on_stream:
        box.ctx.sync()
    torch.cuda.synchronize()
    for maps, got in calls:
        for i, p in enumerate((0, 2)):
            assert np.array_equal(ints(got[i]), wref.warp(box.S(p), maps[i], OUTS[0]))


# ------------------------------------------------------------------------------------------------ the helper's convention against torch
def test_affine_map_follows_grid_sample():
    """rotation and zoom about the centre as torch sees them: grid_sample(bilinear, padding_mode="border", align_corners=False) of
    the float S with a theta built here from the forward transform, independently of export.affine_map.  The coordinate error per
    axis is at most 1/512 (the 8-bit fraction) + (W + H + 1) * 2^-17 (Q16 maps) < 0.006 samples for W, H <= 256, so the values
    differ by at most ceil(0.006 * (Gx + Gy) + 0.51), Gx and Gy the largest adjacent differences of S."""
    torch = _torch()
    import torch.nn.functional as F
    seq = abi.make_seq(W, H, 8, 8, max_pictures=2)
    ctx = libhm_amd.Context(seq)
    try:
        pic = ctx.acquire()
        ctx.upload(pic, synth.smooth_planes(W, H, 8, 3))
        S = ints(ctx.export_batch([pic], "rgb", 8)[0])
        gx, gy = int(np.abs(np.diff(S, axis=2)).max()), int(np.abs(np.diff(S, axis=1)).max())
        bound = math.ceil(0.006 * (gx + gy) + 0.51)
        for (oh, ow), angle, zoom in (((H, W), 20.0, 1.3), ((37, 61), -33.0, 0.8)):
            m = export.affine_map((oh, ow), (H, W), angle=angle, scale=zoom)
            got = ints(ctx.export_batch([pic], "rgb", 8, warp=[m], size=(oh, ow), border="edge")[0])
            # forward, positions with a sample's centre at index + 0.5 and y down: out - oc = zoom * R (src - sc), R counter-clockwise
            c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
            A = np.linalg.inv(zoom * np.array([[c, s], [-s, c]]))
            b = np.array([W / 2.0, H / 2.0]) - A @ np.array([ow / 2.0, oh / 2.0])
            # normalised coordinates: position = (n + 1) * size / 2
            No, Ns = np.diag([ow / 2.0, oh / 2.0]), np.diag([2.0 / W, 2.0 / H])
            theta = np.concatenate([Ns @ A @ No, (Ns @ (A @ No @ np.ones(2) + b) - 1.0)[:, None]], axis=1)
            grid = F.affine_grid(torch.tensor(theta[None], dtype=torch.float64), (1, 3, oh, ow), align_corners=False)
            want = F.grid_sample(torch.tensor(S[None], dtype=torch.float64), grid, mode="bilinear", padding_mode="border", align_corners=False)[0].numpy()
            diff = np.abs(got - want)
            print("affine_map vs grid_sample: angle %g zoom %g max |diff| %.3f bound %d (Gx %d Gy %d)" % (angle, zoom, diff.max(), bound, gx, gy))
            assert diff.max() <= bound, (angle, zoom, float(diff.max()), bound)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ refusals on a live context
def planar_destination(n, h, w, es=1):
    torch = _torch()
    buf = torch.full((n * 3 * h * w * es + 64,), CANARY, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr() + 32
    return buf, [base + k * h * w * es for k in range(3)], [w * es] * 3, [3 * h * w * es] * 3


def test_refused_calls_leave_the_destination_untouched(box):
    es = 1 if box.bd == 8 else 2
    h, w = OUTS[0]
    good = abi.make_export_desc(abi.EXPORT_RGB, box.bd, es)
    yuv = abi.make_export_desc(abi.EXPORT_PLANAR, box.bd, es)
    maps = abi.warp_map_array([ID] * 3)

    def wp(**kw):
        x = abi.make_export_warp(kw.pop("width", w), kw.pop("height", h), kw.pop("filter", 1), kw.pop("border", 0), kw.pop("fill", (0, 0, 0)))
        x.reserved[3] = kw.pop("reserved", 0)
        assert not kw
        return x
    bad_maps = abi.warp_map_array([ID] * 3)
    bad_maps[2].reserved[0] = 1
    buf, ptrs, pitches, bs = planar_destination(3, h, w, es)
    E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    cases = [(good, (None, maps), {}, E), (good, (wp(), None), {}, E), (good, (wp(reserved=1), maps), {}, E), (good, (wp(), bad_maps), {}, E),
             (good, (wp(width=0), maps), {}, E), (good, (wp(height=16385), maps), {}, E),
             (good, (wp(border=1, fill=(0, 1 << box.bd, 0)), maps), {}, E), (good, (wp(border=1, fill=(-1, 0, 0)), maps), {}, E),
             (yuv, (wp(), maps), {}, E), (good, (wp(filter=2), maps), {}, U), (good, (wp(border=2), maps), {}, U),
             # the matching call's refusals and those of the stages come first
             (abi.make_export_desc(abi.EXPORT_RGB, box.bd, es, matrix=7), (None, None), {}, U),
             (good, (wp(filter=2), maps), dict(lut=12345), E),
             (good, (wp(filter=2), maps), dict(chroma=abi.make_export_chroma(abi.CHROMA_LINEAR, 6)), E),
             (good, (wp(width=0), maps), dict(chroma=abi.make_export_chroma(2, 0)), U),
             (good, (wp(filter=2), maps), dict(windows=[abi.make_export_window((1, 0, 0, 0))] * 3), E),
             (good, (wp(filter=2), maps), dict(pixel=abi.make_export_pixel(9)), E)]
    pics = box.pics[:3]
    for desc, warp, kw, status in cases:
        with pytest.raises(libhm_amd.HmgpuError) as e:
            box.ctx.export_warp_into(pics, desc, warp, ptrs, pitches, bs, **kw)
        assert e.value.status == status, (status, e.value.status, kw.keys())
        assert box.ctx.export_warp_destination_status(3, desc, warp, ptrs, pitches, bs, **kw) == status
    ok = (wp(), maps)
    # a batch stride one byte short of a plane, a destination sized for a smaller output, a handle that is no picture
    short = list(bs)
    short[2] = h * w * es - 1
    with pytest.raises(libhm_amd.HmgpuError) as e:
        box.ctx.export_warp_into(pics, good, ok, ptrs, pitches, short)
    assert e.value.status == E
    assert box.ctx.export_warp_destination_status(3, good, (wp(width=w + 1), maps), ptrs, pitches, bs) == E
    with pytest.raises(libhm_amd.HmgpuError) as e:
        box.ctx.export_warp_into(pics[:2] + [99], good, ok, ptrs, pitches, bs)
    assert e.value.status == E
    box.ctx.sync()
    assert (buf == CANARY).all()
    # the next valid call works, and writes what the tensor call writes
    assert box.ctx.export_warp_destination_status(3, good, ok, ptrs, pitches, bs) == abi.HMGPU_OK
    box.ctx.export_warp_into(pics, good, ok, ptrs, pitches, bs)
    box.ctx.sync()
    want = box.warp([0, 1, 2], [ID] * 3, OUTS[0])
    assert _torch().equal(buf[32:32 + 9 * h * w * es], raw(want).reshape(-1)) and (buf[:32] == CANARY).all() and (buf[-32:] == CANARY).all()
    # the keywords
    for kw in (dict(filter="bicubic"), dict(border="reflect"), dict(size=None), dict(warp=[ID] * 2)):
        args = dict(warp=[ID] * 3, size=OUTS[0])
        args.update(kw)
        with pytest.raises(ValueError):
            box.ctx.export_batch(pics, "rgb", box.bd, **args)
    with pytest.raises(ValueError):
        box.ctx.export_batch(pics, "planar", box.bd, warp=[ID] * 3, size=OUTS[0])
    with pytest.raises(ValueError):
        box.ctx.export_batch(pics, "rgb", box.bd, border="fill")
