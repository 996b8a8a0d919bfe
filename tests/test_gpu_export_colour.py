"""The colour stage of the RGB exports on the GPU: hmgpu_pictures_export_colour behind lut= of Context.export_batch and
Context.export, in every form of the RGB export -- planes, packed pixels, channels-last, windows and mirrors, scaled, every element
kind.  The arithmetic is integer, so every comparison is an equality of bit patterns with tests/export_colour_ref.py.  Before each
comparison the integers that enter the LUT are checked, on the CPU, to exercise all six orderings of the fractions, a two-way and a
three-way tie, and the first and the last cell of every axis."""
import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_batch_ref as bref
from tests import export_colour_ref as cref
from tests import export_ref as ref
from tests import export_windows_ref as wref
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

W, H = 200, 72
CANARY = 0xA5
FILTER_NAMES = {abi.SCALE_NEAREST: "nearest", abi.SCALE_BILINEAR: "bilinear", abi.SCALE_BICUBIC: "bicubic", abi.SCALE_AREA: "area"}
# element kinds: (output depth = LUT depth, msb_aligned, sample type or None)
U8, U10, U10M, U12, U16, F16, BF16, F32 = (8, 0, None), (10, 0, None), (10, 1, None), (12, 0, None), (16, 0, None), \
    (8, 0, abi.SAMPLE_F16), (8, 0, abi.SAMPLE_BF16), (10, 0, abi.SAMPLE_F32)
KINDS = [U8, U10, U10M, F16, BF16, F32, U12, U16]
# forms: None three planes [N, 3, H, W]; "cl" the same, channels-last; else packed pixels [N, H, W, C]
FORMS = [None, "rgb", "bgr", "rgba", "bgra", "argb", "abgr", "cl"]
# LUTs: (nodes per axis or 0, with a shaper)
LUTS = [(2, False), (2, True), (17, False), (17, True), (33, False), (33, True), (65, False), (65, True), (0, True)]
ORIGINS = {96: [(0, 0), (2, 2), (4, 4), (6, 6), (W - 96, 10), (10, H - 40), (W - 96, H - 40)],
           94: [(0, 0), (2, 2), (4, 4), (6, 6), (W - 94, 10), (10, H - 40), (W - 94, H - 40)]}


def _torch():
    import torch
    return torch


def torch_dtype(st_type):
    torch = _torch()
    return {None: None, abi.SAMPLE_F16: torch.float16, abi.SAMPLE_BF16: torch.bfloat16, abi.SAMPLE_F32: torch.float32}[st_type]


def bits(t):
    """a tensor's elements as unsigned integers of their own width (bit patterns), in logical order, on the host"""
    torch = _torch()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    a = t.contiguous().view(view).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def canary(shape, dtype):
    torch = _torch()
    return torch.full(tuple(shape), CANARY, dtype=torch.uint8, device="cuda").view(dtype)


def random_planes(w, h, fmt, bd, seed):
    """random samples; at every origin of ORIGINS, one row down and eight columns in, eight planted luma samples over planted chroma:
    black, white and two greys (Cb = Cr = mid: R = G = B, a three-way tie, the first and the last cell), then four samples over
    Cb = mid + 1, Cr = mid (R and G mostly agree, B differs: a two-way tie)"""
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    p = [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
        [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]
    my, mc = (1 << bd[0]) - 1, 1 << (bd[1] - 1)
    for x0, y0 in set(ORIGINS[96] + ORIGINS[94]):
        x, y = x0 + 8, y0 + 1
        p[0][y, x:x + 8] = [0, my, my // 3, my // 2, my // 5, my // 4 + 1, my // 2 + 3, (3 * my) // 4]
        p[1][y >> sy, x >> sx:(x + 8) >> sx] = mc
        p[2][y >> sy, x >> sx:(x + 8) >> sx] = mc
        p[1][y >> sy, (x + 4) >> sx:(x + 8) >> sx] = mc + 1
    return p


def make_lut(depth, size, with_shaper, rgb, seed, mono=False):
    """(depth, lattice, shaper) with seeded random nodes and, with_shaper, a random shaper; rgb [3, N]: the integers about to enter
    it.  A random shaper scatters the positions, so a few of its entries are set from pixels of rgb whose values no other planted
    pixel shares: all three to 0 and to 65535 (the first and the last cell of every axis, three-way ties) and two equal with one
    apart (a two-way tie).  Then the coverage is asserted -- for a LUT without shaper it comes from the planted samples of
    random_planes; on 4:0:0 without a shaper R = G = B everywhere, and only the diagonal can be asked for."""
    rng = np.random.default_rng(seed)
    lattice = rng.integers(0, 1 << depth, (size, size, size, 3)).astype(np.uint16) if size else None
    shaper = None
    if with_shaper:
        shaper = rng.integers(0, 65536 if size else 1 << depth, (3, 1 << depth)).astype(np.uint16)
        if size:
            plans = [(0, 0, 0), (65535, 65535, 65535), (0x5123, 0x5123, 0x9321)]
            used = [set(), set(), set()]
            for px in rgb.T:
                if not plans:
                    break
                if any(int(px[c]) in used[c] for c in range(3)):
                    continue
                for c, u in enumerate(plans.pop(0)):
                    shaper[c][px[c]] = u
                    used[c].add(int(px[c]))
            assert not plans
    if size:
        cov = cref.coverage(rgb, depth, size, shaper)
        if mono and not with_shaper:
            assert cov["tie3"] and all(cov["cell0"]) and all(cov["cell_last"]), cov
        else:
            assert cref.covered(cov), (cov, depth, size, with_shaper)
    return depth, lattice, shaper


class Pictures:
    """a context with `count` uploaded pictures; the integers in front of the colour stage are computed once per (picture, window,
    export) and shared by every LUT, element kind and form"""

    def __init__(self, fmt, bd=(10, 10), count=4, seed=0):
        self.fmt, self.bd = fmt, bd
        self.seq = abi.make_seq(W, H, bd[0], bd[1], max_pictures=8)
        self.seq.chroma_format = fmt
        self.planes = {i: random_planes(W, H, fmt, bd, seed=1000 * seed + 10 * fmt + i) for i in range(count)}
        self.cache = {}
        self.open()

    def open(self):
        self.ctx = libhm_amd.Context(self.seq)
        self.pics = [self.ctx.acquire() for _ in self.planes]
        for i, p in enumerate(self.pics):
            self.ctx.upload(p, self.planes[i])
        self.index = {p: i for i, p in enumerate(self.pics)}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.__exit__(*a)

    def descs(self, kind, colour, size, filt, crop=(0, 0, 0, 0)):
        depth, msb, st_type = kind
        desc = abi.make_export_desc(ref.RGB, depth, 1 if depth <= 8 else 2, msb, crop, colour[0], colour[1])
        scale = None if size is None else sref.scale_of(size, filt)
        tensor = None if st_type is None else abi.make_export_tensor(st_type, *export.affine(depth, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
        return desc, scale, tensor

    def integers(self, pic, xywh, depth, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        key = (pic, tuple(xywh), depth, colour, size, filt)
        if key not in self.cache:
            desc, scale, _ = self.descs((depth, 0, None), colour, size, filt)
            self.cache[key] = cref.integers(self.seq, self.planes[self.index[pic]], self.fmt, self.bd, desc, scale, wref.window_of(self.seq, xywh))
        return self.cache[key]

    def entering(self, pics, windows, depth, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        """[3, N]: every integer triple the call sends into the colour stage"""
        return np.concatenate([self.integers(p, windows[i], depth, colour, size, filt).reshape(3, -1) for i, p in enumerate(pics)], axis=1)

    def want(self, pic, xywh, flip, kind, form, alpha, lut, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        desc, _, tensor = self.descs(kind, colour, size, filt)
        out = cref.lut_apply(self.integers(pic, xywh, kind[0], colour, size, filt), *lut)
        px = None
        if form not in (None, "cl"):
            code = export.PIXELS[form]
            px = abi.make_export_pixel(code) if alpha is None else abi.make_export_pixel(code, alpha, alpha) if tensor is not None \
                else abi.make_export_pixel(code, alpha)
        got = cref.finish(out, desc, tensor, wref.window_of(self.seq, xywh, flip), px)
        return got if px is not None else np.stack(got)

    def export(self, pics, windows, flips, kind, form, alpha, lut, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR, **kw):
        depth, msb, st_type = kind
        if st_type is not None:
            kw = dict(kw, dtype=torch_dtype(st_type), mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
        if form == "cl":
            kw = dict(kw, memory_format=_torch().channels_last)
        elif form is not None:
            kw = dict(kw, pixel=form, alpha=alpha)
        return self.ctx.export_batch(pics, "rgb", depth, matrix=colour[0], full_range=colour[1], msb_aligned=bool(msb), size=size,
                                     filter=FILTER_NAMES[filt], windows=windows, flip=flips, lut=lut, **kw)

    def compare(self, got, pics, windows, flips, kind, form, alpha, lut, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        g = bits(got)
        for i, p in enumerate(pics):
            want = self.want(p, windows[i], bool(flips[i]), kind, form, alpha, lut, colour, size, filt)
            where = (self.fmt, self.bd, kind, form, alpha, lut[0], None if lut[1] is None else lut[1].shape[0], lut[2] is not None, colour, size, filt,
                     i, windows[i], flips[i])
            assert g.shape == (len(pics),) + want.shape, where
            assert np.array_equal(g[i], want), where

    def run(self, pics, windows, flips, kind, form, alpha, size_shaper, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR, seed=0):
        """one LUT of size_shaper = (nodes per axis, with a shaper) built for what the call sends into it, one export, one comparison"""
        lut = make_lut(kind[0], size_shaper[0], size_shaper[1], self.entering(pics, windows, kind[0], colour, size, filt), seed,
                       mono=self.fmt == 0)
        with self.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
            got = self.export(pics, windows, flips, kind, form, alpha, h, colour, size, filt)
            self.compare(got, pics, windows, flips, kind, form, alpha, lut, colour, size, filt)
        return lut


def interior_alpha(kind, form):
    """None (opaque) for the orders with A last, an interior value for those with A first"""
    if form not in ("argb", "abgr"):
        return None
    return 0.3 if kind[2] is not None else 5


# ------------------------------------------------------------------------------------------------ 1. unscaled
@pytest.mark.parametrize("bd", [(8, 8), (10, 10), (12, 10)])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_unscaled(fmt, bd):
    """every LUT (2, 17, 33 and 65 nodes with and without a shaper, and a shaper alone) on windows of 96 and 94 columns at every
    left edge and at the right and bottom borders, alternating flips; n = 1, 3 and 16 with repeated handles; the element kinds and
    the forms rotate so that each occurs with each window width; BT.709 limited, BT.2020 full range, and the identity on 4:4:4"""
    n = (1, 3, 16)[(fmt + bd[0] // 2) % 3]
    with Pictures(fmt, bd, count=min(n, 4), seed=bd[0]) as P:
        pics = [P.pics[i % len(P.pics)] for i in range(n)]
        j = fmt
        for k, w in enumerate((96, 94)):
            windows = [ORIGINS[w][(i + 1) % 7] + (w, 40) for i in range(n)]
            flips = [(i + k) % 2 == 0 for i in range(n)]
            for lut in LUTS:
                kind, form = KINDS[j % len(KINDS)], FORMS[(j // 2 + k) % len(FORMS)]
                # (the identity only under a shaper: the planted greys are greys of a matrix, not of G = Y, B = Cb, R = Cr)
                colour = (9, 1) if j % 3 == 1 else (0, 0) if fmt == 3 and j % 3 == 2 and lut[1] else (1, 0)
                P.run(pics, windows, flips, kind, form, interior_alpha(kind, form), lut, colour, seed=j)
                j += 1


def test_every_kind_and_form():
    """the full product of element kinds and forms on one LUT of 17 nodes with a shaper, three pictures, 94 columns, mirrored;
    unscaled and scaled"""
    with Pictures(1, count=3) as P:
        windows = [ORIGINS[94][i] + (94, 40) for i in (1, 4, 6)]
        flips = [True, False, True]
        for kind in KINDS:
            lut = make_lut(kind[0], 17, True, P.entering(P.pics, windows, kind[0]), kind[0])
            with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
                for form in FORMS:
                    alpha = interior_alpha(kind, form)
                    P.compare(P.export(P.pics, windows, flips, kind, form, alpha, h), P.pics, windows, flips, kind, form, alpha, lut)
            # and through the scaled kernel: 30 x 20 outputs of the same windows
            size, filt = (20, 30), abi.SCALE_BILINEAR
            lut = make_lut(kind[0], 17, True, P.entering(P.pics, windows, kind[0], size=size, filt=filt), kind[0])
            with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
                for form in FORMS:
                    alpha = interior_alpha(kind, form)
                    got = P.export(P.pics, windows, flips, kind, form, alpha, h, size=size, filt=filt)
                    P.compare(got, P.pics, windows, flips, kind, form, alpha, lut, size=size, filt=filt)


def test_one_picture_and_the_crop_of_the_descriptor():
    """Context.export(lut=) without the batch dimension, planes and pixels, unscaled and scaled; export_batch without windows"""
    with Pictures(1, count=2) as P:
        pic = P.pics[0]
        for kind, form in ((U8, None), (F32, "bgra"), (U10M, "rgb")):
            xywh = (2, 2, 94, 40)
            lut = make_lut(kind[0], 33, False, P.entering([pic], [xywh], kind[0]), 3)
            kw = {} if kind[2] is None else dict(dtype=torch_dtype(kind[2]), mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            if form is not None:
                kw["pixel"] = form
            with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
                got = P.ctx.export(pic, "rgb", kind[0], crop=(2, W - 96, 2, H - 42), msb_aligned=bool(kind[1]), lut=h, **kw)
                assert np.array_equal(bits(got), P.want(pic, xywh, False, kind, form, None, lut))
                got = P.ctx.export_batch(P.pics, "rgb", kind[0], crop=(2, W - 96, 2, H - 42), msb_aligned=bool(kind[1]), lut=h, **kw)
                for i, p in enumerate(P.pics):
                    assert np.array_equal(bits(got[i]), P.want(p, xywh, False, kind, form, None, lut))
            full = (0, 0, W, H)
            lut = make_lut(kind[0], 17, True, P.entering([pic], [full], kind[0], size=(6, 7), filt=abi.SCALE_AREA), 4)
            with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
                got = P.ctx.export(pic, "rgb", kind[0], msb_aligned=bool(kind[1]), size=(6, 7), filter="area", lut=h, **kw)
                assert np.array_equal(bits(got), P.want(pic, full, False, kind, form, None, lut, size=(6, 7), filt=abi.SCALE_AREA))


# ------------------------------------------------------------------------------------------------ 2. scaled
MIXED = [(8, 8, 16, 16), (0, 0, 200, 72), (20, 0, 64, 72), (2, 2, 198, 70), (120, 10, 80, 40), (10, 42, 100, 30)]


@pytest.mark.parametrize("fmt", [1, 3])
@pytest.mark.parametrize("filt", [abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA])
def test_scaled(filt, fmt):
    """a reduction to 60 x 34 and to 7 x 6 and an enlargement to 150 x 100, from windows that all differ (the per-picture tables) and
    that are all equal (the cached slot); flips on the odd slots; planes, pixels and channels-last; LUTs with a shaper, whose
    entries carry the coverage (resampled noise reaches neither black nor white)"""
    with Pictures(fmt, count=4, seed=filt) as P:
        n = 6
        pics = [P.pics[i % 4] for i in range(n)]
        flips = [i % 2 == 1 for i in range(n)]
        jobs = (((34, 60), [MIXED[i % len(MIXED)] for i in range(n)]), ((34, 60), [(2, 2, 198, 70)] * n),
                ((6, 7), [(4 * (i % 3), 2 * i, 96, 40) for i in range(n)]), ((100, 150), [(8 * i, 2 * i, 64, 40) for i in range(n)]))
        j = filt + fmt
        for size, windows in jobs:
            for kind in (U8, F16, U10M):
                form = FORMS[j % len(FORMS)]
                lut = LUTS[1 + 2 * (j % 4)] if j % 5 else LUTS[8]
                P.run(pics, windows, flips, kind, form, interior_alpha(kind, form), lut, (9, 1) if j % 2 else (1, 0), size, filt, seed=j)
                j += 1


# ------------------------------------------------------------------------------------------------ 3. destinations, streams
def test_destinations_keep_their_canaries():
    """out= views into larger canary-filled tensors: planes with padded rows and an odd pitch, a base off by one element, packed
    pixels with a pitch that is no multiple of 4, a channels-last view; the samples are those of the dense call and every other
    byte keeps its canary"""
    torch = _torch()
    n, w, h = 3, 94, 40
    with Pictures(1, count=n) as P:
        pics = P.pics
        windows = [(2, 2, w, h), (4, 4, w, h), (W - w, H - h, w, h)]
        flips = [True, False, True]

        def check(big, view, dense):
            expect = canary(big.shape[:-1] + (big.shape[-1] * big.element_size(),), big.dtype)
            assert view(expect).shape == dense.shape
            view(expect).copy_(dense)
            assert torch.equal(big.view(torch.uint8), expect.view(torch.uint8))

        for kind in (U8, F16, U10M):
            lut = make_lut(kind[0], 17, False, P.entering(pics, windows, kind[0]), 11)
            dt = torch_dtype(kind[2]) or export.torch_dtype(1 if kind[0] <= 8 else 2)
            with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as hl:
                dense = P.export(pics, windows, flips, kind, None, None, hl)
                P.compare(dense, pics, windows, flips, kind, None, None, lut)
                es = dense.element_size()
                # planes: rows padded by 1 sample left and 2 right (u8: a pitch of 97 bytes), a spare row, every second entry
                big = canary((2 * n, 3, h + 1, (w + 3) * es), dt)
                view = lambda t: t[::2, :, :h, 1:w + 1]
                assert P.export(pics, windows, flips, kind, None, None, hl, out=view(big)).data_ptr() == view(big).data_ptr()
                check(big, view, dense)
                # the base off by one element
                flat = canary(((n * 3 * h * w + 8) * es,), dt)
                off = lambda t: torch.as_strided(t, (n, 3, h, w), (3 * h * w, h * w, w, 1), 1)
                P.export(pics, windows, flips, kind, None, None, hl, out=off(flat))
                check(flat, off, dense)
                # packed pixels: rows padded by one pixel left and two right (u8 x 3: a pitch of 291 bytes)
                packed = P.export(pics, windows, flips, kind, "bgr", None, hl)
                P.compare(packed, pics, windows, flips, kind, "bgr", None, lut)
                big = canary((n, h + 2, w + 3, 3 * es), dt)
                view = lambda t: t[:, 1:h + 1, 1:w + 1, :]
                P.export(pics, windows, flips, kind, "bgr", None, hl, out=view(big))
                check(big, view, packed)
                # a channels-last [N, 3, H, W] view
                big = canary((n, h + 1, w + 2, 3 * es), dt)
                view = lambda t: t[:, :h, 1:w + 1, :].permute(0, 3, 1, 2)
                P.export(pics, windows, flips, kind, "cl", None, hl, out=view(big))
                check(big, view, dense)


def test_streams():
    """on_stream: torch's current stream (a side stream, the result consumed on it without a host synchronisation), and the
    context's own stream with a context synchronisation"""
    torch = _torch()
    with Pictures(1, count=4) as P:
        pics = [P.pics[i % 4] for i in range(8)]
        windows = [(2 * i, 2 * (i % 3), 96, 40) for i in range(8)]
        flips = [False] * 8
        lut = make_lut(8, 33, True, P.entering(pics, windows, 8), 5)
        with P.ctx.colour_lut(lut[1], lut[2], lut[0]) as h:
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                got = P.export(pics, windows, flips, U8, "rgba", None, h)
                copy = got.clone()
            side.synchronize()
            P.compare(copy, pics, windows, flips, U8, "rgba", None, lut)
            got = P.export(pics, windows, flips, U8, None, None, h, on_stream=False)
            P.ctx.sync()
            P.compare(got, pics, windows, flips, U8, None, None, lut)


# ------------------------------------------------------------------------------------------------ 4. refusals, lifetime
def test_refusals_leave_the_destination_untouched():
    """a LUT of another depth, a layout that is not RGB, a destroyed handle, the handle of another context, no handle: HMGPU_EINVAL
    from the entry point and from the destination check, the canary intact; the ninth live LUT: HMGPU_ENOMEM, and the eight still
    work; then the call that is not refused writes"""
    torch = _torch()
    n, w, h = 3, 94, 40
    with Pictures(1, count=n) as P, Pictures(1, count=1, seed=1) as Q:
        pics = P.pics
        xywh = [(2 * i, 2 * i, w, h) for i in range(n)]
        wins = [wref.window_of(P.seq, xywh[i], i & 1) for i in range(n)]
        desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        rgb = P.entering(pics, xywh, 8)
        lut = make_lut(8, 17, False, rgb, 1)
        good = P.ctx.colour_lut(lut[1], lut[2], 8)
        deep = P.ctx.colour_lut(cref.identity_lattice(5, 10), None, 10)
        foreign = Q.ctx.colour_lut(lut[1], lut[2], 8)
        gone = P.ctx.colour_lut(lut[1], lut[2], 8)
        gone_handle = gone.handle
        gone.close()
        dst = canary((n, 3, h, w), torch.uint8)
        ptrs = [dst.data_ptr() + k * h * w for k in range(3)]
        pitches, bstrides = [w] * 3, [3 * h * w] * 3
        stream = torch.cuda.current_stream().cuda_stream

        def refused(handle, desc_=desc, pitches_=pitches):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                P.ctx.export_colour_into(pics, desc_, handle, ptrs, pitches_, bstrides, 1, stream, None, None, wins)
            assert e.value.status == abi.HMGPU_EINVAL
            assert P.ctx.export_colour_destination_status(n, desc_, handle, ptrs, pitches_, bstrides, None, None, wins) == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            P.ctx.sync()
            assert bool((dst == CANARY).all())

        refused(deep)                                                        # a LUT of depth 10 on an 8-bit export
        planar = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        cw = [dst.data_ptr(), dst.data_ptr() + h * w, dst.data_ptr() + h * w + (h // 2) * (w // 2)]
        with pytest.raises(libhm_amd.HmgpuError) as e:                       # a layout that is not RGB (its own planes fit the destination)
            P.ctx.export_colour_into(pics, planar, good, cw, [w, w // 2, w // 2], bstrides, 1, stream, None, None, wins)
        assert e.value.status == abi.HMGPU_EINVAL
        assert P.ctx.export_colour_destination_status(n, planar, good, cw, [w, w // 2, w // 2], bstrides, None, None, wins) == abi.HMGPU_EINVAL
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all())
        refused(gone_handle)
        refused(foreign)
        refused(0)
        refused(-1)
        with pytest.raises(libhm_amd.HmgpuError) as e:
            libhm_amd.ColourLut(P.ctx, gone_handle, abi.make_colour_lut_desc(8, 17, 0)).close()     # destroyed twice
        assert e.value.status == abi.HMGPU_EINVAL
        # the matching call's own refusals stay in front: a pitch one byte short of a row is refused whatever the LUT is
        refused(good, pitches_=[w, w, w - 1])
        # at most eight live LUTs per context
        more = [P.ctx.colour_lut(None, np.zeros((3, 256), np.uint16), 8) for _ in range(abi.COLOUR_MAX_LUTS - 2)]
        with pytest.raises(libhm_amd.HmgpuError) as e:
            P.ctx.colour_lut(None, np.zeros((3, 256), np.uint16), 8)
        assert e.value.status == abi.HMGPU_ENOMEM
        assert P.ctx.export_colour_destination_status(n, desc, good, ptrs, pitches, bstrides, None, None, wins) == abi.HMGPU_OK
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all())
        more.pop().close()
        ninth = P.ctx.colour_lut(lut[1], lut[2], 8)                          # a slot is free again
        for handle in (good, ninth):
            dst.view(torch.uint8).fill_(CANARY)
            P.ctx.export_colour_into(pics, desc, handle, ptrs, pitches, bstrides, 1, stream, None, None, wins)
            for i, p in enumerate(pics):
                assert np.array_equal(bits(dst[i]), P.want(p, xywh[i], bool(i & 1), U8, None, None, lut))
        foreign.close()


def test_lifetime():
    """a LUT destroyed right after an export that reads it was enqueued: the export completes with that LUT's values; a LUT created
    afterwards (which may take the same memory) serves the next export, and the first result stays what it was"""
    torch = _torch()
    with Pictures(1, count=4) as P:
        pics = [P.pics[i % 4] for i in range(16)]
        windows = [ORIGINS[96][i % 7] + (96, 40) for i in range(16)]
        flips = [i % 2 == 0 for i in range(16)]
        rgb = P.entering(pics, windows, 8)
        first, second = make_lut(8, 65, False, rgb, 21), make_lut(8, 65, False, rgb, 22)
        for size, windows_ in ((None, windows), ((34, 60), [(2, 2, 198, 70)] * 16)):
            a = P.ctx.colour_lut(first[1], first[2], 8)
            got_a = P.export(pics, windows_, flips, U8, "rgb", None, a, size=size)
            a.close()                                                        # (no synchronisation in between)
            b = P.ctx.colour_lut(second[1], second[2], 8)
            got_b = P.export(pics, windows_, flips, U8, "rgb", None, b, size=size)
            b.close()
            torch.cuda.synchronize()
            P.compare(got_a, pics, windows_, flips, U8, "rgb", None, first, size=size)
            P.compare(got_b, pics, windows_, flips, U8, "rgb", None, second, size=size)


def test_without_the_stage_nothing_changes():
    """the identity: a shaper-only LUT of v -> v through the colour call writes the bits of the call without lut="""
    torch = _torch()
    with Pictures(2, count=3) as P:
        windows = [ORIGINS[94][i] + (94, 40) for i in (0, 3, 5)]
        flips = [False, True, False]
        for kind in (U8, U10M, F16):
            ramp = np.tile(np.arange(1 << kind[0], dtype=np.uint16), (3, 1))
            with P.ctx.colour_lut(None, ramp, kind[0]) as h:
                for form in (None, "abgr"):
                    for size in (None, (30, 44)):
                        assert torch.equal(P.export(P.pics, windows, flips, kind, form, None, h, size=size),
                                           P.export(P.pics, windows, flips, kind, form, None, None, size=size))
