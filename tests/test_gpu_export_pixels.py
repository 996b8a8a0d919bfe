"""Packed pixel export on the GPU: hmgpu_pictures_export_pixels / hmdec_pictures_export_pixels behind pixel= / alpha= /
memory_format= of Context.export_batch, Context.export, hmdec.export_batch, Picture.export and Decoder.frames.  No arithmetic is new,
so every comparison is an equality of bit patterns with the numpy restatement (tests/export_pixels_ref.py: the planes of the existing
restatements stacked in channel order, A inserted) or, on the device, with the planar call permuted."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, hmdec
from tests import export_batch_ref as bref
from tests import export_pixels_ref as pref
from tests import export_ref as ref
from tests import export_windows_ref as wref
from tests import golden_util as gu
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

W, H = 200, 72
CANARY = 0xA5
ORDERS = ["rgb", "bgr", "rgba", "bgra", "argb", "abgr"]
FILTER_NAMES = {abi.SCALE_NEAREST: "nearest", abi.SCALE_BILINEAR: "bilinear", abi.SCALE_BICUBIC: "bicubic", abi.SCALE_AREA: "area"}
# element kinds: (output depth, msb_aligned, sample type or None, interior alpha)
U8, U10, F16, BF16, F32 = (8, 0, None, 100), (10, 1, None, 700), (8, 0, abi.SAMPLE_F16, 0.3), (8, 0, abi.SAMPLE_BF16, -2.75), (10, 0, abi.SAMPLE_F32, 0.3)


def _torch():
    import torch
    return torch


def torch_dtype(st_type):
    torch = _torch()
    return {None: None, abi.SAMPLE_F16: torch.float16, abi.SAMPLE_BF16: torch.bfloat16, abi.SAMPLE_F32: torch.float32}[st_type]


def random_planes(w, h, fmt, bd, seed):
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    return [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
           [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]


def bits(t):
    """a tensor's elements as unsigned integers of their own width (bit patterns), on the host"""
    torch = _torch()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    a = t.contiguous().view(view).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def canary(shape, dtype):
    torch = _torch()
    return torch.full(tuple(shape), CANARY, dtype=torch.uint8, device="cuda").view(dtype)


class Pictures:
    """a context with `count` uploaded random pictures; the planar reference of (picture, window, export) is computed once and packed
    per channel order"""

    def __init__(self, fmt, bd=(10, 10), count=4, seed=0):
        self.fmt, self.bd = fmt, bd
        self.seq = abi.make_seq(W, H, bd[0], bd[1], max_pictures=8)
        self.seq.chroma_format = fmt
        self.ctx = libhm_amd.Context(self.seq)
        self.pics = [self.ctx.acquire() for _ in range(count)]
        self.planes = {}
        for i, p in enumerate(self.pics):
            self.planes[p] = random_planes(W, H, fmt, bd, seed=1000 * seed + 10 * fmt + i)
            self.ctx.upload(p, self.planes[p])
        self.cache = {}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.__exit__(*a)

    def descs(self, kind, colour, size, filt):
        depth, msb, st_type, _ = kind
        desc = abi.make_export_desc(ref.RGB, depth, 1 if depth <= 8 else 2, msb, (0, 0, 0, 0), colour[0], colour[1])
        scale = None if size is None else sref.scale_of(size, filt)
        tensor = None if st_type is None else abi.make_export_tensor(st_type, *export.affine(depth, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
        return desc, scale, tensor

    def want(self, pic, xywh, flip, kind, order, alpha, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        """[H, W, C] of one slot: the unmirrored planes cached, the mirror and the packing per slot"""
        desc, scale, tensor = self.descs(kind, colour, size, filt)
        key = (pic, tuple(xywh), kind, colour, size, filt)
        if key not in self.cache:
            self.cache[key] = wref.export_slot_ref(self.seq, self.planes[pic], self.fmt, self.bd, desc, scale, tensor, wref.window_of(self.seq, xywh))
        planes = wref.mirror(self.cache[key], ref.RGB) if flip else self.cache[key]
        px = abi.make_export_pixel(export.PIXELS[order])
        if alpha is not None:
            px = abi.make_export_pixel(export.PIXELS[order], alpha, alpha) if tensor is not None else abi.make_export_pixel(export.PIXELS[order], alpha)
        return pref.pack(planes, desc, tensor, px, kind[0])

    def export(self, pics, windows, flips, kind, order, alpha, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR, **kw):
        depth, msb, st_type, _ = kind
        if st_type is not None:
            kw = dict(kw, dtype=torch_dtype(st_type), mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
        if order is not None:
            kw = dict(kw, pixel=order, alpha=alpha)
        return self.ctx.export_batch(pics, "rgb", depth, matrix=colour[0], full_range=colour[1], msb_aligned=bool(msb), size=size,
                                     filter=FILTER_NAMES[filt], windows=windows, flip=flips, **kw)

    def check(self, got, pics, windows, flips, kind, order, alpha, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        g = bits(got)
        for i, p in enumerate(pics):
            want = self.want(p, windows[i], bool(flips[i]), kind, order, alpha, colour, size, filt)
            where = (self.fmt, kind, order, alpha, colour, size, filt, i, windows[i], flips[i])
            assert g.shape == (len(pics),) + want.shape, where
            assert np.array_equal(g[i], want), where

    def run(self, pics, windows, flips, kind, order, alpha, colour=(1, 0), size=None, filt=abi.SCALE_BILINEAR):
        got = self.export(pics, windows, flips, kind, order, alpha, colour, size, filt)
        assert got.dtype == (torch_dtype(kind[2]) or export.torch_dtype(1 if kind[0] <= 8 else 2)) and got.is_contiguous()
        self.check(got, pics, windows, flips, kind, order, alpha, colour, size, filt)


# ------------------------------------------------------------------------------------------------ 1. unscaled
# 96 x 40 at left edges 0, 2, 4 and 6 and at the right and bottom borders; 94 x 40 (no multiple of 4: partial groups, and mirrored
# partial groups at the row's start) the same
ORIGINS = {96: [(0, 0), (2, 2), (4, 4), (6, 6), (W - 96, 10), (10, H - 40), (W - 96, H - 40)],
           94: [(0, 0), (2, 2), (4, 4), (6, 6), (W - 94, 10), (10, H - 40), (W - 94, H - 40)]}


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_unscaled(fmt, n):
    """every element kind x every channel order (alpha opaque and an interior value), windows of 96 and 94 columns at every left
    edge and at the borders, alternating flips; BT.709 limited, BT.2020 full range, and the identity on 4:4:4"""
    with Pictures(fmt, count=min(n, 4)) as P:
        pics = [P.pics[i % len(P.pics)] for i in range(n)]
        for k, w in enumerate((96, 94)):
            windows = [ORIGINS[w][(i + 1) % 7] + (w, 40) for i in range(n)]
            flips = [(i + k) % 2 == 0 for i in range(n)]
            for kind in (U8, U10, F16, BF16, F32):
                for j, order in enumerate(ORDERS):
                    P.run(pics, windows, flips, kind, order, None if (j + k) % 2 else kind[3])
            for kind, order in ((U8, "bgr"), (F16, "argb"), (U10, "rgba")):
                P.run(pics, windows, flips, kind, order, None, colour=(9, 1))
                if fmt == 3:
                    P.run(pics, windows, flips, kind, order, kind[3], colour=(0, 0))
        # windows None: the crop of the descriptor (hmgpu_pictures_export's planes)
        got = P.ctx.export_batch(pics, "rgb", 8, crop=(6, 100, 2, 30), pixel="abgr", alpha=7)
        for i, p in enumerate(pics):
            assert np.array_equal(bits(got[i]), P.want(p, (6, 2, 94, 40), False, U8, "abgr", 7))


def test_one_picture():
    """Context.export(pixel=): [H, W, C] without the batch dimension"""
    with Pictures(1, count=1) as P:
        for kind, order in ((U8, "bgra"), (F32, "rgb"), (U10, "abgr")):
            kw = {} if kind[2] is None else dict(dtype=torch_dtype(kind[2]), mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
            got = P.ctx.export(P.pics[0], "rgb", kind[0], crop=(2, W - 96, 2, H - 42), msb_aligned=bool(kind[1]), pixel=order, **kw)
            assert np.array_equal(bits(got), P.want(P.pics[0], (2, 2, 94, 40), False, kind, order, None))
            got = P.ctx.export(P.pics[0], "rgb", kind[0], msb_aligned=bool(kind[1]), size=(6, 7), filter="area", pixel=order, **kw)
            assert np.array_equal(bits(got), P.want(P.pics[0], (0, 0, W, H), False, kind, order, None, size=(6, 7), filt=abi.SCALE_AREA))


# ------------------------------------------------------------------------------------------------ 2. destinations
def test_destinations_keep_their_canaries():
    """out= views into larger canary-filled tensors -- padded rows, a base off by one pixel and by one element (no dword stores), a
    pitch that is no multiple of 4 with 3-byte pixels, clip[:, 1] of [N, 2, H, W, C], a channels-last [N, 3, H, W] tensor: the
    pixels are those of the dense call and every other byte keeps its canary"""
    torch = _torch()
    n, w, h = 3, 94, 40
    with Pictures(1, count=n) as P:
        pics = P.pics
        windows = [(2, 2, w, h), (4, 4, w, h), (W - w, H - h, w, h)]

        def check(big, view, dense):
            expect = canary(big.shape[:-1] + (big.shape[-1] * big.element_size(),), big.dtype)
            assert view(expect).shape == dense.shape
            view(expect).copy_(dense)
            assert torch.equal(big.view(torch.uint8), expect.view(torch.uint8))

        for flips in ([True, False, True], [False, True, False]):
            for kind, order, alpha in ((U8, "rgb", None), (U8, "bgra", 9), (F16, "bgr", None), (F16, "argb", 0.3), (U10, "rgba", None), (F32, "rgb", None)):
                c = len(order)
                dt = torch_dtype(kind[2]) or export.torch_dtype(1 if kind[0] <= 8 else 2)
                dense = P.export(pics, windows, flips, kind, order, alpha)
                P.check(dense, pics, windows, flips, kind, order, alpha)
                # rows padded by 1 pixel left and 2 right (u8 x 3: a pitch of 291 bytes), a spare row above and below, every second entry
                views = [lambda t: t[::2, 1:h + 1, 1:w + 1, :]]
                bigs = [canary((2 * n, h + 2, w + 3, c * dense.element_size()), dt)]
                # a pitch of 4-byte multiples, the base on a pixel boundary 4 pixels in: dword stores on aligned rows
                views.append(lambda t: t[:n, :h, 4:w + 4, :])
                bigs.append(canary((n + 1, h, w + 6, c * dense.element_size()), dt))
                # one frame of a clip
                views.append(lambda t: t[:, 1])
                bigs.append(canary((n, 2, h, w, c * dense.element_size()), dt))
                for view, big in zip(views, bigs):
                    r = P.export(pics, windows, flips, kind, order, alpha, out=view(big))
                    assert r.data_ptr() == view(big).data_ptr()
                    check(big, view, dense)
                # the base off by one element: every group element by element
                flat = canary(((n * h * w * c + 8) * dense.element_size(),), dt)
                off = lambda t: torch.as_strided(t, (n, h, w, c), (h * w * c, w * c, c, 1), 1)
                P.export(pics, windows, flips, kind, order, alpha, out=off(flat))
                check(flat, off, dense)
                if c == 3:                                                    # channels-last [N, 3, H, W] as out=
                    big = canary((n, h + 1, w + 2, 3 * dense.element_size()), dt)
                    view = lambda t: t[:, :h, 1:w + 1, :].permute(0, 3, 1, 2)
                    assert view(big).shape == (n, 3, h, w)
                    P.export(pics, windows, flips, kind, order, alpha, out=view(big))
                    check(big, view, dense.permute(0, 3, 1, 2))
        # what out= refuses: pixels that are not dense, a wrong shape, a wrong dtype
        for bad in (torch.empty((n, h, w, 6), dtype=torch.uint8, device="cuda")[..., ::2], torch.empty((n, h, 2 * w, 3), dtype=torch.uint8, device="cuda")[:, :, ::2],
                    torch.empty((n, h, w, 4), dtype=torch.uint8, device="cuda"), torch.empty((n, h, w, 3), dtype=torch.int16, device="cuda"),
                    torch.empty((n, 3, h, w), dtype=torch.uint8, device="cuda")):
            with pytest.raises(ValueError):
                P.export(pics, windows, [False] * n, U8, "rgb", None, out=bad)


def test_channels_last_and_repeated_handles():
    """memory_format=torch.channels_last: a [N, 3, H, W] tensor with channels-last strides holding the bytes of pixel="rgb", equal
    to the planar call; the same handle twice in one batch"""
    torch = _torch()
    with Pictures(1, count=2) as P:
        pics = [P.pics[0], P.pics[1], P.pics[0], P.pics[0]]
        windows = [(2, 2, 94, 40), (4, 4, 94, 40), (2, 2, 94, 40), (6, 6, 94, 40)]
        flips = [False, True, False, True]
        for kind in (U8, F16):
            for size in (None, (34, 60)):
                cl = P.export(pics, windows, flips, kind, None, None, size=size, memory_format=torch.channels_last)
                hh, ww = size or (40, 94)
                assert cl.shape == (4, 3, hh, ww) and cl.is_contiguous(memory_format=torch.channels_last) and not cl.is_contiguous()
                planar = P.export(pics, windows, flips, kind, None, None, size=size)
                assert planar.is_contiguous() and torch.equal(cl, planar)
                packed = P.export(pics, windows, flips, kind, "rgb", None, size=size)
                assert torch.equal(cl.permute(0, 2, 3, 1), packed)
                P.check(packed, pics, windows, flips, kind, "rgb", None, size=size)
                assert torch.equal(packed[0], packed[2])
        with pytest.raises(ValueError):
            P.export(pics, windows, flips, U8, "rgb", None, memory_format=torch.channels_last)
        with pytest.raises(ValueError):
            P.ctx.export_batch(pics, "planar", 8, memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------ 3. scaled
MIXED = [(8, 8, 16, 16), (0, 0, 200, 72), (20, 0, 64, 72), (2, 2, 198, 70), (120, 10, 80, 40), (10, 42, 100, 30)]
LARGE = [(0, 0, 200, 72), (20, 0, 64, 72), (2, 2, 198, 70), (120, 10, 80, 40), (10, 42, 100, 30)]       # (224 outputs: within 8x)


@pytest.mark.parametrize("fmt", [1, 3])
@pytest.mark.parametrize("filt", [abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA])
def test_scaled(filt, fmt):
    """60 x 34 outputs from windows that all differ (the per-picture tables) and that are all equal (the cached slot), 224 x 224, and
    7 x 6 from a 96 x 40 window (one full and one partial group per row); flips on the odd slots, u8 and float16, 3 and 4 channels"""
    with Pictures(fmt, count=4) as P:
        n = 8
        pics = [P.pics[i % 4] for i in range(n)]
        flips = [i % 2 == 1 for i in range(n)]
        jobs = (((34, 60), [MIXED[i % len(MIXED)] for i in range(n)]), ((34, 60), [(2, 2, 198, 70)] * n),
                ((6, 7), [(4 * (i % 3), 2 * i, 96, 40) for i in range(n)]), ((6, 7), [(6, 2, 96, 40)] * n))
        for j, (size, windows) in enumerate(jobs):
            for kind, order, alpha in ((U8, "rgb", None), (U8, "bgra", 100), (F16, "bgr", None), (F16, "abgr", 0.3)):
                P.run(pics, windows, flips, kind, order, alpha, size=size, filt=filt)
            P.run(pics, windows, flips, U10, ORDERS[(j + filt) % 6], None, colour=(9, 1), size=size, filt=filt)
        if filt == abi.SCALE_BILINEAR:                       # bfloat16 packed pixels of the scaled kernel, 3 and 4 channels
            P.run(pics, windows, flips, BF16, "rgb", None, size=size, filt=filt)
            P.run(pics, windows, flips, BF16, "argb", BF16[3], size=size, filt=filt)
        windows = LARGE[:4]
        P.run(pics[:4], windows, flips[:4], U8, "rgb", None, size=(224, 224), filt=filt)
        P.run(pics[:4], windows, flips[:4], F16, "rgba", None, size=(224, 224), filt=filt)


# ------------------------------------------------------------------------------------------------ 4. the existing path on the device
def test_equals_the_planar_call_permuted():
    """export_batch(pixel="rgb") equals export_batch(...).permute(0, 2, 3, 1), unscaled and bilinear; and two packed calls back to
    back without synchronisation into two tensors"""
    torch = _torch()
    with Pictures(1, count=4) as P:
        pics = [P.pics[i % 4] for i in range(16)]
        gen = torch.Generator().manual_seed(3)
        for size, filt in ((None, "bilinear"), ((48, 64), "bilinear")):
            for kw in (dict(bit_depth=8), dict(bit_depth=10, dtype=torch.float32), dict(bit_depth=8, dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)):
                kw = dict(kw, layout="rgb", size=size, filter=filt)
                if size is None:
                    kw.update(windows=[(2 * (i % 5), 2 * (i % 3), 190, 64) for i in range(16)], flip=[i % 3 == 0 for i in range(16)])
                else:
                    w, f = export.random_resized_crop(16, W, H, scale=(0.2, 1.0), generator=gen, chroma_format=1)
                    kw.update(windows=w, flip=f)
                planar = P.ctx.export_batch(pics, **kw)
                a = P.ctx.export_batch(pics, pixel="rgb", **kw)
                b = P.ctx.export_batch(pics[::-1], pixel="bgra", **dict(kw, windows=kw["windows"][::-1], flip=kw["flip"][::-1]))   # (no sync between)
                assert torch.equal(a, planar.permute(0, 2, 3, 1))
                assert torch.equal(b[..., :3], torch.flip(planar, dims=[0, 1]).permute(0, 2, 3, 1))
                whole = P.ctx.export_batch(pics, crop=(2, 4, 2, 6), **dict(kw, windows=None, flip=None))
                assert torch.equal(P.ctx.export_batch(pics, crop=(2, 4, 2, 6), pixel="rgb", **dict(kw, windows=None, flip=None)), whole.permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------ 5. refusals on the device
def _hip():
    """the HIP runtime this process already runs on"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            L.hipFree.argtypes = [C.c_void_p]
            L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return L
    raise RuntimeError("no HIP runtime loaded")


def test_refusals_leave_the_destination_untouched():
    """a host pointer, a span past the end of its allocation, a batch stride too small, an invalid handle in the middle of the list,
    a bad pixel description: HMGPU_EINVAL from the entry point and from the destination check, the canary intact; then the call that
    is not refused writes"""
    torch = _torch()
    n, w, h = 4, 94, 40
    with Pictures(1, count=3) as P:
        pics = P.pics + P.pics[:1]
        desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        wins = [wref.window_of(P.seq, (2 * i, 2 * i, w, h), i & 1) for i in range(n)]
        px = abi.make_export_pixel(abi.PIXEL_BGRA)
        dst = canary((n, h, w, 4), torch.uint8)
        stream = torch.cuda.current_stream().cuda_stream
        pitch, bstride = w * 4, h * w * 4
        gone = P.ctx.acquire()
        P.ctx.upload(gone, P.planes[P.pics[0]])
        P.ctx.release(gone)
        host = np.zeros(n * bstride, np.uint8)

        def refused(pics_=pics, px_=px, ptr=None, pitch_=pitch, bstride_=bstride, wins_=wins, check=True):
            ptr = dst.data_ptr() if ptr is None else ptr
            with pytest.raises(libhm_amd.HmgpuError) as e:
                P.ctx.export_pixels_into(pics_, desc, px_, ptr, pitch_, bstride_, 1, stream, None, None, wins_)
            assert e.value.status == abi.HMGPU_EINVAL
            if check:
                assert P.ctx.export_pixels_destination_status(len(pics_), desc, px_, ptr, pitch_, bstride_, None, None, wins_) == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            P.ctx.sync()
            assert bool((dst == CANARY).all())

        refused(ptr=host.ctypes.data)                                        # a host pointer
        hip = _hip()                                                         # the last slot one byte past an allocation of its own
        raw = C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), n * bstride - 1) == 0
        try:
            assert hip.hipMemset(raw, CANARY, n * bstride - 1) == 0
            refused(ptr=raw.value)
            back = np.zeros(n * bstride - 1, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, n * bstride - 1, 2) == 0
            assert (back == CANARY).all()
            P.ctx.export_pixels_into(pics[:3], desc, px, raw.value, pitch, bstride, 1, stream, None, None, wins[:3])      # three fit
            torch.cuda.synchronize()
        finally:
            hip.hipFree(raw)
        refused(bstride_=bstride - 1)                                        # a batch stride one byte short of a picture
        refused(pitch_=pitch - 1)
        refused(ptr=0)
        refused(pics_=[pics[0], gone, pics[2], pics[3]], check=False)        # an invalid handle in the middle (the check names no picture)
        refused(pics_=[pics[0], pics[1], -1, pics[3]], check=False)
        refused(px_=abi.make_export_pixel(9))
        refused(px_=abi.make_export_pixel(abi.PIXEL_BGRA, 256))
        refused(px_=None, check=False)
        refused(wins_=wins[:3] + [wref.window_of(P.seq, (0, 0, w, h - 2))])  # unscaled: another size
        assert P.ctx.export_pixels_destination_status(n, desc, px, dst.data_ptr(), pitch, bstride, None, None, wins) == abi.HMGPU_OK
        torch.cuda.synchronize()
        assert bool((dst == CANARY).all())
        P.ctx.export_pixels_into(pics, desc, px, dst.data_ptr(), pitch, bstride, 1, stream, None, None, wins)
        for i, p in enumerate(pics):
            assert np.array_equal(bits(dst[i]), P.want(p, (2 * i, 2 * i, w, h), bool(i & 1), U8, "bgra", None))


# ------------------------------------------------------------------------------------------------ 6. decoder
def fetched(dec, nals):
    """the pictures put out after each push"""
    for i, nal in enumerate(nals):
        while True:
            new_pic, check = dec.push(nal, i == len(nals) - 1)
            got = []
            while check:
                p = dec.get_picture()
                if p is None:
                    break
                got.append(p)
            if got:
                yield got
            if not new_pic:
                break


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_decoder(devices):
    """Decoder.frames(pixel="bgra") and frames(batch=4, memory_format=torch.channels_last, float16 ImageNet) equal the planar frames
    permuted; hmdec.export_batch(pixel=) of the pictures fetched after a push.  devices [0, 0]: two device contexts on one GPU (the
    hmdec_set_devices path: the destination validated once, then one call per run of slots)"""
    torch = _torch()
    z = gu.load("lite_ra_notmvp_main8_208x120")
    frames = int(z["geom"][2])
    kw = dict(threads=1, device_output=True, devices=devices)
    with hmdec.Decoder(**kw) as d:
        planar = {poc: t.clone() for poc, t in d.frames(z["bitstream"], layout="rgb")}
    assert len(planar) == frames
    with hmdec.Decoder(**kw) as d:
        seen = []
        for poc, t in d.frames(z["bitstream"], layout="rgb", pixel="bgra", alpha=77):
            hh, ww = planar[poc].shape[1:]
            assert t.shape == (hh, ww, 4) and t.dtype == torch.uint8
            assert torch.equal(t[..., :3], torch.flip(planar[poc], dims=[0]).permute(1, 2, 0)) and bool((t[..., 3] == 77).all())
            seen.append(poc)
        assert d.download_bytes == 0
    assert sorted(seen) == sorted(planar)
    fkw = dict(layout="rgb", dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)
    with hmdec.Decoder(**kw) as d:
        fplanar = {}
        for pocs, t in d.frames(z["bitstream"], batch=4, **fkw):
            fplanar.update({poc: t[i].clone() for i, poc in enumerate(pocs)})
    with hmdec.Decoder(**kw) as d:
        seen = []
        for pocs, t in d.frames(z["bitstream"], batch=4, memory_format=torch.channels_last, **fkw):
            assert t.shape[1] == 3 and t.dtype == torch.float16
            assert t.is_contiguous(memory_format=torch.channels_last) or len(pocs) < 4
            assert t.stride()[1:] == (1, 3 * t.shape[3], 3)
            for i, poc in enumerate(pocs):
                assert torch.equal(t[i], fplanar[poc]), poc
            seen += pocs
    assert sorted(seen) == sorted(fplanar) and len(seen) == frames
    # hmdec.export_batch: the pictures fetched after one push (each twice), windows and flips, packed against planar
    total = 0
    with hmdec.Decoder(**kw) as d:
        for got in fetched(d, hmdec.split_nal_units(z["bitstream"])):
            pictures = got + got
            xywh = [(2 * ((3 * i) % 7), 2 * (i % 5), 94, 60) for i in range(len(pictures))]
            flips = [i % 2 == 0 for i in range(len(pictures))]
            for size in (None, (30, 44)):
                want = hmdec.export_batch(pictures, layout="rgb", windows=xywh, flip=flips, size=size)
                got_px = hmdec.export_batch(pictures, layout="rgb", windows=xywh, flip=flips, size=size, pixel="argb")
                assert got_px.shape == (len(pictures),) + tuple(want.shape[2:]) + (4,)
                assert torch.equal(got_px[..., 1:], want.permute(0, 2, 3, 1)) and bool((got_px[..., 0] == 255).all())
            one = got[0].export(layout="rgb", pixel="rgb")
            assert torch.equal(one, got[0].export(layout="rgb").permute(1, 2, 0))
            total += len(got)
    assert total == frames
