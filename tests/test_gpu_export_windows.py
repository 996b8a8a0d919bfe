"""Batched export with a source window and a mirror per picture on the GPU: hmgpu_pictures_export_windows /
hmdec_pictures_export_windows behind Context.export_batch(windows=, flip=), hmdec.export_batch and Decoder.frames(windows=).  Every
slot is compared bit for bit with the numpy restatement (tests/export_windows_ref.py: the batched reference at the slot's crop, rows
reversed): unscaled and scaled, at the scaling limits, against the existing call, into strided views, back to back without
synchronisation, and through the decoder."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, hmdec
from tests import export_batch_ref as bref
from tests import export_ref as ref
from tests import export_windows_ref as wref
from tests import golden_util as gu
from tests import scale_ref as sref

pytestmark = pytest.mark.gpu

W, H = 200, 72
CANARY = 0xA5
LAYOUTS = {"planar": ref.PLANAR, "nv12": ref.SEMIPLANAR, "rgb": ref.RGB}
FILTER_NAMES = {abi.SCALE_NEAREST: "nearest", abi.SCALE_BILINEAR: "bilinear", abi.SCALE_BICUBIC: "bicubic", abi.SCALE_AREA: "area"}


def _torch():
    import torch
    return torch


def random_planes(w, h, fmt, bd, seed):
    rng = np.random.default_rng(seed)
    sx, sy = ref.chroma_shift(fmt)
    return [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + \
           [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]


def seq_of(fmt, bd, max_pictures=8, w=W, h=H):
    seq = abi.make_seq(w, h, bd[0], bd[1], max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def bits(t):
    """a tensor's elements as unsigned integers of their own width (bit patterns), on the host"""
    torch = _torch()
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]
    a = t.contiguous().view(view).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[t.element_size()])


def as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


class Pictures:
    """a context with `count` uploaded random pictures; the references of (picture, window, export) are computed once"""

    def __init__(self, fmt, bd=(10, 10), count=4, seed=0, max_pictures=8):
        self.fmt, self.bd = fmt, bd
        self.seq = seq_of(fmt, bd, max_pictures)
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

    def want(self, pic, xywh, flip, layout, depth, msb, size, filt, st_type):
        """the planes of one slot: the unmirrored reference cached, the mirror applied per slot"""
        key = (pic, xywh, layout, depth, msb, size, filt, st_type)
        if key not in self.cache:
            desc = abi.make_export_desc(LAYOUTS[layout], depth, 1 if depth <= 8 else 2, msb, (0, 0, 0, 0), 1, 0)
            scale = None if size is None else sref.scale_of(size, filt)
            tensor = None if st_type is None else abi.make_export_tensor(st_type, *export.affine(depth, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
            self.cache[key] = wref.export_slot_ref(self.seq, self.planes[pic], self.fmt, self.bd, desc, scale, tensor,
                                                   wref.window_of(self.seq, xywh))
        return wref.mirror(self.cache[key], LAYOUTS[layout]) if flip else self.cache[key]

    def export(self, pics, windows, flips, layout, depth, msb=0, size=None, filt=abi.SCALE_BILINEAR, st_type=None, **kw):
        torch = _torch()
        if st_type is not None:
            kw = dict(kw, dtype={abi.SAMPLE_F16: torch.float16, abi.SAMPLE_F32: torch.float32}[st_type], mean=bref.IMAGENET_MEAN,
                      std=bref.IMAGENET_STD)
        return self.ctx.export_batch(pics, layout, depth, matrix=1, full_range=0, msb_aligned=bool(msb), size=size,
                                     filter=FILTER_NAMES[filt], windows=windows, flip=flips, **kw)

    def check(self, got, pics, windows, flips, layout, depth, msb=0, size=None, filt=abi.SCALE_BILINEAR, st_type=None):
        got = as_tuple(got)
        for i, p in enumerate(pics):
            want = self.want(p, tuple(windows[i]), bool(flips[i]), layout, depth, msb, size, filt, st_type)
            where = (self.fmt, layout, depth, msb, size, filt, st_type, i, windows[i], flips[i])
            if layout == "rgb":
                assert got[0].shape == (len(pics), 3) + want[0].shape, where
                assert np.array_equal(bits(got[0][i]), np.stack(want)), where
            else:
                assert len(got) == len(want), where
                for k in range(len(want)):
                    assert got[k].shape == (len(pics),) + want[k].shape, where
                    assert np.array_equal(bits(got[k][i]), want[k]), where + (k,)

    def run(self, pics, windows, flips, layout, depth, msb=0, size=None, filt=abi.SCALE_BILINEAR, st_type=None):
        self.check(self.export(pics, windows, flips, layout, depth, msb, size, filt, st_type), pics, windows, flips, layout, depth, msb,
                   size, filt, st_type)


# ------------------------------------------------------------------------------------------------ 1. unscaled
# 96 x 40 at left edges 0, 2, 4 and 6 and at the right and bottom borders; 94 x 40 (no multiple of 4: mirrored partial groups) the same
ORIGINS_96 = [(0, 0), (2, 2), (4, 4), (6, 6), (W - 96, 10), (10, H - 40), (W - 96, H - 40)]
ORIGINS_94 = [(0, 0), (2, 2), (4, 4), (6, 6), (W - 94, 10), (10, H - 40), (W - 94, H - 40)]


@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_unscaled_windows_and_mirrors(fmt, n):
    """equal-size windows at different origins, alternating flips (n = 1: a flipped window at left edge 2), every layout, u8 and
    10 bits msb-aligned in u16"""
    with Pictures(fmt, count=min(n, 5)) as P:
        pics = [P.pics[i % len(P.pics)] for i in range(n)]
        for k, (w, origins) in enumerate(((96, ORIGINS_96), (94, ORIGINS_94))):
            windows = [origins[(i + 1) % len(origins)] + (w, 40) for i in range(n)]
            flips = [(i + k) % 2 == 0 for i in range(n)]
            for layout in ("planar", "nv12", "rgb"):
                for depth, msb in ((8, 0), (10, 1)):
                    P.run(pics, windows, flips, layout, depth, msb)
        if n == 16:                                              # float elements take the same stores: once, all flipped or none
            windows = [ORIGINS_94[i % len(ORIGINS_94)] + (94, 40) for i in range(n)]
            P.run(pics, windows, [True] * n, "rgb", 8, st_type=abi.SAMPLE_F16)
            P.run(pics, windows, [False] * n, "planar", 10, st_type=abi.SAMPLE_F32)


# ------------------------------------------------------------------------------------------------ 2. scaled
# 16 x 16, the whole picture, 64 x 72, 198 x 70 at (2, 2), a window on the right border, one on the bottom border
MIXED = [(8, 8, 16, 16), (0, 0, 200, 72), (20, 0, 64, 72), (2, 2, 198, 70), (120, 10, 80, 40), (10, 42, 100, 30)]
# 160 outputs from 16 samples would be a 10x enlargement, beyond the 8x limit: the small window is 20 x 16 for that output
MIXED_160 = [(8, 8, 20, 16)] + MIXED[1:]
SCALED_OUTPUTS = [((24, 40), MIXED), ((22, 30), MIXED), ((40, 160), MIXED_160)]          # size = (height, width)


@pytest.mark.parametrize("filt,fmt", [(abi.SCALE_NEAREST, 1), (abi.SCALE_BILINEAR, 1), (abi.SCALE_BICUBIC, 1), (abi.SCALE_AREA, 1),
                                      (abi.SCALE_NEAREST, 3), (abi.SCALE_BILINEAR, 3), (abi.SCALE_BICUBIC, 3), (abi.SCALE_AREA, 3),
                                      (abi.SCALE_BICUBIC, 2), (abi.SCALE_BILINEAR, 0)])
def test_scaled_windows_of_mixed_sizes(filt, fmt):
    """one call of 16 slots mixes windows of six sizes (each with its own tables, spans and passes), flips on the odd slots; outputs
    40 x 24, 30 x 22 and 160 x 40 (several tile columns whose source spans differ per picture)"""
    n = 16
    with Pictures(fmt, count=4) as P:
        pics = [P.pics[i % 4] for i in range(n)]
        flips = [i % 2 == 1 for i in range(n)]
        for size, mixed in SCALED_OUTPUTS:
            windows = [mixed[i % len(mixed)] for i in range(n)]
            for layout in ("rgb", "planar", "nv12"):
                P.run(pics, windows, flips, layout, 8, 0, size, filt)
                if layout != "nv12":
                    P.run(pics, windows, flips, layout, 8, 0, size, filt, abi.SAMPLE_F16)


# ------------------------------------------------------------------------------------------------ 3. at the limits
@pytest.mark.parametrize("fmt", [1, 3])
def test_windows_at_the_scaling_limits(fmt):
    """a 192 x 64 window to 6 x 2 (32x reduction on both axes), an 8 x 8 window to 64 x 64 (8x enlargement on both), each beside
    windows well inside the limits; and both limits in one call (192 x 64 and 8 x 8 to 6 x 64: 32x horizontally for the one, 8x
    vertically for the other).  One window just beyond a limit refuses the call and the destination keeps its canary."""
    torch = _torch()
    with Pictures(fmt, count=3) as P:
        pics = P.pics + P.pics[:1]
        flips = [False, True, True, False]
        # one call has one output size, so 192 x 64 -> 6 x 2 and 8 x 8 -> 64 x 64 cannot share a call: each runs beside ordinary windows,
        # and a third call (6 x 64 outputs) holds a window at the 32x limit and one at the 8x limit at once
        for filt in (abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
            for layout in ("rgb", "nv12"):
                P.run(pics, [(4, 2, 192, 64), (0, 0, 96, 40), (4, 2, 192, 64), (100, 8, 100, 64)], flips, layout, 8, 0, (2, 6), filt)
                P.run(pics, [(6, 4, 8, 8), (0, 0, 64, 64), (192, 64, 8, 8), (20, 0, 128, 72)], flips, layout, 8, 0, (64, 64), filt)
                P.run(pics, [(4, 2, 192, 64), (6, 4, 8, 8), (192, 64, 8, 8), (8, 8, 192, 64)], flips, layout, 8, 0, (64, 6), filt)
        # refusals: the Python layer (the plan), then the entry point itself with a canary-filled destination
        with pytest.raises(libhm_amd.HmgpuError) as e:
            P.export(pics, [(4, 2, 192, 64), (0, 0, 96, 40), (4, 2, 194, 64), (0, 0, 96, 40)], flips, "rgb", 8, size=(2, 6))
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        dst = torch.full((4, 3, 64, 64), CANARY, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def refused(windows, size, status, desc_=desc, flips_=flips):
            hh, ww = size if size is not None else (64, 64)
            wins = [wref.window_of(P.seq, w, f) if not isinstance(w, abi.ExportWindow) else w for w, f in zip(windows, flips_)]
            with pytest.raises(libhm_amd.HmgpuError) as e:
                P.ctx.export_batch_into(pics, desc_, [dst.data_ptr() + k * hh * ww for k in range(3)], [ww] * 3, [3 * hh * ww] * 3, 1, stream,
                                        None if size is None else sref.scale_of(size, abi.SCALE_BILINEAR), None, wins)
            assert e.value.status == status
            torch.cuda.synchronize()
            P.ctx.sync()
            assert bool((dst == CANARY).all())

        U, E = abi.HMGPU_EUNSUPPORTED, abi.HMGPU_EINVAL
        good = [(4, 2, 192, 64), (0, 0, 96, 40), (4, 2, 192, 64), (0, 0, 96, 40)]
        for place in range(4):
            for bad in ((4, 2, 194, 64), (4, 2, 192, 66)):                        # one luma sample pair beyond the 32x reduction
                refused(good[:place] + [bad] + good[place + 1:], (2, 6), U)
            refused([(6, 4, 8, 8)] * place + [(6, 4, 6, 8)] + [(6, 4, 8, 8)] * (3 - place), (64, 64), U)     # beyond the 8x enlargement
            refused([(0, 0, 64, 64)] * place + [(0, 0, 64, 62)] + [(0, 0, 64, 64)] * (3 - place), None, E)  # unscaled: another size
        odd = wref.window_of(P.seq, (0, 0, 64, 64))
        odd.flip = 2
        refused([(0, 0, 64, 64)] * 3 + [odd], None, E)
        odd = wref.window_of(P.seq, (0, 0, 64, 64))
        odd.reserved[2] = 1
        refused([odd] + [(0, 0, 64, 64)] * 3, None, E)
        refused([(0, 0, 64, 64)] * 4, None, E, desc_=abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 2, 0, 0), 1, 0))   # desc->crop is not 0
        # and the call that is not refused writes
        P.ctx.export_batch_into(pics, desc, [dst.data_ptr() + k * 64 * 64 for k in range(3)], [64] * 3, [3 * 64 * 64] * 3, 1, stream, None, None,
                                [wref.window_of(P.seq, (0, 0, 64, 64), f) for f in flips])
        P.check(dst, pics, [(0, 0, 64, 64)] * 4, flips, "rgb", 8)


# ------------------------------------------------------------------------------------------------ 4. identity with the existing call
@pytest.mark.parametrize("size,filt", [(None, abi.SCALE_BILINEAR), ((24, 40), abi.SCALE_BICUBIC)])
def test_equal_unflipped_windows_equal_the_existing_call(size, filt):
    """sixteen equal unflipped windows write what hmgpu_pictures_export with that crop writes (and take its table slot); all
    flipped, its mirror image"""
    torch = _torch()
    with Pictures(1, count=4) as P:
        pics = [P.pics[i % 4] for i in range(16)]
        x, y, w, h = 6, 2, 180, 60
        crop = (x, W - x - w, y, H - y - h)
        for layout, kw in (("rgb", dict(dtype=torch.float16, mean=bref.IMAGENET_MEAN, std=bref.IMAGENET_STD)), ("nv12", {}), ("planar", {})):
            kw = dict(kw, layout=layout, bit_depth=8, size=size, filter=FILTER_NAMES[filt])
            old = as_tuple(P.ctx.export_batch(pics, crop=crop, **kw))
            new = as_tuple(P.ctx.export_batch(pics, windows=[(x, y, w, h)] * 16, **kw))
            rel = as_tuple(P.ctx.export_batch(pics, crop=(2, 4, 2, 2), windows=[(x - 2, y - 2, w, h)] * 16, flip=[False] * 16, **kw))
            mir = as_tuple(P.ctx.export_batch(pics, windows=[(x, y, w, h)] * 16, flip=[True] * 16, **kw))
            for a, b, c, m in zip(old, new, rel, mir):
                assert torch.equal(a, b) and torch.equal(a, c)
                assert torch.equal(torch.flip(a, dims=[-2 if layout == "nv12" and a.dim() == 4 else -1]), m)


# ------------------------------------------------------------------------------------------------ 5. strides and canaries
@pytest.mark.parametrize("offset", [1, 4])          # elements: 1 = no vector stores possible, 4 = 16-byte aligned rows
@pytest.mark.parametrize("size", [None, (22, 30)])
def test_strided_out_views_keep_their_canaries(offset, size):
    """out= views into larger canary-filled tensors, mirrored slots and not: every byte outside the planned samples keeps its canary
    and the samples are those of the dense call (float16 RGB, uint8 semi-planar; unscaled windows of 94 x 40)"""
    torch = _torch()
    n = 3
    with Pictures(1, count=n) as P:
        pics = P.pics
        windows = [(2, 2, 94, 40), (4, 4, 94, 40), (W - 94, H - 40, 94, 40)] if size is None else [(8, 8, 20, 16), (0, 0, 200, 72), (2, 2, 198, 70)]
        hh, ww = size or (40, 94)

        def canary(shape, dtype):
            return torch.full(shape, CANARY, dtype=torch.uint8, device="cuda").view(dtype)

        def check(big, view_of, want):
            expect = canary(tuple(big.shape[:-1]) + (big.shape[-1] * big.element_size(),), big.dtype)
            view_of(expect).copy_(want)
            assert torch.equal(big.view(torch.uint8), expect.view(torch.uint8))

        for flips in ([True, False, True], [False, True, False]):
            kw = dict(size=size, filt=abi.SCALE_BICUBIC)
            rgb_view = lambda t: t[::2, 1:4, 1:hh + 1, offset:offset + ww]
            big = canary((2 * n, 4, hh + 3, 2 * (ww + 18)), torch.float16)
            r = P.export(pics, windows, flips, "rgb", 8, st_type=abi.SAMPLE_F16, out=rgb_view(big), **kw)
            assert r.data_ptr() == rgb_view(big).data_ptr()
            dense = P.export(pics, windows, flips, "rgb", 8, st_type=abi.SAMPLE_F16, **kw)
            P.check(dense, pics, windows, flips, "rgb", 8, st_type=abi.SAMPLE_F16, **kw)
            check(big, rgb_view, dense)
            dense = P.export(pics, windows, flips, "nv12", 8, **kw)
            P.check(dense, pics, windows, flips, "nv12", 8, **kw)
            big_y = canary((n + 1, hh + 2, ww + 14), torch.uint8)
            big_c = canary((n + 1, hh // 2 + 2, ww // 2 + 7, 2), torch.uint8)
            y_view = lambda t: t[:n, 1:hh + 1, offset:offset + ww]
            c_view = lambda t: t[1:, :hh // 2, offset // 2 + 1:offset // 2 + 1 + ww // 2]
            P.export(pics, windows, flips, "nv12", 8, out=(y_view(big_y), c_view(big_c)), **kw)
            check(big_y, y_view, dense[0])
            check(big_c, c_view, dense[1])


# ------------------------------------------------------------------------------------------------ 6. per-call table buffers
def test_back_to_back_calls_keep_their_tables():
    """twelve scaled calls of 16 random windows each, more than there are per-call table buffers, issued without host
    synchronisation, each into its own tensor and checked after one final sync: a buffer rewritten while an export still reads it
    would show as a wrong slot"""
    torch = _torch()
    calls, n, size = 12, 16, (24, 40)
    gen = torch.Generator().manual_seed(5)
    with Pictures(1, count=4) as P:
        pics = [P.pics[i % 4] for i in range(n)]
        jobs = [export.random_resized_crop(n, W, H, scale=(0.2, 1.0), generator=gen, chroma_format=1) for _ in range(calls)]
        assert len({w for ws, _ in jobs for w in ws}) > calls * n // 2          # (the windows differ: no key repeats)
        outs = [P.export(pics, ws, fs, "rgb", 8, 0, size, abi.SCALE_BICUBIC, abi.SAMPLE_F16) for ws, fs in jobs]
        torch.cuda.synchronize()
        for (ws, fs), out in zip(jobs, outs):
            P.check(out, pics, ws, fs, "rgb", 8, 0, size, abi.SCALE_BICUBIC, abi.SAMPLE_F16)


# ------------------------------------------------------------------------------------------------ 7. decoder
def host_pictures(z):
    """POC -> the planes of the host path, and the conformance window"""
    host, crop = {}, []
    with hmdec.Decoder() as d:
        def on_output(p):
            host[p.poc] = [np.asarray(p.plane(c)).astype(np.int16) for c in range(3)]
            crop.append(tuple(p.conformance_window()))
        d.decode_stream(z["bitstream"], on_output=on_output)
    return host, crop[0]


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
def test_decoder_frames_and_export_batch_with_windows(devices):
    """Decoder.frames(batch=4, windows=fn) with random-resized-crop windows, float16 ImageNet RGB at 64 x 48, and
    hmdec.export_batch(windows=, flip=) unscaled: every slot equals the reference computed from the host planes of the same picture"""
    torch = _torch()
    name = "ra_notmvp_main8_208x120"
    z = gu.load("lite_" + name)
    host, crop = host_pictures(z)
    frames = int(z["geom"][2])
    assert len(host) == frames
    fmt, bd, size = 1, (8, 8), (48, 64)
    seq = abi.make_seq(208, 120, 8, 8)
    cw, ch = 208 - crop[0] - crop[1], 120 - crop[2] - crop[3]
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    tensor = abi.make_export_tensor(abi.SAMPLE_F16, *export.affine(8, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
    scale = sref.scale_of(size, abi.SCALE_BILINEAR)
    gen = torch.Generator().manual_seed(11)
    handed = []

    def fn(n):
        w, f = export.random_resized_crop(n, cw, ch, generator=gen, chroma_format=fmt)
        handed.extend(zip(w, f))
        return w, f

    seen = []
    with hmdec.Decoder(threads=1 if devices else 2, device_output=True, devices=devices) as d:
        for pocs, t in d.frames(z["bitstream"], batch=4, windows=fn, layout="rgb", dtype=torch.float16, mean=bref.IMAGENET_MEAN,
                                std=bref.IMAGENET_STD, size=size, filter="bilinear"):
            assert t.shape == (len(pocs), 3) + size and t.dtype == torch.float16
            for i, poc in enumerate(pocs):
                w, f = handed[len(seen) + i]
                win = export.make_windows(seq, crop, [w], [f], 1)[0]
                want = wref.export_slot_ref(seq, host[poc], fmt, bd, desc, scale, tensor, win)
                assert np.array_equal(bits(t[i]), np.stack(want)), (poc, w, f)
            seen += pocs
        assert d.download_bytes == 0
    assert seen == sorted(host) and len(handed) == frames
    # hmdec.export_batch: the pictures fetched after one push (each twice), equal-size windows at different origins, planar integers
    pdesc = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    nals = hmdec.split_nal_units(z["bitstream"])
    total = 0
    with hmdec.Decoder(threads=1, device_output=True, devices=devices) as d:
        for got in fetched(d, nals):
            pictures = got + got
            xywh = [(2 * ((3 * i) % 7), 2 * (i % 5), 94, 60) for i in range(len(pictures))]
            flips = [i % 2 == 0 for i in range(len(pictures))]
            batch = hmdec.export_batch(pictures, layout="planar", bit_depth=8, windows=xywh, flip=flips)
            for i, p in enumerate(pictures):
                win = export.make_windows(seq, crop, [xywh[i]], [flips[i]], 1)[0]
                want = wref.export_slot_ref(seq, host[p.poc], fmt, bd, pdesc, None, None, win)
                for k in range(3):
                    assert np.array_equal(bits(batch[k][i]), want[k]), (p.poc, i, k)
            total += len(got)
    assert total == frames


def test_hmdec_refusals_with_windows():
    """pictures of two sequences (two decoders, 4:2:0 8-bit and 4:4:4 10-bit, either first) and pictures of two decoders of one
    sequence are refused with windows as without, and the destination stays untouched; the call is accepted again afterwards"""
    torch = _torch()
    a, b = gu.load("lite_ra_notmvp_main8_208x120"), gu.load("lite_ldb_444_main10_208x120")
    w = [(2, 2, 94, 60)]
    with hmdec.Decoder(device_output=True) as d, hmdec.Decoder(device_output=True) as d2, hmdec.Decoder(device_output=True) as d3:
        got = next(fetched(d, hmdec.split_nal_units(a["bitstream"])))
        same = next(fetched(d2, hmdec.split_nal_units(a["bitstream"])))
        other = next(fetched(d3, hmdec.split_nal_units(b["bitstream"])))
        out = tuple(torch.full((2,) + shape, CANARY, dtype=torch.uint8, device="cuda") for shape in ((60, 94), (30, 47), (30, 47)))
        for pictures in (got[:1] + other[:1], got[:1] + same[:1]):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                hmdec.export_batch(pictures, layout="planar", bit_depth=8, windows=w * 2, flip=[True, False], out=out)
            assert e.value.status == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            assert all(bool((t == CANARY).all()) for t in out)
        with pytest.raises((libhm_amd.HmgpuError, ValueError)):                    # (the first picture gives the geometry: 4:4:4 planes)
            hmdec.export_batch(other[:1] + got[:1], layout="planar", bit_depth=8, windows=w * 2, out=out)
        torch.cuda.synchronize()
        assert all(bool((t == CANARY).all()) for t in out)
        hmdec.export_batch(got[:1] * 2, layout="planar", bit_depth=8, windows=w * 2, flip=[True, False], out=out)
        assert torch.equal(out[0][0], torch.flip(out[0][1], dims=[-1])) and not bool((out[0] == CANARY).all())


def test_stale_pictures_are_refused():
    """a stale picture, in both forms the library can tell.  libhmdec: a picture of a sequence that has ended -- two clips back to
    back through a decoder with parser threads whose caller does not fetch on the push that is answered "new picture": what the first
    clip still had to put out is fetched after the second clip's first slice has replaced the picture store, so those pictures are
    alive (the decoder keeps them until the next change of sequence) but their device context is gone.  First, last and alone in a
    batch they are refused and the destination keeps its canary.  hmgpu: a released handle, first and last among 16."""
    torch = _torch()
    a, b = gu.load("lite_ra_notmvp_main8_208x120"), gu.load("lite_ldb_444_main10_208x120")
    nals = hmdec.split_nal_units(bytes(a["bitstream"]) + bytes(b["bitstream"]))
    w = (2, 2, 94, 60)
    out = tuple(torch.full((3, 60, 94), CANARY, dtype=torch.uint8, device="cuda") for _ in range(3))
    L = hmdec.lib()

    def raw_status(dec, pictures, flips):
        """hmdec_pictures_export_windows itself, past the Python layer's own look at the first picture"""
        g = pictures[0].geometry()
        seq = abi.make_seq(208, 120, g["bd_y"], g["bd_c"])
        desc = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        wins = (abi.ExportWindow * len(pictures))(*[wref.window_of(seq, w, f) for f in flips])
        h = (C.c_void_p * len(pictures))(*[p.h for p in pictures])
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in out])
        pitch, bstr = (C.c_int64 * 3)(94, 94, 94), (C.c_int64 * 3)(60 * 94, 60 * 94, 60 * 94)
        return L.hmdec_pictures_export_windows(dec.ctx, len(pictures), h, C.byref(desc), None, None, wins, ptrs, pitch, bstr, 1, None)

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == CANARY).all()) for t in out)

    checked = False
    with hmdec.Decoder(threads=2, device_output=True) as d:
        stale = []
        for i, nal in enumerate(nals):
            while True:
                new_pic, check = d.push(nal, i == len(nals) - 1)
                if new_pic:
                    continue                                     # not fetched now: the unit comes again first
                got = []
                while check:
                    p = d.get_picture()
                    if p is None:
                        break
                    got.append(p)
                stale += [p for p in got if p.device < 0]
                live = [p for p in got if p.device >= 0 and p.geometry()["chroma_format"] == 3]
                if stale and live and not checked:
                    checked = True
                    assert all(p.geometry()["chroma_format"] == 1 for p in stale)
                    kw = dict(layout="planar", bit_depth=8, out=out)
                    for pictures in ([live[0], live[0], stale[0]], [live[0], stale[-1], live[0]]):
                        with pytest.raises(libhm_amd.HmgpuError) as e:
                            hmdec.export_batch(pictures, windows=[w] * 3, flip=[True, False, True], **kw)
                        assert e.value.status == abi.HMGPU_EINVAL and untouched()
                    with pytest.raises(RuntimeError):            # first in the batch: the Python layer finds no device to allocate on
                        hmdec.export_batch([stale[0], live[0], live[0]], windows=[w] * 3, flip=[False] * 3, **kw)
                    assert untouched()
                    assert raw_status(d, [stale[0], live[0], live[0]], [0, 1, 0]) == abi.HMGPU_EINVAL and untouched()
                    assert raw_status(d, [stale[0]], [1]) == abi.HMGPU_EINVAL and untouched()
                    assert raw_status(d, [live[0], live[0], live[0]], [0, 1, 0]) == abi.HMGPU_OK and not untouched()
                break
    assert checked
    # a released handle of a context
    for t in out:
        t.fill_(CANARY)
    with Pictures(3, count=3, max_pictures=20) as P:
        gone = P.ctx.acquire()
        P.ctx.upload(gone, P.planes[P.pics[0]])
        P.ctx.release(gone)
        good = [P.pics[i % 3] for i in range(15)]
        desc = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        big = tuple(torch.full((16, 60, 94), CANARY, dtype=torch.uint8, device="cuda") for _ in range(3))
        wins = [wref.window_of(P.seq, (2 * (i % 4), 2, 94, 60), i & 1) for i in range(16)]
        for pics in ([gone] + good, good + [gone]):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                P.ctx.export_batch_into(pics, desc, [t.data_ptr() for t in big], [94] * 3, [60 * 94] * 3, 1,
                                        torch.cuda.current_stream().cuda_stream, None, None, wins)
            assert e.value.status == abi.HMGPU_EINVAL
            with pytest.raises(libhm_amd.HmgpuError) as e:
                P.ctx.export_batch(pics, "planar", 8, windows=[(2, 2, 94, 60)] * 16, flip=[True] * 16, out=big)
            assert e.value.status == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            P.ctx.sync()
            assert all(bool((t == CANARY).all()) for t in big)


def test_windows_destination_check():
    """hmgpu_export_windows_destination_check on its own (what libhmdec asks before it spreads a batch over several contexts): the
    status the export would give -- a window beyond a limit, windows of two sizes, a batch stride one byte short, not device memory --
    and nothing written"""
    torch = _torch()
    with Pictures(1, count=2) as P:
        desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
        scale = sref.scale_of((2, 6), abi.SCALE_BILINEAR)
        dst = torch.full((4, 3, 64, 64), CANARY, dtype=torch.uint8, device="cuda")
        U, E = abi.HMGPU_EUNSUPPORTED, abi.HMGPU_EINVAL

        def chk(windows, size, sc=None, base=None, short=0, **kw):
            hh, ww = size
            base = dst.data_ptr() if base is None else base
            wins = [wref.window_of(P.seq, w_) for w_ in windows]
            return P.ctx.export_windows_destination_status(desc, [base + k * hh * ww for k in range(3)], [ww] * 3,
                                                           [3 * hh * ww, 3 * hh * ww, hh * ww - short], wins, sc, None, **kw)

        good = [(4, 2, 192, 64), (0, 0, 96, 40), (8, 8, 192, 64), (100, 8, 100, 64)]
        assert chk(good, (2, 6), scale) == abi.HMGPU_OK
        assert chk(good[:3] + [(4, 2, 194, 64)], (2, 6), scale) == U                   # one window beyond the 32x reduction
        assert chk([(4, 2, 194, 64)] + good[1:], (2, 6), scale) == U
        assert chk([(0, 0, 64, 64)] * 4, (64, 64)) == abi.HMGPU_OK                      # unscaled: exactly the four slots of dst
        assert chk([(0, 0, 64, 64)] * 3 + [(0, 0, 64, 62)], (64, 64)) == E             # another size
        assert chk([(0, 0, 64, 64)] * 4, (64, 64), short=0) == abi.HMGPU_OK             # (a batch stride of exactly one plane)
        assert chk([(0, 0, 64, 64)] * 4, (64, 64), short=1) == E                       # a batch stride one byte short of a plane
        assert chk([(0, 0, 64, 64)] * 4, (64, 64), base=np.zeros(4 * 3 * 64 * 64, np.uint8).ctypes.data) == E
        assert chk([(0, 0, 64, 64)] * 4, (64, 64), n=0) == E and chk([(0, 0, 64, 64)] * 4, (64, 64), n=17) == E
        torch.cuda.synchronize()
        P.ctx.sync()
        assert bool((dst == CANARY).all())
