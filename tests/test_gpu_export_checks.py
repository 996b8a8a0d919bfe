"""What the export side promises about its own bookkeeping, on the GPU: a destination check returns exactly the status the export
gives the same destination (all eight families), and the table slots of the scaled export give the same bits after an eviction as a
fresh context does.  What the other GPU tests hold of this: test_gpu_export_pixels has all four destination cases with the check
next to the export; test_gpu_export_batch has the batch stride and the short allocation for the export and the batch stride for the
check; test_gpu_export_windows the batch stride for the check; test_gpu_motion and test_gpu_residual the short allocation for both
and the strides for the check.  None has the null pointer or the short pitch as a pair (but pixels), and none evicts a slot."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import synth
from tests.test_gpu_motion import Ctx, _hip, make_seq, picture

pytestmark = pytest.mark.gpu

W = H = 64
CANARY = 0x5A


def _torch():
    import torch
    return torch


def _status(call):
    try:
        call()
    except libhm_amd.HmgpuError as e:
        return e.status
    return abi.HMGPU_OK


def _families(ctx, pics, stream):
    """per family: the bytes two 64x64 pictures take, and (base or None, pitch, batch stride) -> (the check's status, the export's status)"""
    n = len(pics)
    rgb = abi.make_export_desc(abi.EXPORT_RGB, 8, 1)
    wins = [abi.make_export_window((0, 0, 0, 0)), abi.make_export_window((0, 0, 0, 0), True)]
    px = abi.make_export_pixel(abi.PIXEL_RGBA)
    mdesc = abi.make_motion_desc(abi.MOTION_BLOCKS, 3)
    rdesc = abi.make_residual_desc(abi.RESIDUAL_PLANES, 1)
    plane = W * H
    axis = np.array([0, 255], np.uint16)
    b, g, r = np.meshgrid(axis, axis, axis, indexing="ij")
    lut = ctx.colour_lut(np.stack([r, g, b], axis=-1), None, 8)          # the identity, two nodes per axis
    chroma = abi.make_export_chroma(abi.CHROMA_LINEAR, 0)
    warp = (abi.make_export_warp(W, H), abi.warp_map_array([(65536, 0, 0, 0, 65536, 0)] * n))

    def planes(base, pitch, bstride):                # R and G of a picture side by side, then every picture's B: its pitch and batch stride vary
        ptrs = [None if base is None else base + k * plane for k in (0, 1, 2 * n)]
        return ptrs, [W, W, pitch], [2 * plane, 2 * plane, bstride]

    def batch(base, pitch, bstride):
        a = planes(base, pitch, bstride)
        return (ctx.export_destination_status(n, rgb, *a),
                _status(lambda: ctx.export_batch_into(pics, rgb, *a, 1, stream)))

    def windows(base, pitch, bstride):
        a = planes(base, pitch, bstride)
        return (ctx.export_windows_destination_status(rgb, *a, wins),
                _status(lambda: ctx.export_batch_into(pics, rgb, *a, 1, stream, windows=wins)))

    def pixels(base, pitch, bstride):
        return (ctx.export_pixels_destination_status(n, rgb, px, base, pitch, bstride),
                _status(lambda: ctx.export_pixels_into(pics, rgb, px, base, pitch, bstride, 1, stream)))

    def colour(base, pitch, bstride):
        a = planes(base, pitch, bstride)
        return (ctx.export_colour_destination_status(n, rgb, lut, *a),
                _status(lambda: ctx.export_colour_into(pics, rgb, lut, *a, 1, stream)))

    def chroma_(base, pitch, bstride):
        a = planes(base, pitch, bstride)
        return (ctx.export_chroma_destination_status(n, rgb, chroma, *a),
                _status(lambda: ctx.export_chroma_into(pics, rgb, chroma, *a, 1, stream)))

    def warp_(base, pitch, bstride):
        a = planes(base, pitch, bstride)
        return (ctx.export_warp_destination_status(n, rgb, warp, *a),
                _status(lambda: ctx.export_warp_into(pics, rgb, warp, *a, 1, stream)))

    def motion(base, pitch, bstride):                # ref_poc alone: int32 [n, 2, 16, 16]
        a = ([None, None, base, None], [0, 0, pitch, 0], [0, 0, 16 * 16 * 4, 0], [0, 0, bstride, 0])
        return (ctx.motion_destination_status(n, mdesc, *a),
                _status(lambda: ctx.export_motion_into(pics, mdesc, *a, 1, stream)))

    def residual(base, pitch, bstride):              # luma alone: int16 [n, 64, 64]
        a = ([base, None, None], [pitch, 0, 0], [0, 0, 0], [bstride, 0, 0])
        return (ctx.residual_destination_status(n, rdesc, *a),
                _status(lambda: ctx.export_residual_into(pics, rdesc, *a, 1, stream)))

    # name: (both statuses, bytes of n pictures, the pitch, the batch stride)
    return {"batch": (batch, n * 3 * plane, W, plane), "windows": (windows, n * 3 * plane, W, plane),
            "pixels": (pixels, n * plane * 4, W * 4, plane * 4), "colour": (colour, n * 3 * plane, W, plane),
            "chroma": (chroma_, n * 3 * plane, W, plane), "warp": (warp_, n * 3 * plane, W, plane), "motion": (motion, n * 2 * 16 * 16 * 4, 16 * 4, 2 * 16 * 16 * 4),
            "residual": (residual, n * plane * 2, W * 2, plane * 2)}


@pytest.mark.parametrize("family", ["batch", "windows", "pixels", "colour", "chroma", "warp", "motion", "residual"])
def test_destination_status_is_the_exports_status(family):
    """a destination that fits exactly, then a null pointer, a pitch one byte short, a batch stride one byte short, and an allocation
    that ends one byte before the last slot does: the check and the export agree every time, and a refusal writes nothing"""
    torch = _torch()
    seq = make_seq(W, H)
    hip = _hip()
    with Ctx(seq) as c:
        good = c.decode(picture(seq, 7, True, 0.2))
        both, total, pitch, bstride = _families(c.ctx, [good, good], torch.cuda.current_stream().cuda_stream)[family]
        raw, short = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), total) == 0 and hip.hipMalloc(C.byref(short), total - 1) == 0
        try:
            assert hip.hipMemset(raw, CANARY, total) == 0 and hip.hipMemset(short, CANARY, total - 1) == 0
            E = abi.HMGPU_EINVAL
            assert both(None, pitch, bstride) == (E, E)
            assert both(raw.value, pitch - 1, bstride) == (E, E)
            assert both(raw.value, pitch, bstride - 1) == (E, E)
            assert both(short.value, pitch, bstride) == (E, E)
            torch.cuda.synchronize()
            c.ctx.sync()
            back = np.zeros(total, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, total, 2) == 0 and (back == CANARY).all()
            assert hip.hipMemcpy(back.ctypes.data, short, total - 1, 2) == 0 and (back[:total - 1] == CANARY).all()
            assert both(raw.value, pitch, bstride) == (abi.HMGPU_OK, abi.HMGPU_OK)
            torch.cuda.synchronize()
            c.ctx.sync()
        finally:
            hip.hipFree(raw)
            hip.hipFree(short)


# nine (crop, (height, width)): one more than the context has table slots; outputs from 8x8 to 24x16
SHAPES = [((0, 0, 0, 0), (8, 8)), ((2, 0, 0, 0), (8, 10)), ((0, 2, 0, 0), (10, 12)), ((0, 0, 2, 0), (12, 14)), ((0, 0, 0, 2), (12, 16)),
          ((4, 4, 0, 0), (14, 18)), ((0, 0, 4, 4), (16, 20)), ((2, 2, 2, 2), (16, 22)), ((8, 0, 8, 0), (16, 24))]


@pytest.mark.parametrize("layout", ["rgb", "planar"])
def test_an_evicted_table_slot_is_filled_again(layout):
    """nine scaled exports of distinct crop and size on one context, then the first shape again (its slot was the least recently used
    one and went to the ninth): every result is bit-equal to the same call on a fresh context"""
    seq = make_seq(W, H)
    planes = [synth.noise_planes(W, H, 10, 5 + k, 1) for k in range(2)]

    def context():
        ctx = libhm_amd.Context(seq)
        for p in planes:
            ctx.upload(ctx.acquire(), p)
        return ctx

    def run(ctx, crop, size):
        out = ctx.export_batch([0, 1], layout, 8, crop=crop, size=size, filter="bicubic")
        return [t.cpu().numpy() for t in (out if isinstance(out, (tuple, list)) else [out])]

    with context() as old:
        for crop, size in SHAPES + SHAPES[:2]:
            got = run(old, crop, size)
            with context() as fresh:
                want = run(fresh, crop, size)
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), (crop, size)
