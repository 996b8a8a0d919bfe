"""Packed pixel export, host side (no GPU): hmgpu_export_pixel's size and offsets against the header and the ctypes mirror,
hmgpu_export_pixels_plan_for's geometry (one plane of W * C * ES bytes per row, the coef of the planar plan) and refusals (its own,
and each inherited one of the planar calls once), and the Python layer's reading of pixel= / alpha= / memory_format=."""
import ctypes as C
import math
import os
import subprocess

import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_ref as ref
from tests.export_windows_ref import window_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 200, 72
E, U, OK = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED, abi.HMGPU_OK
ORDERS = [abi.PIXEL_RGB, abi.PIXEL_BGR, abi.PIXEL_RGBA, abi.PIXEL_BGRA, abi.PIXEL_ARGB, abi.PIXEL_ABGR]


def seq_of(fmt, bd=10, w=W, h=H):
    s = abi.make_seq(w, h, bd, bd)
    s.chroma_format = fmt
    return s


def plan_status(seq, desc, scale, tensor, windows, pixel, n=None):
    plan = abi.ExportPlan()
    arr = None
    if windows is not None:
        windows = list(windows)
        arr = (abi.ExportWindow * max(len(windows), 1))(*windows)
    st = libhm_amd.lib().hmgpu_export_pixels_plan_for(C.byref(seq), C.byref(desc), C.byref(scale) if scale is not None else None,
                                                      C.byref(tensor) if tensor is not None else None,
                                                      (len(windows) if windows is not None else 1) if n is None else n, arr,
                                                      C.byref(pixel) if pixel is not None else None, C.byref(plan))
    return st, plan


def test_struct_matches_the_header_and_the_mirror(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d\\n",'
                   'sizeof(hmgpu_export_pixel),offsetof(hmgpu_export_pixel,order),offsetof(hmgpu_export_pixel,alpha),'
                   'offsetof(hmgpu_export_pixel,alpha_value),offsetof(hmgpu_export_pixel,reserved),HMGPU_PIXEL_RGB,HMGPU_PIXEL_BGR,'
                   'HMGPU_PIXEL_RGBA,HMGPU_PIXEL_BGRA,HMGPU_PIXEL_ARGB,HMGPU_PIXEL_ABGR);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P = abi.ExportPixel
    assert got[:5] == [C.sizeof(P), P.order.offset, P.alpha.offset, P.alpha_value.offset, P.reserved.offset] == [32, 0, 4, 8, 12]
    assert got[5:] == ORDERS == list(range(6))
    p = abi.make_export_pixel(abi.PIXEL_BGRA, 7, 0.5)
    assert (p.order, p.alpha, p.alpha_value, list(p.reserved)) == (3, 7, 0.5, [0] * 5)


TENSORS = [(None, 1, 8), (None, 2, 10), (abi.SAMPLE_F16, 2, 8), (abi.SAMPLE_BF16, 2, 8), (abi.SAMPLE_F32, 4, 10)]     # sample type, ES, depth


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_plan_geometry_and_coef(fmt):
    """one plane, the size in pixels, W * C * ES bytes per row (pixels of 3, 4, 6, 8, 12 and 16 bytes), the coef of the planar RGB
    plan: unscaled and scaled, with desc.crop and with windows"""
    seq = seq_of(fmt)
    sizes = set()
    for st_type, es, depth in TENSORS:
        tensor = None if st_type is None else abi.make_export_tensor(st_type)
        nbytes = 1 if depth <= 8 else 2
        for order in ORDERS:
            c = 3 if order <= abi.PIXEL_BGR else 4
            sizes.add(c * es)
            px = abi.make_export_pixel(order)
            for scale in (None, abi.make_export_scale(40, 24, abi.SCALE_BICUBIC)):
                desc = abi.make_export_desc(ref.RGB, depth, nbytes, 0, (2, 4, 2, 6), 1, 0)
                st, plan = plan_status(seq, desc, scale, tensor, None, px)
                planar = libhm_amd.export_tensor_plan(seq, desc, scale, tensor)
                w, h = (40, 24) if scale is not None else (W - 6, H - 8)
                assert st == OK and (planar.width[0], planar.height[0]) == (w, h)
                assert (plan.planes, list(plan.width), list(plan.height), list(plan.row_bytes)) == (1, [w, 0, 0], [h, 0, 0], [w * c * es, 0, 0])
                assert list(plan.coef) == list(planar.coef)
                assert libhm_amd.export_pixels_plan(seq, desc, scale, tensor, None, px).row_bytes[0] == w * c * es
                desc0 = abi.make_export_desc(ref.RGB, depth, nbytes, 0, (0, 0, 0, 0), 1, 0)
                wins = [window_of(seq, (2 * i, 2 * i, 94, 40), i & 1) for i in range(5)]
                st, plan = plan_status(seq, desc0, scale, tensor, wins, px)
                planar = libhm_amd.export_windows_plan(seq, desc0, scale, tensor, wins)
                w, h = (40, 24) if scale is not None else (94, 40)
                assert st == OK
                assert (plan.planes, list(plan.width), list(plan.height), list(plan.row_bytes)) == (1, [w, 0, 0], [h, 0, 0], [w * c * es, 0, 0])
                assert list(plan.coef) == list(planar.coef)
    assert sizes == {3, 4, 6, 8, 12, 16}
    if fmt == 3:                                                       # identity (GBR), 4:4:4 only
        desc = abi.make_export_desc(ref.RGB, 10, 2, 1, (0, 0, 0, 0), 0, 0)
        st, plan = plan_status(seq, desc, None, None, None, abi.make_export_pixel(abi.PIXEL_ABGR))
        assert st == OK and plan.row_bytes[0] == W * 8 and plan.coef[10] == 1


def test_refusals_of_the_pixel_description():
    seq = seq_of(1)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    d10 = abi.make_export_desc(ref.RGB, 10, 2, 1, (0, 0, 0, 0), 1, 0)
    f16 = abi.make_export_tensor(abi.SAMPLE_F16)

    def status(px, desc_=desc, tensor=None):
        st, plan = plan_status(seq, desc_, None, tensor, None, px)
        assert (st == OK) == (plan.planes == 1) and (st == OK or plan.planes == 0)
        return st

    assert status(None) == E                                            # pixel NULL
    for order in (-1, 6, 1 << 20):
        assert status(abi.make_export_pixel(order)) == E
    for k in range(5):
        px = abi.make_export_pixel(abi.PIXEL_RGB)
        px.reserved[k] = 1
        assert status(px) == E
    # alpha of unsigned elements: -1 .. 2^D - 1, D the output depth (8 here, 10 msb-aligned in u16 below)
    for order in (abi.PIXEL_RGBA, abi.PIXEL_BGRA, abi.PIXEL_ARGB, abi.PIXEL_ABGR):
        assert [status(abi.make_export_pixel(order, a)) for a in (-2, -1, 0, 128, 255, 256)] == [E, OK, OK, OK, OK, E]
        assert [status(abi.make_export_pixel(order, a), d10) for a in (-2, -1, 1023, 1024, 65535)] == [E, OK, OK, E, E]
        # float elements: alpha is not looked at, alpha_value must be finite
        assert [status(abi.make_export_pixel(order, 1 << 20, v), desc, f16) for v in (0.0, 1.0, -3.5, 1e30, math.inf, -math.inf, math.nan)] == \
               [OK, OK, OK, OK, E, E, E]
        assert status(abi.make_export_pixel(order, -1, math.nan)) == OK                      # unsigned: alpha_value is not looked at
    for order in (abi.PIXEL_RGB, abi.PIXEL_BGR):                         # three channels ignore both fields
        assert status(abi.make_export_pixel(order, 1 << 20, math.nan)) == OK
        assert status(abi.make_export_pixel(order, -7, math.inf), desc, f16) == OK


def test_inherited_refusals():
    """each refusal of the planar calls once, with its status: they come from the same plan functions"""
    seq = seq_of(1)
    px = abi.make_export_pixel(abi.PIXEL_RGBA)
    rgb = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    good = window_of(seq, (0, 0, 96, 40))

    def status(desc=rgb, scale=None, tensor=None, windows=None, n=None):
        st, plan = plan_status(seq, desc, scale, tensor, windows, px, n)
        assert st != OK and plan.planes == 0
        return st

    assert plan_status(seq, rgb, None, None, [good] * 16, px)[0] == OK
    for layout in (ref.PLANAR, ref.SEMIPLANAR):                           # a layout other than RGB
        assert status(abi.make_export_desc(layout, 8, 1, 0, (0, 0, 0, 0), 1, 0)) == E
        assert status(abi.make_export_desc(layout, 8, 1, 0, (0, 0, 0, 0), 1, 0), windows=[good]) == E
    assert status(abi.make_export_desc(3, 8, 1, 0, (0, 0, 0, 0), 1, 0)) == E                                  # (layout code 3)
    assert status(abi.make_export_desc(ref.RGB, 10, 2, 1, (0, 0, 0, 0), 1, 0), tensor=abi.make_export_tensor(abi.SAMPLE_F16)) == E   # msb_aligned floats
    assert status(scale=abi.make_export_scale(6, 2, abi.SCALE_BILINEAR), windows=[good, window_of(seq, (0, 0, 194, 40))]) == U       # beyond 32x
    assert status(abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 2, 0, 0), 1, 0), windows=[good]) == E           # desc->crop with windows
    assert status(abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 4, 0)) == U                            # a matrix the export does not have
    assert status(abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 0, 0)) == E                            # identity on 4:2:0
    assert status(windows=[good, window_of(seq, (0, 0, 94, 40))]) == E                                        # unscaled: two sizes
    assert status(windows=[good] * 17) == E and status(windows=[good], n=0) == E
    d = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    d.reserved[3] = 1
    assert status(d) == E
    t = abi.make_export_tensor(abi.SAMPLE_F32)
    t.reserved[0] = 1
    assert status(tensor=t) == E
    # the planar refusal comes first: a status of the plan (EUNSUPPORTED) is not hidden by a bad pixel description
    bad = abi.make_export_pixel(17)
    assert plan_status(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 4, 0), None, None, None, bad)[0] == U
    assert plan_status(seq, rgb, None, None, None, bad)[0] == E


def test_python_keywords():
    import torch
    px = export.make_pixel("bgra", None, None, "rgb", None, 4)
    assert (px.order, px.alpha) == (abi.PIXEL_BGRA, -1)
    px = export.make_pixel("ARGB", 100, None, "rgb", None, None)
    assert (px.order, px.alpha) == (abi.PIXEL_ARGB, 100)
    px = export.make_pixel("rgba", 0.25, None, "rgb", torch.float16, 4)
    assert (px.order, px.alpha_value) == (abi.PIXEL_RGBA, 0.25)
    assert export.make_pixel("rgba", None, None, "rgb", torch.float16, 4).alpha_value == 1.0
    px = export.make_pixel(None, None, torch.channels_last, "rgb", torch.float16, 4)
    assert px.order == abi.PIXEL_RGB and export.pixel_channels(px) == 3
    assert export.make_pixel(None, None, None, "planar", None, 4) is None
    for args in (("rgb", None, None, "planar", None, 4), ("rgbx", None, None, "rgb", None, 4), (None, 3, None, "rgb", None, 4),
                 (None, None, torch.channels_last, "nv12", None, 4), (None, None, torch.channels_last, "rgb", None, None),
                 ("rgb", None, torch.channels_last, "rgb", None, 4), (None, None, torch.contiguous_format, "rgb", None, 4),
                 ("rgba", 0.5, None, "rgb", None, 4)):
        with pytest.raises(ValueError):
            export.make_pixel(*args)
