"""Device export, host side (no GPU): hmgpu_export_plan_for's validation and geometry, the published RGB integers against H.273's
floating-point equations, the numpy restatement of the YUV bit-depth rule against HM's own `TAppDecoder -d N` files, and the VUI
colour description the parser now keeps."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_ref as ref
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HM_D = ["d8_ldp_main10_208x120", "d8_ldb_main12_208x120", "d10_ldb_main12_208x120", "d10_ldp_main8_416x240", "d16_ldp_main8_416x240",
        "d8_ldb_422_main10_208x120", "d8_intra_444_ccp_main10_208x120", "d10_ldp_crop_main8_204x116", "d8_ldb_mono_wp_crop_main10_204x116"]


def seq_of(w, h, fmt, bd_y, bd_c=None):
    s = abi.make_seq(w, h, bd_y, bd_c if bd_c is not None else bd_y)
    s.chroma_format = fmt
    return s


def plan_status(seq, desc):
    plan = abi.ExportPlan()
    st = libhm_amd.lib().hmgpu_export_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    return st, plan


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ref.PLANAR, ref.SEMIPLANAR, ref.RGB])
@pytest.mark.parametrize("crop", [(0, 0, 0, 0), (4, 8, 2, 6), (0, 12, 0, 4)])
@pytest.mark.parametrize("nbytes", [1, 2])
def test_plan_geometry(fmt, layout, crop, nbytes):
    w, h = 208, 120
    seq = seq_of(w, h, fmt, 10)
    desc = abi.make_export_desc(layout, (8 if nbytes == 1 else 10), nbytes, 0, crop, 1, 0)
    st, plan = plan_status(seq, desc)
    assert st == abi.HMGPU_OK
    planes = ref.export_yuv([np.zeros((h, w), np.int16)] + [np.zeros((h >> ref.chroma_shift(fmt)[1], w >> ref.chroma_shift(fmt)[0]), np.int16)] * 2,
                            fmt, (10, 10), (10, 10), layout, crop) if layout != ref.RGB else list(np.zeros((3, h - crop[2] - crop[3], w - crop[0] - crop[1])))
    assert plan.planes == len(planes)
    for k, p in enumerate(planes):
        assert (plan.height[k], plan.width[k]) == p.shape[:2]
        assert plan.row_bytes[k] == p.shape[1] * (p.shape[2] if p.ndim == 3 else 1) * nbytes
    assert all(v == 0 for v in plan.coef) == (layout != ref.RGB)


def test_plan_rejects_bad_descriptors():
    s420, s444, s400 = seq_of(208, 120, 1, 10), seq_of(208, 120, 3, 8), seq_of(208, 120, 0, 10)
    E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    mk = abi.make_export_desc
    assert plan_status(s420, mk(ref.PLANAR, 8, 1, crop=(1, 0, 0, 0)))[0] == E          # odd chroma crop
    assert plan_status(s420, mk(ref.PLANAR, 8, 1, crop=(0, 0, 0, 3)))[0] == E
    assert plan_status(seq_of(208, 120, 2, 8), mk(ref.PLANAR, 8, 1, crop=(0, 0, 0, 3)))[0] == abi.HMGPU_OK   # 4:2:2: rows are whole
    assert plan_status(s400, mk(ref.PLANAR, 8, 1, crop=(1, 0, 3, 0)))[0] == abi.HMGPU_OK                      # 4:0:0: no chroma
    assert plan_status(s420, mk(ref.PLANAR, 10, 1))[0] == E                              # 1-byte samples above 8 bits
    assert plan_status(s420, mk(ref.RGB, 10, 1))[0] == E
    assert plan_status(s420, mk(ref.PLANAR, 0, 1))[0] == E                               # (0 = coding depth = 10)
    assert plan_status(s420, mk(ref.PLANAR, 8, 1, msb_aligned=1))[0] == E                # msb_aligned with 1 byte
    assert plan_status(s420, mk(ref.RGB, 8, 1, matrix=0))[0] == E                        # identity on 4:2:0
    assert plan_status(s400, mk(ref.RGB, 8, 1, matrix=0))[0] == E
    assert plan_status(s444, mk(ref.RGB, 8, 1, matrix=0))[0] == abi.HMGPU_OK
    for m in (2, 3, 4, 7, 8, 10, 14, 255):                                                 # unknown / unimplemented matrix codes
        assert plan_status(s420, mk(ref.RGB, 8, 1, matrix=m))[0] == U
    assert plan_status(s420, mk(3, 8, 1))[0] == E                                        # layout
    assert plan_status(s420, mk(ref.PLANAR, 8, 3))[0] == E                               # bytes per sample
    assert plan_status(s420, mk(ref.PLANAR, 17, 2))[0] == E
    assert plan_status(s420, mk(ref.PLANAR, 8, 1, crop=(104, 104, 0, 0)))[0] == E        # nothing left
    d = mk(ref.PLANAR, 8, 1)
    d.reserved[2] = 1
    assert plan_status(s420, d)[0] == E


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu\\n",sizeof(hmgpu_export_desc),'
                   'sizeof(hmgpu_export_plan));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(v) for v in subprocess.check_output([str(exe)], text=True).split()] == [C.sizeof(abi.ExportDesc), C.sizeof(abi.ExportPlan)]


def _source_planes(fixture):
    """native-depth planes per POC of the fixture a -d N file was made from (HM's decoder output, uncropped, or the cropped
    encoder reconstruction of a lite fixture) and the conformance window still to apply"""
    if fixture.startswith("stream_"):
        return {p.poc: list(p.fin) for p in gu.stream_pictures(fixture[7:])}, (0, 0, 0, 0)
    z = gu.load(fixture)
    out = {}
    for poc in range(int(z["geom"][2])):
        out[poc] = [z["poc%02d_%d" % (poc, c)] for c in range(3) if ("poc%02d_%d" % (poc, c)) in z]
    return out, (0, 0, 0, 0)


@pytest.mark.parametrize("name", HM_D)
def test_yuv_rule_reproduces_hm_d_files(name):
    g = gu.load("export_" + name)
    w, h, fmt, frames, out_bd = (int(v) for v in g["geom"])
    src, crop = _source_planes(str(g["source"]))
    bd = {"main8": (8, 8), "main10": (10, 10), "main12": (12, 12)}[[t for t in name.split("_") if t.startswith("main")][0]]
    assert sorted(src) == list(range(frames))
    for poc in range(frames):
        planes = src[poc]
        if fmt == 0:
            planes = planes[:1] + [np.zeros((1, 1), np.int16)] * 2
        got = ref.export_yuv(planes, fmt, bd, (out_bd, out_bd), ref.PLANAR, crop)
        for c in range(1 if fmt == 0 else 3):
            want = g["poc%02d_%d" % (poc, c)]
            assert got[c].shape == want.shape
            assert np.array_equal(got[c], want.astype(np.int64)), (name, poc, c)


MATRICES = [(1, 0), (1, 1), (5, 0), (5, 1), (9, 0), (9, 1)]


def _plan_rgb(bd_y, bd_c, out_bd, matrix, full):
    st, plan = plan_status(seq_of(64, 64, 1, bd_y, bd_c), abi.make_export_desc(ref.RGB, out_bd, 1 if out_bd <= 8 else 2, 0, (0, 0, 0, 0), matrix, full))
    assert st == abi.HMGPU_OK
    return list(plan.coef)


def _check_close(y, u, v, bd_y, bd_c, out_bd, matrix, full):
    coef = _plan_rgb(bd_y, bd_c, out_bd, matrix, full)
    got, sums = ref.rgb_int(y, u, v, coef)
    assert np.abs(sums).max() < 2 ** 31
    want = np.clip(ref.rgb_float(y, u, v, bd_y, bd_c, out_bd, matrix, full), 0, (1 << out_bd) - 1)
    err = np.abs(got - want)
    assert err.max() <= 1.0, (matrix, full, bd_y, out_bd, err.max())


@pytest.mark.parametrize("matrix,full", MATRICES)
def test_rgb_integers_exhaustive_8bit(matrix, full):
    """every (Y, Cb, Cr) triple at 8 bits, out 8 bits: within one code value of H.273's equations"""
    y = np.arange(256, dtype=np.int64)
    for u0 in range(0, 256, 64):
        yy, uu, vv = np.meshgrid(y, np.arange(u0, u0 + 64), y, indexing="ij")
        _check_close(yy.ravel(), uu.ravel(), vv.ravel(), 8, 8, 8, matrix, full)


@pytest.mark.parametrize("bd", [10, 12])
@pytest.mark.parametrize("matrix,full", MATRICES)
def test_rgb_integers_random_high_bit_depth(bd, matrix, full):
    rng = np.random.default_rng(bd * 100 + matrix * 2 + full)
    y, u, v = (rng.integers(0, 1 << bd, 10 ** 6) for _ in range(3))
    for out_bd in (8, 10):
        _check_close(y, u, v, bd, bd, out_bd, matrix, full)


def test_rgb_integers_never_overflow():
    """the extremes of every coding depth pair against every output depth: each partial sum stays inside int32"""
    for bd_y, bd_c, out_bd, (matrix, full) in itertools.product(range(8, 13), range(8, 13), range(8, 17), MATRICES):
        coef = _plan_rgb(bd_y, bd_c, out_bd, matrix, full)
        ext_y, ext_c = [0, (1 << bd_y) - 1], [0, (1 << bd_c) - 1]
        y, u, v = (np.array(a) for a in zip(*itertools.product(ext_y, ext_c, ext_c)))
        S, rnd, yo, co, cy, crv, cgu, cgv, cbu = coef[:9]
        t = cy * (y - yo) + rnd
        for part in (t, t + crv * (v - co), t + cgu * (u - co), t + cgu * (u - co) + cgv * (v - co), t + cbu * (u - co)):
            assert np.abs(part).max() < 2 ** 31, (bd_y, bd_c, out_bd, matrix, full)
        assert 1 <= S <= 30


def _colours(bitstream):
    out = []
    with hmdec.Decoder(parse_only=True) as d:
        d.decode_stream(bitstream, on_decoded=lambda p: out.append(p.colour()))
    assert out
    return out


def test_vui_colour_description():
    for c in _colours(gu.load("export_vui_bt2020_main10_208x120")["bitstream"]):
        assert (c["full_range"], c["primaries"], c["transfer"], c["matrix"], c["video_format"]) == (1, 9, 16, 9, 5)


@pytest.mark.parametrize("fixture", ["lite_ldp_cqp_vui_main10_208x120", "stream_ldp_main8_416x240"])
def test_vui_defaults(fixture):
    """a VUI without video_signal_type, and no VUI at all: E.3.1's defaults"""
    for c in _colours(gu.load(fixture)["bitstream"]):
        assert (c["full_range"], c["primaries"], c["transfer"], c["matrix"], c["video_format"]) == (0, 2, 2, 2, 5)


def test_colour_policy():
    from libhm_amd import export
    assert export.resolve_colour(None, None, 2, 0) == (1, 0)
    assert export.resolve_colour(None, None, 9, 1) == (9, 1)
    assert export.resolve_colour(5, 1, 9, 0) == (5, 1)
    assert export.torch_dtype(1).itemsize == 1 and export.torch_dtype(2).itemsize == 2
