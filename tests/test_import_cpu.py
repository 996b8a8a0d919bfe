"""The picture import without a device (include/hmgpu.h "picture import"): the structs against the header; the plans
hmgpu_import_plan_for reports; every refusal of the descriptor, with its status and in its order; the published RGB integers
against the derivation of tests/import_ref.py, their three required properties and the overflow bound; the model against the
existing export models (an import undoes an export); the float rule and the padding rule on cases worked by hand."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import export_batch_ref as bref
from tests import export_format_ref as fref
from tests import export_ref as eref
from tests import import_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
PLANAR, SEMI, RGB = abi.EXPORT_PLANAR, abi.EXPORT_SEMIPLANAR, abi.EXPORT_RGB
MATRICES = (1, 5, 6, 9)


def _seq(fmt=1, w=72, h=40, bd=8, bdc=None):
    s = abi.make_seq(w, h, bd, bdc)
    s.chroma_format = fmt
    return s


def _status(seq, desc, want=OK):
    plan = abi.ImportPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    st = libhm_amd.lib().hmgpu_import_plan_for(C.byref(seq), abi.ref(desc), C.byref(plan))
    assert st == want, "status %d, expected %d" % (st, want)
    if want != OK:
        assert bytes(plan) == bytes(C.sizeof(plan)), "a refused plan must be all zero"
    return plan


# ------------------------------------------------------------------------------------------------ the structs
def test_structs_match_the_header(tmp_path):
    fields = ["layout", "order", "width", "height", "bit_depth", "bytes_per_sample", "msb_aligned", "sample_type", "scale", "bias",
              "chroma_format", "down", "loc", "matrix", "full_range", "reserved"]
    pfields = ["planes", "width", "height", "row_bytes", "coef"]
    src = tmp_path / "imp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu", sizeof(hmgpu_import_desc), '
                   'sizeof(hmgpu_import_plan));\n'
                   + "".join('printf(" %%zu", offsetof(hmgpu_import_desc, %s));\n' % f for f in fields)
                   + "".join('printf(" %%zu", offsetof(hmgpu_import_plan, %s));\n' % f for f in pfields)
                   + 'printf("\\n");return 0;}\n')
    exe = tmp_path / "imp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    D, P = abi.ImportDesc, abi.ImportPlan
    assert got == [C.sizeof(D), C.sizeof(P)] + [getattr(D, f).offset for f in fields] + [getattr(P, f).offset for f in pfields]
    d = abi.make_import_desc(RGB, abi.PIXEL_BGRA, (70, 38), 10, 2, 0, abi.SAMPLE_F16, (2, 3, 4), (5, 6, 7), "422", "linear", 3, 9, 1)
    assert (d.layout, d.order, d.width, d.height, list(d.bit_depth), d.bytes_per_sample, d.msb_aligned, d.sample_type, list(d.scale),
            list(d.bias), d.chroma_format, d.down, d.loc, d.matrix, d.full_range, list(d.reserved)) == \
        (2, 3, 70, 38, [10, 10], 2, 0, 1, [2, 3, 4], [5, 6, 7], 2, 1, 3, 9, 1, [0] * 8)


# ------------------------------------------------------------------------------------------------ the plans
@pytest.mark.parametrize("pic_fmt", (0, 1, 2, 3))
def test_plans_of_the_yuv_layouts(pic_fmt):
    for layout, src_fmt, depth, size in itertools.product((PLANAR, SEMI), (0, 1, 2, 3), (1, 8, 10, 16), ((0, 0), (68, 36))):
        nbytes = 2 if depth > 8 else 1
        plan = _status(_seq(pic_fmt, bd=8), abi.make_import_desc(layout, size=size, bit_depth=depth, bytes_per_sample=nbytes,
                                                                 chroma_format=src_fmt))
        w, h = size if size[0] else (72, 40)
        sx, sy = iref.shifts(src_fmt) if src_fmt else (0, 0)
        planes = 1 if src_fmt == 0 or pic_fmt == 0 else 3 if layout == PLANAR else 2
        assert plan.planes == planes and list(plan.coef) == [0] * 16
        want = [(w, h, w * nbytes)] + [(w >> sx, h >> sy, (1 if layout == PLANAR else 2) * (w >> sx) * nbytes)] * (planes - 1)
        want += [(0, 0, 0)] * (3 - planes)
        assert [(plan.width[k], plan.height[k], plan.row_bytes[k]) for k in range(3)] == want


def test_plans_of_the_rgb_layout():
    for pic_fmt, order, (stype, es, nbytes, depth) in itertools.product(
            (0, 1, 2, 3), range(-1, 6),
            ((abi.SAMPLE_UINT, 1, 1, 8), (abi.SAMPLE_UINT, 2, 2, 12), (abi.SAMPLE_F16, 2, 1, 8), (abi.SAMPLE_BF16, 2, 2, 10),
             (abi.SAMPLE_F32, 4, 2, 16))):
        plan = _status(_seq(pic_fmt), abi.make_import_desc(RGB, order, (70, 38), depth, nbytes, 0, stype))
        nch = 0 if order < 0 else iref.PIXEL_POS[order][1]
        assert plan.planes == (1 if nch else 3)
        for k in range(3):
            want = (70, 38, 70 * max(nch, 1) * es) if k < plan.planes else (0, 0, 0)
            assert (plan.width[k], plan.height[k], plan.row_bytes[k]) == want


# ------------------------------------------------------------------------------------------------ the refusals and their order
def _desc(**kw):
    base = dict(layout=PLANAR, bit_depth=8, bytes_per_sample=1)
    base.update(kw)
    return abi.make_import_desc(**base)


def test_refusals_of_the_descriptor():
    seq = _seq(1)
    plan = abi.ImportPlan()
    assert libhm_amd.lib().hmgpu_import_plan_for(C.byref(seq), None, C.byref(plan)) == EINVAL
    assert libhm_amd.lib().hmgpu_import_plan_for(None, C.byref(_desc()), C.byref(plan)) == EINVAL
    assert libhm_amd.lib().hmgpu_import_plan_for(C.byref(seq), C.byref(_desc()), None) == EINVAL
    _status(seq, _desc())
    for k in range(8):
        d = _desc()
        d.reserved[k] = 1
        _status(seq, d, EINVAL)
    for kw in (dict(layout=-1), dict(layout=3), dict(order=0), dict(layout=SEMI, order=2), dict(layout=RGB, order=-2),
               dict(layout=RGB, order=6), dict(chroma_format=-1), dict(chroma_format=4),
               dict(bit_depth=(-1, 8)), dict(bit_depth=(8, 17), bytes_per_sample=2), dict(bit_depth=(9, 8)), dict(bit_depth=(8, 9)),
               dict(bytes_per_sample=0), dict(bytes_per_sample=3), dict(bytes_per_sample=4), dict(msb_aligned=2), dict(msb_aligned=1),
               dict(sample_type=abi.SAMPLE_F32, bytes_per_sample=2, msb_aligned=1),
               dict(sample_type=abi.SAMPLE_F16, bytes_per_sample=2),                    # the container the depths need is 1
               dict(sample_type=abi.SAMPLE_F16, bit_depth=10, bytes_per_sample=1),
               dict(sample_type=abi.SAMPLE_F32, scale=(1, float("inf"), 1)), dict(sample_type=abi.SAMPLE_F32, bias=(float("nan"), 0, 0)),
               dict(size=(-2, 0)), dict(size=(74, 40)), dict(size=(72, 42)), dict(size=(71, 40)), dict(size=(72, 39)),
               dict(chroma_format=3, size=(71, 40)), dict(chroma_format=2, size=(72, 39)),
               dict(loc=-1), dict(loc=6),
               dict(layout=RGB, full_range=2), dict(layout=RGB, matrix=0)):
        _status(seq, _desc(**kw), EINVAL)
    # a 4:4:4 picture from a 4:4:4 source takes odd sizes; matrix 0 belongs to it; a non-finite scale is not looked at for integers
    s444 = _seq(3)
    _status(s444, _desc(chroma_format=3, size=(71, 39)))
    _status(s444, _desc(chroma_format=1, size=(71, 39)), EINVAL)
    _status(s444, _desc(layout=RGB, matrix=0))
    _status(seq, _desc(scale=(float("inf"), 1, 1)))
    # a 4:0:0 picture does not look at the chroma depth
    _status(_seq(0), _desc(bit_depth=(8, 99)))
    _status(seq, _desc(chroma_format=0, bit_depth=(8, 99)), EINVAL)       # ... a 4:0:0 source into a picture with chroma does (1 << (D - 1))
    for kw in (dict(layout=RGB, matrix=2), dict(layout=RGB, matrix=4), dict(layout=RGB, matrix=10), dict(down=2), dict(down=-1),
               dict(sample_type=4), dict(sample_type=-1, bytes_per_sample=1), dict(layout=SEMI, sample_type=abi.SAMPLE_F16)):
        _status(seq, _desc(**kw), EUNSUPPORTED)
    _status(seq, _desc(matrix=77))                                         # (the YUV layouts do not look at the matrix)


def test_refusals_come_in_their_order():
    """a descriptor with one fault of step 1 (EINVAL) and one of step 2 (EUNSUPPORTED) is refused for the first"""
    seq = _seq(1)
    for bad2 in (dict(down=5), dict(sample_type=9), dict(layout=RGB, matrix=3)):
        for bad1 in (dict(size=(71, 40)), dict(loc=7), dict(bit_depth=(17, 17))):
            _status(seq, _desc(**dict(bad2, **bad1)), EINVAL)
        _status(seq, _desc(**bad2), EUNSUPPORTED)
    d = _desc(layout=SEMI, sample_type=abi.SAMPLE_F16)
    d.reserved[7] = 5
    _status(seq, d, EINVAL)


# ------------------------------------------------------------------------------------------------ RGB: the integers and what they promise
DEPTH_PAIRS = [(d, bdy, bdc) for d in range(1, 17) for bdy, bdc in ((8, 8), (9, 9), (10, 10), (11, 11), (12, 12), (8, 12), (12, 8), (10, 8))]


def _coef(depth, bdy, bdc, matrix, full_range):
    d = abi.make_import_desc(RGB, bit_depth=depth, bytes_per_sample=2 if depth > 8 else 1, matrix=matrix, full_range=full_range)
    return list(_status(_seq(3, bd=bdy, bdc=bdc), d).coef)


@pytest.fixture(scope="module")
def all_coefs():
    return {(d, y, c, m, f): _coef(d, y, c, m, f) for (d, y, c) in DEPTH_PAIRS for m in MATRICES for f in (0, 1)}


def test_published_coefficients_are_the_models(all_coefs):
    for (d, y, c, m, f), coef in all_coefs.items():
        assert coef == iref.rgb_coef(d, (y, c), m, f), (d, y, c, m, f)
        assert coef[13] == (1 << d) - 1 and coef[14] == 0 and coef[15] == 0
    assert _coef(10, 8, 8, 0, 0) == [0] * 13 + [1023, 1, 0]
    assert all_coefs[(8, 8, 8, 5, 0)] == all_coefs[(8, 8, 8, 6, 0)]


def test_no_sum_overflows_and_the_shift_is_the_largest(all_coefs):
    for (d, y, c, m, f), coef in all_coefs.items():
        s = coef[0]
        assert 17 <= s <= 30 and coef[1] == 1 << (s - 1)
        assert iref.overflow_bound(coef[4:13], d, s) <= 2 ** 31 - 1
        if s < 30:
            rows = iref.rgb_rows(d, (y, c), m, f, s + 1)[0]
            assert iref.overflow_bound(rows, d, s + 1) > 2 ** 31 - 1
        # the sums the rows can reach, evaluated at the corners of the cube, where a linear form has its extremes
        mx = (1 << d) - 1
        for row in (coef[4:7], coef[7:10], coef[10:13]):
            for r, g, b in itertools.product((0, mx), repeat=3):
                assert abs(row[0] * r + row[1] * g + row[2] * b + coef[1]) <= 2 ** 31 - 1


def test_grey_gives_mid_chroma_black_and_white_the_end_points(all_coefs):
    for (d, y, c, m, f), coef in all_coefs.items():
        mx = (1 << d) - 1
        v = np.unique(np.concatenate([np.arange(min(mx + 1, 4096)), np.linspace(0, mx, 4096).astype(np.int64), [mx]]))
        Y, cb, cr = iref.rgb_to_ycc(v, v, v, coef, d, (y, c))
        assert np.all(cb == 1 << (c - 1)) and np.all(cr == 1 << (c - 1)), (d, y, c, m, f)
        lo, hi = (0, (1 << y) - 1) if f else (16 << (y - 8), 235 << (y - 8))
        assert (Y[0], Y[-1]) == (lo, hi), (d, y, c, m, f)
        assert np.all(np.diff(Y) >= 0)


def test_luma_never_falls_when_a_colour_rises_all_of_8_bits(all_coefs):
    ax = np.arange(256, dtype=np.int32)
    for (d, y, c, m, f), coef in all_coefs.items():
        if d != 8 or y != c or m == 5:
            continue
        assert min(coef[4:7]) >= 0
        t = (coef[4] * ax)[:, None, None] + (coef[5] * ax)[None, :, None] + (coef[6] * ax)[None, None, :] + np.int32(coef[1])
        Y = np.clip((t >> coef[0]) + coef[2], 0, (1 << y) - 1)
        for axis in range(3):
            assert np.all(np.diff(Y, axis=axis) >= 0), (y, m, f, axis)


def test_luma_never_falls_at_the_extremes_and_on_a_sample_above_8_bits(all_coefs):
    rng = np.random.default_rng(11)
    for (d, y, c, m, f), coef in all_coefs.items():
        if d <= 8:
            continue
        mx = (1 << d) - 1
        base = rng.integers(0, mx + 1, (3, 4000))
        base[:, :64] = np.array(list(itertools.product((0, 1, mx - 1, mx), repeat=3))).T        # every corner and its neighbours
        for k in range(3):
            up = base.copy()
            up[k] = np.minimum(up[k] + 1, mx)
            far = base.copy()
            far[k] = mx
            y0 = iref.rgb_to_ycc(*base, coef, d, (y, c))[0]
            assert np.all(iref.rgb_to_ycc(*up, coef, d, (y, c))[0] >= y0) and np.all(iref.rgb_to_ycc(*far, coef, d, (y, c))[0] >= y0)


# ------------------------------------------------------------------------------------------------ an import undoes an export
def _planes(fmt, w, h, bd, seed):
    rng = np.random.default_rng(seed)
    p = [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)]
    if fmt:
        sx, sy = iref.shifts(fmt)
        p += [rng.integers(0, 1 << bd[1], (h >> sy, w >> sx)).astype(np.int16) for _ in range(2)]
    return p


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt", (0, 1, 2, 3))
@pytest.mark.parametrize("layout", (PLANAR, SEMI))
def test_import_of_an_export_is_the_picture(fmt, layout):
    for bd, out_bd, msb in (((8, 8), (8, 8), False), ((10, 10), (10, 10), False), ((10, 9), (10, 9), True), ((8, 8), (8, 8), True),
                            ((8, 10), (12, 16), True), ((9, 9), (16, 16), False)):
        p = _planes(fmt, 24, 16, bd, 5)
        out = eref.export_yuv(p, fmt, bd, out_bd, layout, msb=msb)
        if fmt and layout == SEMI:
            out = [out[0], out[1][..., 0], out[1][..., 1]]
        codes = [iref.uint_codes(v, out_bd[1 if k else 0], msb) for k, v in enumerate(out)]
        assert _same(iref.import_yuv(codes, fmt, fmt, out_bd, bd, (24, 16)), p)


@pytest.mark.parametrize("fmt", (1, 2))
def test_replicate_then_drop_returns_the_planes(fmt):
    p = _planes(fmt, 24, 16, (10, 10), 6)
    up = fref.convert_planes(p, fmt, 3, up=fref.REPLICATE, depth_chroma=10)
    for loc in range(6):
        assert _same(iref.import_yuv(up, 3, fmt, (10, 10), (10, 10), (24, 16), iref.DROP, loc), p)
    mid = fref.convert_planes(p, 1, 2, up=fref.REPLICATE, depth_chroma=10) if fmt == 1 else None
    if mid is not None:
        assert _same(iref.import_yuv(mid, 2, 1, (10, 10), (10, 10), (24, 16)), p)


def test_linear_decimation_is_the_format_exports():
    """the picture's format stands where the format export has the output's: same taps, same clamping"""
    for src, pic in ((3, 1), (3, 2), (2, 1)):
        p = _planes(src, 24, 16, (8, 8), 7)
        for loc in range(6):
            want = fref.convert_planes(p, src, pic, down=1, loc=loc, depth_chroma=8)
            assert _same(iref.import_yuv(p, src, pic, (8, 8), (8, 8), (24, 16), iref.LINEAR, loc), [np.asarray(v, np.int16) for v in want])


@pytest.mark.parametrize("fmt", (0, 1, 3))
def test_float32_import_of_the_float32_export(fmt):
    bd = (10, 9)
    p = _planes(fmt, 24, 16, bd, 8)
    seq = _seq(fmt, 24, 16, bd[0], bd[1])
    desc = abi.make_export_desc(PLANAR, (0, 0), 2)
    tensor = abi.make_export_tensor(abi.SAMPLE_F32)
    floats = [b.view(np.float32) for b in bref.export_batch_ref(seq, p, fmt, bd, desc, None, tensor)]
    codes = [iref.float_codes(v, 1.0, 0.0, bd[1 if k else 0]) for k, v in enumerate(floats)]
    assert _same(iref.import_yuv(codes, fmt, fmt, bd, bd, (24, 16)), p)
    # ... and through the normalised form: the inverse affine map lands on the integer again
    from libhm_amd import export as hexport, imports
    sc, bi = hexport.affine(bd, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    isc, ibi = imports.inverse_affine(bd, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    for k, v in enumerate(p):
        f = bref.affine_f32(v, sc[k], bi[k])
        assert np.array_equal(iref.float_codes(f, isc[k], ibi[k], bd[1 if k else 0]), v)


# ------------------------------------------------------------------------------------------------ the float rule
def test_float_rule_on_a_table():
    f32 = np.float32
    den = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]                    # the smallest denormal
    table = [  # x, scale, bias, depth, v
        (0.5, 1, 0, 8, 0), (1.5, 1, 0, 8, 2), (2.5, 1, 0, 8, 2), (3.5, 1, 0, 8, 4), (254.5, 1, 0, 8, 254), (255.5, 1, 0, 8, 255),
        (-0.5, 1, 0, 8, 0), (-1.0, 1, 0, 8, 0), (-1e30, 1, 0, 8, 0), (256.0, 1, 0, 8, 255), (1e30, 1, 0, 8, 255),
        (float("nan"), 1, 0, 8, 0), (float("inf"), 1, 0, 8, 255), (float("-inf"), 1, 0, 8, 0), (float("inf"), 1, 0, 16, 65535),
        (den, 1, 0, 8, 0), (-den, 1, 0, 8, 0), (den, 1, 0.5, 8, 0), (den, 1, 1.5, 8, 2),
        (1.0, 255, 0, 8, 255), (0.5, 255, 0, 8, 128), (0.1, 1023, 0, 10, 102), (1.0, 65535, 0, 16, 65535), (0.5, 65535, 0, 16, 32768),
        (1e38, 10.0, -1e38, 8, 255),                                              # the product overflows to infinity first
        (2.0, 0.25, 0.0, 1, 0), (2.0, 0.75, 0.0, 1, 1), (6.0, 0.25, 0.0, 1, 1),
    ]
    for x, s, b, d, v in table:
        got = int(iref.float_codes(np.array([x], f32), f32(s), f32(b), d)[0])
        assert got == v, (x, s, b, d, got, v)
    # two roundings, never one fma: x * scale = N + 0.5 exactly with N = 2^23 + 2^13 + 1 odd, so the product rounds to N + 1 and the sum
    # with -N is 1; a fused multiply-add would keep the 0.5, which rint takes to 0
    x, s, b = f32(2.0 ** 23 + 2.0 ** 11), f32(1 + 3 * 2.0 ** -12), f32(-(2.0 ** 23 + 2.0 ** 13 + 1))
    assert float(x) * float(s) + float(b) == 0.5
    assert int(iref.float_codes(np.array([x], f32), s, b, 8)[0]) == 1
    # float16 and bfloat16 elements are float32 values exactly
    h = np.array([0.5, 1.5, 65504.0, 6e-8], np.float16).astype(np.float32)
    assert list(iref.float_codes(h, 1.0, 0.0, 16)) == [0, 2, 65504, 0]


# ------------------------------------------------------------------------------------------------ the padding rule
def test_padding_of_a_70x38_source_in_a_72x40_picture():
    src = _planes(1, 70, 38, (8, 8), 9)
    got = iref.import_yuv(src, 1, 1, (8, 8), (8, 8), (72, 40))
    assert [g.shape for g in got] == [(40, 72), (20, 36), (20, 36)]
    for g, s in zip(got, src):
        h, w = s.shape
        assert np.array_equal(g[:h, :w], s)
        assert np.array_equal(g[:h, w:], np.repeat(s[:, -1:], g.shape[1] - w, axis=1))              # the last column, :333-338
        assert np.array_equal(g[h:, :], np.repeat(g[h - 1:h, :], g.shape[0] - h, axis=0))           # then the last row, :340-345
    # the converted plane is padded, not the source: 4:4:4 -> 4:2:0 LINEAR repeats the last decimated column
    s444 = _planes(3, 70, 38, (8, 8), 10)
    g = iref.import_yuv(s444, 3, 1, (8, 8), (8, 8), (72, 40), iref.LINEAR, 0)
    conv = iref.convert_chroma(s444[1], 0, 0, 1, 1, 1, iref.LINEAR, 0)
    assert conv.shape == (19, 35) and np.array_equal(g[1][:19, :35], conv) and np.all(g[1][:19, 35] == conv[:, 34]) and \
        np.array_equal(g[1][19], g[1][18])
    # RGB: chroma is formed at every pixel of the source, decimated, then padded
    rng = np.random.default_rng(12)
    r, gg, b = rng.integers(0, 256, (3, 38, 70))
    out = iref.import_rgb(r, gg, b, 1, 8, (8, 8), (72, 40), 1, 0, iref.LINEAR, 1)
    y, cb, cr = iref.rgb_to_ycc(r, gg, b, iref.rgb_coef(8, (8, 8), 1, 0), 8, (8, 8))
    assert np.array_equal(out[0][:38, :70], y) and np.all(out[0][:, 71] == out[0][:, 69])
    assert np.array_equal(out[2][:19, :35], iref.convert_chroma(cr, 0, 0, 1, 1, 1, iref.LINEAR, 1))
