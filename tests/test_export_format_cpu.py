"""The format export without a device (include/hmgpu.h "format export"): the numpy model of tests/export_format_ref.py on cases
worked by hand, against TVideoIOYuv::writePlane's index arithmetic and against tests/export_chroma_ref.py; the struct against the
header; every refusal of hmgpu_export_format_plan_for and the order they come in; the plans it reports.

One place where the export and writePlane part, found while transcribing writePlane literally: where the file has more chroma rows
than the source (4:2:0 -> 4:2:2 / 4:4:4) writePlane's row pointer advances after rows with (y444 & mask_y_src) == 0, so file row y
reads source row (y + 1) >> 1 and the last row reads one row below the plane.  The export reads y >> 1 there, the rule it has on
the horizontal axis and the one the RGB exports replicate by.  test_drop_and_replicate_are_writeplane pins both statements for
those two pairs and plain equality for the other fourteen."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import export_chroma_ref as chref
from tests import export_format_ref as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
FORMATS = (0, 1, 2, 3)
PAIRS = [(s, o) for s in FORMATS for o in FORMATS]
CHROMA_PAIRS = [(s, o) for s in (1, 2, 3) for o in (1, 2, 3) if s != o]


def plane_shape(fmt, w=16, h=12):
    sx, sy = fref.shifts(fmt)
    return h >> sy, w >> sx


# ------------------------------------------------------------------------------------------------ the model, by hand
# the response of one axis to a single source sample of value 16 at index i, as {output index: weight}
def up_response(site, i):
    return {fref.COSITED: {2 * i - 1: 2, 2 * i: 4, 2 * i + 1: 2},
            fref.CENTRED: {2 * i - 1: 1, 2 * i: 3, 2 * i + 1: 3, 2 * i + 2: 1},
            fref.BOTTOM: {2 * i: 2, 2 * i + 1: 4, 2 * i + 2: 2}}[site]


def down_response(site, i):
    m, odd = i >> 1, i & 1
    return {fref.COSITED: {m: 1, m + 1: 1} if odd else {m: 2},
            fref.CENTRED: {m: 2},
            fref.BOTTOM: {m: 2} if odd else {m - 1: 1, m: 1}}[site]


def dense(resp, n):
    v = np.zeros(n, np.int64)
    for k, w in resp.items():
        v[k] = w
    return v


@pytest.mark.parametrize("loc", range(6))
def test_every_weight_product_of_every_siting(loc):
    """an isolated sample of 16 in the middle of a plane of zeros comes out as wx * wy: all products of all sitings, both directions,
    at both parities of the sample's position"""
    for src, out in CHROMA_PAIRS:
        hc, wc = plane_shape(src)
        (gx, _, hs), (gy, _, vs) = fref.conversion(src, out, fref.LINEAR, fref.LINEAR, loc)
        for iy in (2, 3):
            for ix in (2, 3):
                c = np.zeros((hc, wc), np.int64)
                c[iy, ix] = 16
                got = fref.convert_plane(c, src, out, fref.LINEAR, fref.LINEAR, loc)
                oh, ow = plane_shape(out)
                assert got.shape == (oh, ow)
                rx = dense(up_response(hs, ix) if gx > 0 else down_response(hs, ix), ow) if gx else dense({ix: 4}, ow)
                ry = dense(up_response(vs, iy) if gy > 0 else down_response(vs, iy), oh) if gy else dense({iy: 4}, oh)
                assert np.array_equal(got, np.outer(ry, rx)), (src, out, loc, iy, ix)


def test_sitings_by_loc():
    assert [fref.siting(True, k) for k in range(6)] == [
        (fref.COSITED, fref.CENTRED), (fref.CENTRED, fref.CENTRED), (fref.COSITED, fref.COSITED), (fref.CENTRED, fref.COSITED),
        (fref.COSITED, fref.BOTTOM), (fref.CENTRED, fref.BOTTOM)]
    assert all(fref.siting(False, k) == (fref.COSITED, None) for k in range(6))     # 4:2:2: co-sited, loc ignored
    # the 4:2:0 side decides: 4:4:4 -> 4:2:2 and 4:2:2 -> 4:4:4 are co-sited whatever loc says, 4:2:2 <-> 4:2:0 converts rows only
    assert fref.conversion(3, 2, 1, 1, 5) == ((-1, 1, fref.COSITED), (0, 1, None))
    assert fref.conversion(2, 3, 1, 1, 5) == ((1, 1, fref.COSITED), (0, 1, None))
    assert fref.conversion(2, 1, 1, 1, 5)[1] == (-1, 1, fref.BOTTOM) and fref.conversion(1, 2, 1, 1, 2)[1] == (1, 1, fref.COSITED)


def test_rounding_is_half_up_after_the_sum():
    """4:4:4 -> 4:2:0 at loc 1 (centred on both axes) is (a + b + c + d + 2) >> 2 of each 2 x 2 block"""
    blocks = {(0, 0, 0, 0): 0, (1, 0, 0, 0): 0, (1, 1, 0, 0): 1, (1, 1, 1, 0): 1, (1, 1, 1, 1): 1, (3, 2, 2, 2): 2, (3, 3, 2, 2): 3,
              (1023, 1023, 1023, 1022): 1023}
    for (a, b, c, d), want in blocks.items():
        p = np.array([[a, b], [c, d]] * 2, np.int64).reshape(4, 2)
        p = np.concatenate([p, p], axis=1)
        assert (fref.convert_plane(p, 3, 1, down=fref.LINEAR, loc=1) == want).all(), (a, b, c, d)
    # one axis converting: the other has the single weight 4 -- 4:4:4 -> 4:2:2, (l + 2 m + r + 2) >> 2
    row = np.array([[0, 1, 0, 0, 3, 1, 0, 0]], np.int64)
    assert fref.convert_plane(row, 3, 2, down=fref.LINEAR).tolist() == [[(0 + 0 + 1 + 2) >> 2, (1 + 0 + 0 + 2) >> 2, (0 + 6 + 1 + 2) >> 2, (1 + 0 + 0 + 2) >> 2]]


def test_first_and_last_rows_and_columns_are_clamped():
    c = (np.arange(8)[:, None] * 100 + np.arange(8)[None, :] * 7 + 5).astype(np.int64)
    # co-sited decimation reaches column / row -1: the first sample counts for it
    got = fref.convert_plane(c, 3, 2, down=fref.LINEAR)
    assert got[3, 0] == (4 * (1 * c[3, 0] + 2 * c[3, 0] + 1 * c[3, 1]) + 8) >> 4
    assert got[3, 3] == (4 * (1 * c[3, 5] + 2 * c[3, 6] + 1 * c[3, 7]) + 8) >> 4
    got = fref.convert_plane(c, 2, 1, down=fref.LINEAR, loc=2)
    assert got[0, 4] == (4 * (1 * c[0, 4] + 2 * c[0, 4] + 1 * c[1, 4]) + 8) >> 4
    # bottom siting reaches row 2j + 2 = 8: the last row counts for it
    got = fref.convert_plane(c, 2, 1, down=fref.LINEAR, loc=4)
    assert got[3, 4] == (4 * (1 * c[6, 4] + 2 * c[7, 4] + 1 * c[7, 4]) + 8) >> 4
    # interpolation: centred reaches j - 1 at the first output and j + 1 at the last
    got = fref.convert_plane(c, 1, 3, up=fref.LINEAR, loc=1)
    assert got[0, 0] == (16 * c[0, 0] + 8) >> 4 and got[15, 15] == (16 * c[7, 7] + 8) >> 4
    assert got[0, 15] == ((1 * c[0, 7] + 3 * c[0, 7]) * 4 + 8) >> 4 and got[1, 0] == (4 * (3 * c[0, 0] + 1 * c[1, 0]) + 8) >> 4


@pytest.mark.parametrize("src,out", CHROMA_PAIRS)
def test_constants_stay_and_ramps_keep_their_range(src, out):
    hc, wc = plane_shape(src)
    for loc in range(6):
        for up in (0, 1):
            for down in (0, 1):
                got = fref.convert_plane(np.full((hc, wc), 777, np.int64), src, out, up, down, loc)
                assert got.shape == plane_shape(out) and (got == 777).all()
                ramp = np.arange(hc)[:, None] * 64 + np.arange(wc)[None, :] * 4
                got = fref.convert_plane(ramp, src, out, up, down, loc)
                assert ramp.min() <= got.min() and got.max() <= ramp.max()


def test_special_formats():
    y = np.arange(48).reshape(6, 8)
    cb, cr = np.full((3, 4), 7), np.full((3, 4), 9)
    assert len(fref.convert_planes([y, cb, cr], 1, 0)) == 1                           # output 4:0:0: Y alone
    for out, shape in ((1, (3, 4)), (2, (6, 4)), (3, (6, 8))):                        # 4:0:0 source: 1 << (D - 1)
        got = fref.convert_planes([y], 0, out, depth_chroma=10)
        assert [p.shape for p in got[1:]] == [shape, shape] and (got[1] == 512).all() and (got[2] == 512).all()
    same = fref.convert_planes([y, cb, cr], 1, 1, 1, 1, 3)
    assert all(np.array_equal(a, b) for a, b in zip(same, [y, cb, cr]))


# ------------------------------------------------------------------------------------------------ against HM and the chroma stage
@pytest.mark.parametrize("src,out", PAIRS)
def test_drop_and_replicate_are_writeplane(src, out):
    """writePlane's index arithmetic, transcribed literally, for all 16 pairs (module docstring: the row pointer of the two pairs
    whose file has more chroma rows than the source)"""
    w, h = 16, 12
    rng = np.random.default_rng(10 * src + out)
    y = rng.integers(0, 256, (h, w))
    planes = [y] if src == 0 else [y] + [rng.integers(0, 256, plane_shape(src, w, h)) for _ in range(2)]
    got = fref.convert_planes(planes, src, out, fref.REPLICATE, fref.DROP, 0, depth_chroma=8)
    idx = fref.write_plane_indices(src, out, w, h)
    if out == 0:
        assert idx == (None, None) and len(got) == 1
        return
    if src == 0:
        assert idx is None and (got[1] == 128).all() and (got[2] == 128).all() and got[1].shape == plane_shape(out, w, h)
        return
    rows, cols = idx
    ssy, osy = fref.shifts(src)[1], fref.shifts(out)[1]
    if ssy > osy:
        # the file has more rows than the source: HM's pointer is one row ahead on odd rows, the export is not
        assert rows == [(r + 1) >> 1 for r in range(h)]
        rows = [r >> 1 for r in range(h)]
    for k in (1, 2):
        assert np.array_equal(got[k], planes[k][rows][:, cols]), (src, out, k)


@pytest.mark.parametrize("loc", range(6))
def test_linear_up_is_the_chroma_stage(loc):
    rng = np.random.default_rng(loc)
    c420, c422 = rng.integers(0, 1024, (10, 9)), rng.integers(0, 1024, (20, 9))
    assert np.array_equal(fref.convert_plane(c420, 1, 3, up=fref.LINEAR, loc=loc), chref.upsample(c420, 1, 1, loc))
    assert np.array_equal(fref.convert_plane(c422, 2, 3, up=fref.LINEAR, loc=loc), chref.upsample(c422, 1, 0, loc))
    # 4:2:0 -> 4:2:2: the vertical taps only -- the columns of c' that sit on a chroma sample (even luma columns, co-sited types)
    if loc % 2 == 0:
        assert np.array_equal(fref.convert_plane(c420, 1, 2, up=fref.LINEAR, loc=loc), chref.upsample(c420, 1, 1, loc)[:, ::2])


@pytest.mark.parametrize("src,out", [(1, 2), (1, 3), (2, 3)])
def test_up_then_drop_is_the_identity(src, out):
    c = np.random.default_rng(src + out).integers(0, 4096, plane_shape(src))
    up = fref.convert_plane(c, src, out, up=fref.REPLICATE)
    assert np.array_equal(fref.convert_plane(up, out, src, down=fref.DROP), c)


# ------------------------------------------------------------------------------------------------ the struct, the refusals, the plans
def test_struct_matches_the_header(tmp_path):
    src = tmp_path / "fmt.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(hmgpu_export_format),offsetof(hmgpu_export_format,chroma_format),offsetof(hmgpu_export_format,up),'
                   'offsetof(hmgpu_export_format,down),offsetof(hmgpu_export_format,loc),offsetof(hmgpu_export_format,reserved),'
                   'HMGPU_DOWN_DROP,HMGPU_DOWN_LINEAR);return 0;}\n')
    exe = tmp_path / "fmt"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    F = abi.ExportFormat
    assert got == [C.sizeof(F), F.chroma_format.offset, F.up.offset, F.down.offset, F.loc.offset, F.reserved.offset, abi.DOWN_DROP, abi.DOWN_LINEAR]
    f = abi.make_export_format("444", "linear", "linear", 2)
    assert (f.chroma_format, f.up, f.down, f.loc, list(f.reserved)) == (3, 1, 1, 2, [0] * 4)


def _seq(fmt=1, w=64, h=48, bd=8):
    s = abi.make_seq(w, h, bd)
    s.chroma_format = fmt
    return s


def _fmt(cf=3, up=0, down=0, loc=0, reserved=0):
    f = abi.make_export_format(cf, up, down, loc)
    f.reserved[3] = reserved
    return f


def _status(seq, desc, fmt, scale=None, tensor=None, windows=None, want=OK):
    plan = abi.ExportPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    wins = None if windows is None else (abi.ExportWindow * len(windows))(*windows)
    st = libhm_amd.lib().hmgpu_export_format_plan_for(C.byref(seq), C.byref(desc), None if scale is None else C.byref(scale),
                                                      None if tensor is None else C.byref(tensor), 1 if windows is None else len(windows), wins,
                                                      None if fmt is None else C.byref(fmt), C.byref(plan))
    assert st == want, "status %d, expected %d" % (st, want)
    if want != OK:
        assert bytes(plan) == bytes(C.sizeof(plan)), "a refused plan must be all zero"
    return plan


PLANAR, SEMI, RGB = abi.EXPORT_PLANAR, abi.EXPORT_SEMIPLANAR, abi.EXPORT_RGB


def test_each_refusal():
    seq, d = _seq(), abi.make_export_desc(PLANAR)
    _status(seq, d, _fmt())
    _status(seq, abi.make_export_desc(RGB), _fmt(), want=EINVAL)                                   # 2
    _status(seq, d, None, want=EINVAL)                                                             # 3
    _status(seq, d, _fmt(reserved=1), want=EINVAL)
    for cf in (-1, 4):
        _status(seq, d, _fmt(cf), want=EINVAL)
    for loc in (-1, 6):
        _status(seq, d, _fmt(loc=loc), want=EINVAL)
    _status(seq, d, _fmt(up=2), want=EUNSUPPORTED)                                                 # 4
    _status(seq, d, _fmt(down=2), want=EUNSUPPORTED)
    _status(seq, d, _fmt(down=-1), want=EUNSUPPORTED)
    # 5: whole chroma samples of the output format as well -- a 4:4:4 picture may be cropped by odd amounts, its 4:2:0 export not
    s444 = _seq(3)
    for crop in ((1, 1, 0, 0), (0, 0, 1, 1), (2, 1, 0, 0), (0, 0, 0, 1)):
        _status(s444, abi.make_export_desc(PLANAR, crop=crop), _fmt(3))
        _status(s444, abi.make_export_desc(PLANAR, crop=crop), _fmt(1), want=EINVAL)
    _status(s444, abi.make_export_desc(PLANAR, crop=(0, 0, 1, 1)), _fmt(2))                        # 4:2:2: rows are not subsampled
    _status(s444, d, _fmt(1), windows=[abi.make_export_window((0, 32, 0, 24)), abi.make_export_window((2, 30, 3, 21))], want=EINVAL)
    _status(s444, d, _fmt(1), windows=[abi.make_export_window((0, 32, 0, 24)), abi.make_export_window((2, 30, 4, 20))])
    _status(s444, d, _fmt(1), scale=abi.make_export_scale(31, 24), want=EINVAL)
    _status(s444, d, _fmt(2), scale=abi.make_export_scale(32, 23))
    # (scaled) a chroma axis beyond the limits: 64 -> 512 luma is 8x, 32 -> 512 chroma 16x
    _status(_seq(1), d, _fmt(3), scale=abi.make_export_scale(512, 48), want=EUNSUPPORTED)
    _status(_seq(3), d, _fmt(3), scale=abi.make_export_scale(512, 48))
    # a 4:0:0 source: the chroma output depth is looked at here
    _status(_seq(0), abi.make_export_desc(PLANAR, (8, 10), 1), _fmt(1), want=EINVAL)
    _status(_seq(0), abi.make_export_desc(PLANAR, (8, 10), 1), _fmt(0))
    _status(_seq(0), abi.make_export_desc(PLANAR, (8, 10), 2), _fmt(1))
    # semi-planar float elements stay unsupported; planar float is fine
    t = abi.make_export_tensor(abi.SAMPLE_F16)
    _status(seq, abi.make_export_desc(SEMI), _fmt(), tensor=t, want=EUNSUPPORTED)
    _status(seq, d, _fmt(), tensor=t)


def test_the_order_of_the_refusals():
    """two rules broken at once: the earlier one's status"""
    seq, d = _seq(), abi.make_export_desc(PLANAR)
    t = abi.make_export_tensor(abi.SAMPLE_F16)
    bad_desc = abi.make_export_desc(PLANAR)
    bad_desc.reserved[0] = 1
    _status(seq, bad_desc, _fmt(up=2), want=EINVAL)                                                # 1 before 4
    _status(seq, abi.make_export_desc(SEMI), _fmt(cf=9), tensor=t, want=EUNSUPPORTED)              # 1 (semi-planar float) before 3
    _status(seq, abi.make_export_desc(SEMI), None, tensor=t, want=EUNSUPPORTED)
    _status(seq, abi.make_export_desc(PLANAR, crop=(1, 0, 0, 0)), _fmt(up=2), want=EINVAL)         # 1 (the source's own crop rule) before 4
    _status(seq, d, _fmt(up=2), scale=abi.make_export_scale(1024, 48), want=EUNSUPPORTED)          # 1 (the limits) ...
    _status(seq, d, _fmt(cf=7), scale=abi.make_export_scale(1024, 48), want=EUNSUPPORTED)          # ... before 3
    _status(seq, abi.make_export_desc(RGB, matrix=3), _fmt(), want=EUNSUPPORTED)                   # 1 (unknown matrix) before 2
    _status(seq, abi.make_export_desc(RGB), _fmt(up=2), want=EINVAL)                               # 2 before 4
    _status(seq, abi.make_export_desc(RGB), None, want=EINVAL)                                     # 2 with 3
    _status(seq, d, _fmt(cf=4, up=2), want=EINVAL)                                                 # 3 before 4
    _status(seq, d, _fmt(loc=6, down=2), want=EINVAL)
    _status(_seq(0), abi.make_export_desc(PLANAR, (8, 10), 1), _fmt(1, up=2), want=EINVAL)         # 3 (4:0:0 chroma depth) before 4
    _status(_seq(3), abi.make_export_desc(PLANAR, crop=(1, 1, 0, 0)), _fmt(1, down=2), want=EUNSUPPORTED)   # 4 before 5
    _status(_seq(3), d, _fmt(1, up=2), scale=abi.make_export_scale(31, 24), want=EUNSUPPORTED)
    win = abi.make_export_window((0, 0, 0, 0))
    win.flip = 2
    _status(seq, d, _fmt(up=2), windows=[win], want=EINVAL)                                        # 1 (a window's own fields) before 4


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("layout", [PLANAR, SEMI])
def test_plan_of_the_source_format_is_the_existing_plan(fmt, layout):
    seq = _seq(fmt, 72, 40, 10)
    d = abi.make_export_desc(layout, (10, 9), 2, 1, (4, 8, 2, 6))
    fields = lambda p: (p.planes, list(p.width), list(p.height), list(p.row_bytes), list(p.coef))
    assert fields(_status(seq, d, _fmt(fmt, 1, 1, 3))) == fields(libhm_amd.export_tensor_plan(seq, d))
    sc = abi.make_export_scale(48, 30, abi.SCALE_BICUBIC)
    assert fields(_status(seq, d, _fmt(fmt), scale=sc)) == fields(libhm_amd.export_tensor_plan(seq, d, sc))
    d0 = abi.make_export_desc(layout, (10, 9), 2, 1)
    wins = [abi.make_export_window((4, 8, 2, 6)), abi.make_export_window((8, 4, 6, 2), True)]
    assert fields(_status(seq, d0, _fmt(fmt), windows=wins)) == fields(libhm_amd.export_windows_plan(seq, d0, None, None, wins))
    if layout == PLANAR:
        t, df = abi.make_export_tensor(abi.SAMPLE_F32), abi.make_export_desc(layout, (10, 9), 2)     # (float elements: not msb_aligned)
        assert fields(_status(seq, df, _fmt(fmt), tensor=t, windows=wins)) == fields(libhm_amd.export_windows_plan(seq, df, None, t, wins))


@pytest.mark.parametrize("src,out", PAIRS)
def test_plan_sizes(src, out):
    seq = _seq(src, 72, 40)
    osx, osy = fref.shifts(out)
    for layout in (PLANAR, SEMI):
        p = _status(seq, abi.make_export_desc(layout, 0, 2, crop=(4, 8, 2, 6)), _fmt(out))
        planes = 1 if out == 0 else 3 if layout == PLANAR else 2
        assert p.planes == planes and (p.width[0], p.height[0], p.row_bytes[0]) == (60, 32, 120)
        for k in range(1, 3):
            want = (60 >> osx, 32 >> osy, (60 >> osx) * 2 * (1 if layout == PLANAR else 2)) if k < planes else (0, 0, 0)
            assert (p.width[k], p.height[k], p.row_bytes[k]) == want
    p = _status(seq, abi.make_export_desc(PLANAR), _fmt(out), tensor=abi.make_export_tensor(abi.SAMPLE_F32))
    assert list(p.row_bytes)[:p.planes] == [4 * p.width[k] for k in range(p.planes)]


@pytest.mark.parametrize("src,out", [(1, 3), (3, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("size", [(96, 64), (300, 232)])
def test_scaled_plan_and_tables(src, out, size):
    """class 1 goes from the cropped source chroma size to the output format's chroma size: its tables are those the existing taps
    function reports for a sequence whose chroma plane has that geometry, and the plan carries the widest of both classes"""
    seq = _seq(src, 264, 200, 10)
    d = abi.make_export_desc(PLANAR, 0, 2, crop=(8, 0, 4, 4))
    ssx, ssy = fref.shifts(src)
    osx, osy = fref.shifts(out)
    for filt in (abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
        sc = abi.make_export_scale(size[0], size[1], filt)
        p = _status(seq, d, _fmt(out), scale=sc)
        assert (p.width[0], p.height[0]) == size and (p.width[1], p.height[1]) == (size[0] >> osx, size[1] >> osy) and p.width[2] == p.width[1]
        widest = [0, 0]
        for axis in (0, 1):
            fl, cl, wl = libhm_amd.export_format_scale_taps(seq, d, sc, _fmt(out), 0, axis)
            f0, c0, w0 = libhm_amd.export_scale_taps(seq, d, sc, 0, axis)
            assert np.array_equal(fl, f0) and np.array_equal(cl, c0) and np.array_equal(wl[:, :w0.shape[1]], w0) and not wl[:, w0.shape[1]:].any()
            fc, cc, wc = libhm_amd.export_format_scale_taps(seq, d, sc, _fmt(out), 1, axis)
            n_in = ((256, 192)[axis]) >> (ssx, ssy)[axis]
            n_out = size[axis] >> (osx, osy)[axis]
            assert len(fc) == n_out and fc.min() >= 0 and (fc + cc).max() <= n_in and (wc.astype(np.int64).sum(axis=1) == 16384).all()
            # the same (in, out, filter) as a luma axis of a 4:0:0 sequence of that size: one rule, one table
            mono = _seq(0, n_in, 64) if axis == 0 else _seq(0, 64, n_in)
            msc = abi.make_export_scale(n_out, 64, filt) if axis == 0 else abi.make_export_scale(64, n_out, filt)
            fm, cm, wm = libhm_amd.export_scale_taps(mono, abi.make_export_desc(PLANAR, 0, 2), msc, 0, axis)
            assert np.array_equal(fc, fm) and np.array_equal(cc, cm) and np.array_equal(wc[:, :wm.shape[1]], wm) and not wc[:, wm.shape[1]:].any()
            widest[axis] = max(int(cc.max()), int(cl.max()))
        assert [p.coef[12], p.coef[13]] == widest
    # no chroma class where either side is 4:0:0
    with pytest.raises(libhm_amd.HmgpuError):
        libhm_amd.export_format_scale_taps(seq, d, abi.make_export_scale(96, 64), _fmt(0), 1, 0)
    with pytest.raises(libhm_amd.HmgpuError):
        libhm_amd.export_format_scale_taps(_seq(0, 264, 200, 10), d, abi.make_export_scale(96, 64), _fmt(1), 1, 0)
