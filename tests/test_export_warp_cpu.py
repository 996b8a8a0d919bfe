"""The affine warp export without a device: the numpy restatement (tests/export_warp_ref.py) against identities it must keep,
hmgpu_export_warp / hmgpu_warp_map against the header, the refusals of hmgpu_export_warp_plan_for in their order, its plans, and the
map helpers of libhm_amd.export."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_warp_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
W, H = 72, 40
Q = 65536


def random_s(seed, hs=11, ws=17, m=1023):
    return np.random.default_rng(seed).integers(0, m + 1, (3, hs, ws)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
@pytest.mark.parametrize("border", ["edge", "fill"])
def test_reference_identity_and_orientations(filt, border):
    S = random_s(1)
    hs, ws = S.shape[1:]
    assert np.array_equal(wref.warp(S, wref.IDENTITY, (hs, ws), filt, border, (1, 2, 3)), S)
    for k in range(4):
        for vflip in (False, True):
            for hflip in (False, True):
                m, size = export.orientation_map(k, vflip, hflip, (hs, ws))
                F = S[:, ::-1] if vflip else S
                F = F[:, :, ::-1] if hflip else F
                want = np.rot90(F, k, axes=(1, 2))
                assert size == want.shape[1:]
                assert np.array_equal(wref.warp(S, m, size, filt, border, (1, 2, 3)), want), (k, vflip, hflip)


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_reference_integer_maps_are_shifted_and_replicated_takes(filt):
    S = random_s(2)
    hs, ws = S.shape[1:]
    fill = (5, 600, 1023)
    for dx, dy in ((3, -2), (-4, 5), (30, 0), (0, -30)):
        m = (Q, 0, dx * Q, 0, Q, dy * Q)
        y, x = np.mgrid[0:hs, 0:ws]
        edge = S[:, np.clip(y + dy, 0, hs - 1), np.clip(x + dx, 0, ws - 1)]
        assert np.array_equal(wref.warp(S, m, (hs, ws), filt, "edge"), edge), (dx, dy)
        inside = (x + dx >= 0) & (x + dx < ws) & (y + dy >= 0) & (y + dy < hs)
        want = np.where(inside[None], edge, np.array(fill).reshape(3, 1, 1))
        assert np.array_equal(wref.warp(S, m, (hs, ws), filt, "fill", fill), want), (dx, dy)
    # a map of 2 * 65536 takes every second sample; 0 replicates one
    assert np.array_equal(wref.warp(S, (2 * Q, 0, 0, 0, 2 * Q, Q), (5, 8), filt), S[:, 1:11:2, 0:16:2])
    assert (wref.warp(S, (0, 0, 4 * Q, 0, 0, 7 * Q), (3, 3), filt) == S[:, 7:8, 4:5]).all()


def test_reference_half_sample_is_the_rounded_mean():
    """fx = 128 (m2 = 32768 - 128 + 128): the two columns weigh 128 * 256 each, (a + b + 1) >> 1; both axes: (a + b + c + d + 2) >> 2"""
    S = random_s(3)
    hs, ws = S.shape[1:]
    out = wref.warp(S, (Q, 0, Q // 2, 0, Q, 0), (hs, ws - 1), "bilinear")
    assert np.array_equal(out, (S[:, :, :-1] + S[:, :, 1:] + 1) >> 1)
    out = wref.warp(S, (Q, 0, Q // 2, 0, Q, Q // 2), (hs - 1, ws - 1), "bilinear")
    assert np.array_equal(out, (S[:, :-1, :-1] + S[:, :-1, 1:] + S[:, 1:, :-1] + S[:, 1:, 1:] + 2) >> 2)
    # the rim under fill: the outside column contributes the fill value with the same weight
    out = wref.warp(S, (Q, 0, -Q // 2, 0, Q, 0), (hs, 1), "bilinear", "fill", (9, 9, 9))
    assert np.array_equal(out[:, :, 0], (9 + S[:, :, 0] + 1) >> 1)
    # nearest rounds the half sample up
    assert np.array_equal(wref.warp(S, (Q, 0, Q // 2, 0, Q, 0), (hs, ws - 1), "nearest"), S[:, :, 1:])


def test_reference_extreme_maps_stay_defined():
    S = random_s(4)
    big, small = (1 << 31) - 1, -(1 << 31)
    for m in ((big, 0, small, 0, Q, 0), (Q, big, 0, small, big, small), (small, small, small, small, small, small), (big,) * 6):
        for border in ("edge", "fill"):
            out = wref.warp(S, m, (4, 6), "bilinear", border, (1, 2, 3))
            assert out.shape == (3, 4, 6) and out.min() >= 0 and out.max() <= 1023


# ------------------------------------------------------------------------------------------------ 2. the structs
def test_structs_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d\\n",'
                   'sizeof(hmgpu_export_warp),offsetof(hmgpu_export_warp,width),offsetof(hmgpu_export_warp,height),'
                   'offsetof(hmgpu_export_warp,filter),offsetof(hmgpu_export_warp,border),offsetof(hmgpu_export_warp,fill),'
                   'offsetof(hmgpu_export_warp,reserved),sizeof(hmgpu_warp_map),offsetof(hmgpu_warp_map,reserved),'
                   'HMGPU_WARP_NEAREST,HMGPU_WARP_BILINEAR,HMGPU_WARP_EDGE,HMGPU_WARP_FILL);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    E, M = abi.ExportWarp, abi.WarpMap
    mine = [C.sizeof(E), E.width.offset, E.height.offset, E.filter.offset, E.border.offset, E.fill.offset, E.reserved.offset, C.sizeof(M),
            M.reserved.offset, abi.WARP_NEAREST, abi.WARP_BILINEAR, abi.WARP_EDGE, abi.WARP_FILL]
    assert got == mine == [48, 0, 4, 8, 12, 16, 28, 32, 24, 0, 1, 0, 1]


# ------------------------------------------------------------------------------------------------ 3. plans and refusals
def seq_of(fmt=1, bd=8):
    seq = abi.make_seq(W, H, bd, bd)
    seq.chroma_format = fmt
    return seq


def rgb(bd=8, **kw):
    return abi.make_export_desc(abi.EXPORT_RGB, bd, 1 if bd == 8 else 2, 0, (0, 0, 0, 0), kw.pop("matrix", 1), 0, **kw)


def status(seq, desc, warp, maps, tensor=None, windows=None, pixel=None, lut=None, chroma=None, n=None):
    return libhm_amd.export_warp_status(seq, desc, tensor, windows, pixel, lut, chroma, warp, maps, n)[0]


def maps_of(n, m=wref.IDENTITY):
    return abi.warp_map_array([m] * n)


def test_plan_is_the_matching_plan_at_the_output_size():
    seq = seq_of()
    wp = abi.make_export_warp(61, 37)
    st, plan = libhm_amd.export_warp_status(seq, rgb(), None, None, None, None, None, wp, maps_of(1))
    assert st == OK and plan.planes == 3 and list(plan.width) == [61] * 3 and list(plan.height) == [37] * 3 and list(plan.row_bytes) == [61] * 3
    assert list(plan.coef) == list(libhm_amd.export_plan(seq, rgb()).coef)
    t = abi.make_export_tensor(abi.SAMPLE_F32)
    st, plan = libhm_amd.export_warp_status(seq, rgb(), t, None, abi.make_export_pixel(abi.PIXEL_BGRA), None, None, wp, maps_of(1))
    assert st == OK and plan.planes == 1 and plan.width[0] == 61 and plan.height[0] == 37 and plan.row_bytes[0] == 61 * 4 * 4
    # windows of different sizes are one call here; the existing unscaled call refuses them
    win = [abi.make_export_window((0, W - 20, 0, H - 10)), abi.make_export_window((2, 0, 4, 0), True)]
    st, plan = libhm_amd.export_warp_status(seq_of(bd=10), rgb(10), None, win, None, None, None, wp, maps_of(2))
    assert st == OK and plan.row_bytes[0] == 122
    with pytest.raises(libhm_amd.HmgpuError):
        libhm_amd.export_windows_plan(seq_of(bd=10), rgb(10), None, None, win)


def test_refusals_and_their_order():
    seq = seq_of()
    good = abi.make_export_warp(61, 37)
    assert status(seq, rgb(), good, maps_of(1)) == OK

    def warp(**kw):
        w = abi.make_export_warp(kw.pop("width", 61), kw.pop("height", 37), kw.pop("filter", 1), kw.pop("border", 0), kw.pop("fill", (0, 0, 0)))
        for k, v in kw.items():
            setattr(w, k, v)
        return w
    # the warp rules, one at a time
    assert status(seq, rgb(), None, maps_of(1)) == EINVAL
    assert status(seq, rgb(), good, None, n=1) == EINVAL
    w = warp()
    w.reserved[4] = 1
    assert status(seq, rgb(), w, maps_of(1)) == EINVAL
    m = maps_of(2)
    m[1].reserved[1] = 1
    assert status(seq, rgb(), good, m) == EINVAL
    for bad in (dict(width=0), dict(height=0), dict(width=16385), dict(height=-1)):
        assert status(seq, rgb(), warp(**bad), maps_of(1)) == EINVAL, bad
    assert status(seq, rgb(), warp(width=16384, height=1), maps_of(1)) == OK
    assert status(seq, rgb(), warp(border=1, fill=(0, 256, 0)), maps_of(1)) == EINVAL
    assert status(seq, rgb(), warp(border=1, fill=(0, 0, -1)), maps_of(1)) == EINVAL
    assert status(seq, rgb(), warp(border=1, fill=(255, 0, 255)), maps_of(1)) == OK
    assert status(seq, rgb(), warp(border=0, fill=(-7, 999, 1 << 20)), maps_of(1)) == OK           # ignored under EDGE
    assert status(seq_of(bd=10), rgb(10), warp(border=1, fill=(1023, 0, 0)), maps_of(1)) == OK     # M follows the output depth
    assert status(seq, abi.make_export_desc(abi.EXPORT_PLANAR, 8, 1), good, maps_of(1)) == EINVAL
    for bad in (dict(filter=2), dict(filter=-1), dict(border=2), dict(border=-1)):
        assert status(seq, rgb(), warp(**bad), maps_of(1)) == EUNSUPPORTED, bad
    # any int32 is a legal map value
    assert status(seq, rgb(), good, abi.warp_map_array([[(1 << 31) - 1, -(1 << 31), 0, -1, 1, -(1 << 31)]])) == OK
    # order within the warp rules: EINVAL (a bad size, a bad fill, the layout) before EUNSUPPORTED (the filter)
    assert status(seq, rgb(), warp(width=0, filter=9), maps_of(1)) == EINVAL
    assert status(seq, rgb(), warp(border=1, fill=(300, 0, 0), filter=9), maps_of(1)) == EINVAL
    assert status(seq, abi.make_export_desc(abi.EXPORT_PLANAR, 8, 1), warp(filter=9), maps_of(1)) == EINVAL
    # the matching call's refusals come first, with their own statuses: an unknown matrix (EUNSUPPORTED) before a NULL warp
    # (EINVAL); a window that is not whole chroma samples, a bad pixel order, a LUT of another depth and a bad chroma descriptor
    # (EINVAL) before an unknown filter (EUNSUPPORTED); an unknown chroma filter (EUNSUPPORTED) before a bad size (EINVAL)
    assert status(seq, rgb(matrix=7), None, None, n=1) == EUNSUPPORTED
    unk = warp(filter=9)
    assert status(seq, rgb(), unk, maps_of(1), windows=[abi.make_export_window((1, 0, 0, 0))]) == EINVAL
    assert status(seq, rgb(), unk, maps_of(1), pixel=abi.make_export_pixel(9)) == EINVAL
    assert status(seq, rgb(), unk, maps_of(1), lut=abi.make_colour_lut_desc(10, 17, 0)) == EINVAL
    assert status(seq, rgb(), unk, maps_of(1), chroma=abi.make_export_chroma(abi.CHROMA_LINEAR, 6)) == EINVAL
    assert status(seq, rgb(), warp(width=0), maps_of(1), chroma=abi.make_export_chroma(2, 0)) == EUNSUPPORTED
    assert status(seq, rgb(), good, maps_of(1), lut=abi.make_colour_lut_desc(8, 17, 0), chroma=abi.make_export_chroma(abi.CHROMA_LINEAR, 3)) == OK
    # the batch: 1 .. 16 slots, with or without windows
    assert status(seq, rgb(), good, maps_of(16), n=16) == OK
    assert status(seq, rgb(), good, maps_of(16), n=0) == EINVAL
    assert status(seq, rgb(), good, maps_of(17), n=17) == EINVAL
    # a refused plan is zeroed
    st, plan = libhm_amd.export_warp_status(seq, rgb(), None, None, None, None, None, unk, maps_of(1))
    assert st == EUNSUPPORTED and bytes(C.string_at(C.byref(plan), C.sizeof(plan))) == bytes(C.sizeof(plan))


def test_the_identity_matrix_needs_444_as_in_the_existing_call():
    assert status(seq_of(1), rgb(matrix=0), abi.make_export_warp(8, 8), maps_of(1)) == EINVAL
    assert status(seq_of(3), rgb(matrix=0), abi.make_export_warp(8, 8), maps_of(1)) == OK


# ------------------------------------------------------------------------------------------------ 4. the helpers
def test_orientation_maps_are_exact_integers():
    want = {(0, False, False): ((Q, 0, 0, 0, Q, 0), (H, W)),
            (1, False, False): ((0, -Q, (W - 1) * Q, Q, 0, 0), (W, H)),
            (2, False, False): ((-Q, 0, (W - 1) * Q, 0, -Q, (H - 1) * Q), (H, W)),
            (3, False, False): ((0, Q, 0, -Q, 0, (H - 1) * Q), (W, H)),
            (0, False, True): ((-Q, 0, (W - 1) * Q, 0, Q, 0), (H, W)),
            (0, True, False): ((Q, 0, 0, 0, -Q, (H - 1) * Q), (H, W)),
            (1, False, True): ((0, Q, 0, Q, 0, 0), (W, H)),                                       # the transpose
            (1, True, False): ((0, -Q, (W - 1) * Q, -Q, 0, (H - 1) * Q), (W, H))}                 # the anti-transpose
    for (k, v, h), (m, size) in want.items():
        got = export.orientation_map(k, v, h, (H, W))
        assert got == (m, size), (k, v, h)
        assert all(isinstance(x, int) and x % Q == 0 for x in got[0])
    # the eight are the whole group: the other combinations repeat them
    eight = {export.orientation_map(k, v, h, (H, W)) for k in range(4) for v in (False, True) for h in (False, True)}
    assert len(eight) == 8 and export.orientation_map(5, False, False, (H, W)) == export.orientation_map(1, False, False, (H, W))


def test_affine_map_conventions():
    assert export.affine_map((H, W), (H, W)) == (Q, 0, 0, 0, Q, 0)
    assert export.affine_map((37, 61), (37, 61), angle=0, scale=1, shear=(0, 0), translate=(0, 0)) == (Q, 0, 0, 0, Q, 0)
    # a quarter turn counter-clockwise is orientation 1 (square source: the centres coincide)
    got = export.affine_map((40, 40), (40, 40), angle=90)
    assert all(abs(a - b) <= 1 for a, b in zip(got, export.orientation_map(1, False, False, (40, 40))[0]))
    # zoom by 2 about the middle: steps of half a sample, output pixel 0 at source index -0.25 + W / 4
    assert export.affine_map((H, W), (H, W), scale=2) == (Q // 2, 0, (W * Q - Q) // 4, 0, Q // 2, (H * Q - Q) // 4)
    # a move of the picture by (+3, -2) output samples reads from (-3, +2)
    assert export.affine_map((H, W), (H, W), translate=(3, -2)) == (Q, 0, -3 * Q, 0, Q, 2 * Q)
    # another output size: the middles coincide
    assert export.affine_map((20, 36), (H, W)) == (Q, 0, 18 * Q, 0, Q, 10 * Q)
    # round half away from zero
    assert export._q16(0.5 / Q) == 1 and export._q16(-0.5 / Q) == -1 and export._q16(1.49 / Q) == 1 and export._q16(-2.5 / Q) == -3


def test_random_affine_is_reproducible():
    import torch
    kw = dict(degrees=45, translate=(0.1, 0.2), scale=(0.5, 2.0), shear=(-10, 10, -5, 5))
    a = export.random_affine(5, (37, 61), (H, W), generator=torch.Generator().manual_seed(7), **kw)
    b = export.random_affine(5, (37, 61), (H, W), generator=torch.Generator().manual_seed(7), **kw)
    c = export.random_affine(5, (37, 61), (H, W), generator=torch.Generator().manual_seed(8), **kw)
    assert a == b and a != c and len(a) == 5 and len(set(a)) == 5 and all(len(m) == 6 for m in a)
    assert export.random_affine(2, (H, W), (H, W)) == [(Q, 0, 0, 0, Q, 0)] * 2
    # within the ranges: with no rotation and no shear the scale is 1 / m0
    for m in export.random_affine(20, (H, W), (H, W), scale=(0.5, 2.0), generator=torch.Generator().manual_seed(1)):
        assert Q // 2 - 1 <= m[0] <= 2 * Q + 1 and m[1] == 0 and m[3] == 0 and m[4] == m[0]


def test_python_keywords():
    assert abi.warp_stage(None, None, "bicubic", "edge", None, 3) is None
    with pytest.raises(ValueError):
        abi.warp_stage(None, None, "bilinear", "fill", None, 1)
    with pytest.raises(ValueError):
        abi.warp_stage([wref.IDENTITY], None, "bilinear", "edge", None, 1)          # size is required
    for bad in (dict(filter="bicubic"), dict(filter="area"), dict(border="reflect")):
        kw = dict(filter="bilinear", border="edge")
        kw.update(bad)
        with pytest.raises(ValueError):
            abi.warp_stage([wref.IDENTITY], (8, 8), kw["filter"], kw["border"], None, 1)
    with pytest.raises(ValueError):
        abi.warp_stage([wref.IDENTITY] * 2, (8, 8), "bilinear", "edge", None, 3)      # one map per picture
    with pytest.raises(ValueError):
        abi.warp_stage([(1, 2, 3)], (8, 8), "bilinear", "edge", None, 1)
    w, maps = abi.warp_stage(np.array([wref.IDENTITY, (1, 2, 3, 4, 5, -6)]), (37, 61), "nearest", "fill", (1, 2, 3), 2)
    assert (w.width, w.height, w.filter, w.border, list(w.fill)) == (61, 37, abi.WARP_NEAREST, abi.WARP_FILL, [1, 2, 3])
    assert list(maps[1].m) == [1, 2, 3, 4, 5, -6] and len(maps) == 2
    assert export.one_map(wref.IDENTITY) == [list(wref.IDENTITY)] and export.one_map([wref.IDENTITY]) == [wref.IDENTITY]
    assert export.one_map(None) is None
