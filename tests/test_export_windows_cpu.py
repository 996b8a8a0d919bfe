"""Batched export with per-picture windows, host side (no GPU): the new struct's size, hmgpu_export_windows_plan_for's geometry and
refusals, export.random_resized_crop's sampling, export.make_windows' composition with a crop."""
import ctypes as C
import os
import subprocess

import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_ref as ref
from tests.export_windows_ref import desc_with_crop, window_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 200, 72
E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED


def seq_of(fmt, bd=10, w=W, h=H):
    s = abi.make_seq(w, h, bd, bd)
    s.chroma_format = fmt
    return s


def plan_status(seq, desc, scale, tensor, windows, n=None, null=False):
    plan = abi.ExportPlan()
    windows = list(windows)
    arr = (abi.ExportWindow * max(len(windows), 1))(*windows)
    st = libhm_amd.lib().hmgpu_export_windows_plan_for(C.byref(seq), C.byref(desc), C.byref(scale) if scale is not None else None,
                                                       C.byref(tensor) if tensor is not None else None,
                                                       len(windows) if n is None else n, None if null else arr, C.byref(plan))
    return st, plan


def test_struct_size_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(hmgpu_export_window),offsetof(hmgpu_export_window,flip),offsetof(hmgpu_export_window,reserved));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.ExportWindow), abi.ExportWindow.flip.offset, abi.ExportWindow.reserved.offset] == [32, 16, 20]


MIXED = [(8, 8, 16, 16), (0, 0, 200, 72), (20, 0, 64, 72), (2, 2, 198, 70), (120, 10, 80, 40), (10, 42, 100, 30)]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ref.PLANAR, ref.SEMIPLANAR, ref.RGB])
def test_plan_is_that_of_the_single_calls(fmt, layout):
    """sizes, row bytes and coef[0 .. 11] of every single plan; coef[12] / coef[13] the maximum over the windows"""
    seq = seq_of(fmt)
    desc = abi.make_export_desc(layout, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    for filt in (abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
        for tensor in (None, abi.make_export_tensor(abi.SAMPLE_F16)):
            if tensor is not None and layout == ref.SEMIPLANAR:
                continue
            scale = abi.make_export_scale(40, 24, filt)
            wins = [window_of(seq, MIXED[i % len(MIXED)], i & 1) for i in range(16)]
            st, plan = plan_status(seq, desc, scale, tensor, wins)
            assert st == abi.HMGPU_OK
            singles = [libhm_amd.export_tensor_plan(seq, desc_with_crop(desc, tuple(w.crop)), scale, tensor) for w in wins]
            for s in singles:
                assert (s.planes, list(s.width), list(s.height), list(s.row_bytes), list(s.coef)[:12]) == \
                       (plan.planes, list(plan.width), list(plan.height), list(plan.row_bytes), list(plan.coef)[:12])
            assert plan.coef[12] == max(s.coef[12] for s in singles) and plan.coef[13] == max(s.coef[13] for s in singles)
            assert len({s.coef[12] for s in singles}) > 1 or filt == abi.SCALE_NEAREST
    # unscaled: equal sizes at different origins (left edges that are no multiple of 4 included)
    wins = [window_of(seq, (x, y, 94, 40)) for x, y in ((0, 0), (2, 2), (6, 6), (106, 32))]
    st, plan = plan_status(seq, desc, None, None, wins)
    single = libhm_amd.export_tensor_plan(seq, desc_with_crop(desc, tuple(wins[0].crop)))
    assert st == abi.HMGPU_OK
    assert (plan.planes, list(plan.width), list(plan.height), list(plan.row_bytes), list(plan.coef)) == \
           (single.planes, list(single.width), list(single.height), list(single.row_bytes), list(single.coef))


@pytest.mark.parametrize("place", [0, 7, 15])
def test_refusals_wherever_the_bad_window_stands(place):
    """every refusal of the header, the bad window first, in the middle and last among 16, with the status the single call gives"""
    seq = seq_of(1)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    planar = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    scale = abi.make_export_scale(6, 2, abi.SCALE_BILINEAR)
    good = window_of(seq, (0, 0, 96, 40))

    def status(bad, desc_=desc, scale_=None):
        wins = [good] * 16
        wins[place] = bad
        st, plan = plan_status(seq, desc_, scale_, None, wins)
        assert st != abi.HMGPU_OK and plan.planes == 0
        single = abi.ExportPlan()
        d = desc_with_crop(desc_, tuple(bad.crop))
        st1 = libhm_amd.lib().hmgpu_export_tensor_plan_for(C.byref(seq), C.byref(d), C.byref(scale_) if scale_ is not None else None, None,
                                                          C.byref(single))
        return st, st1

    assert status(abi.make_export_window((-2, 106, 0, 32))) == (E, E)                  # negative
    assert status(abi.make_export_window((100, 100, 0, 32))) == (E, E)                 # empty
    assert status(abi.make_export_window((1, 103, 0, 32))) == (E, E)                   # half a chroma sample (4:2:0)
    assert status(abi.make_export_window((0, 104, 1, 31))) == (E, E)
    assert status(window_of(seq, (0, 0, 94, 40)))[0] == E                             # unscaled: another size
    assert status(window_of(seq, (0, 0, 96, 38)))[0] == E
    assert status(window_of(seq, (0, 0, 194, 40)), scale_=scale) == (U, U)             # beyond the 32x reduction (6 outputs)
    assert status(window_of(seq, (0, 0, 96, 66)), scale_=scale) == (U, U)              # (2 outputs)
    assert status(window_of(seq, (0, 0, 6, 40)), scale_=abi.make_export_scale(50, 20, abi.SCALE_BICUBIC)) == (U, U)   # beyond 8x enlargement
    assert status(window_of(seq, (0, 0, 96, 2)), planar, abi.make_export_scale(50, 20, abi.SCALE_BICUBIC)) == (U, U)   # (vertically, both classes)
    for bits in (2, 3, 1 << 31, -2):
        w = window_of(seq, (0, 0, 96, 40))
        w.flip = bits
        assert status(w)[0] == E
    for k in range(3):
        w = window_of(seq, (0, 0, 96, 40))
        w.reserved[k] = 1
        assert status(w)[0] == E


def test_refusals_of_the_call_itself():
    seq = seq_of(1)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    good = window_of(seq, (0, 0, 96, 40))
    assert plan_status(seq, desc, None, None, [good] * 16)[0] == abi.HMGPU_OK
    assert plan_status(seq, desc, None, None, [good] * 17)[0] == E
    assert plan_status(seq, desc, None, None, [good], n=0)[0] == E
    assert plan_status(seq, desc, None, None, [good], null=True)[0] == E
    for k in range(4):                                                                 # the window is the crop: desc->crop must be 0
        crop = [0, 0, 0, 0]
        crop[k] = 2
        assert plan_status(seq, abi.make_export_desc(ref.RGB, 8, 1, 0, tuple(crop), 1, 0), None, None, [good])[0] == E
    # what the tensor plan refuses is refused here: float semi-planar, a reserved word of the scale
    nv = abi.make_export_desc(ref.SEMIPLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    assert plan_status(seq, nv, None, abi.make_export_tensor(abi.SAMPLE_F16), [good])[0] == U
    sc = abi.make_export_scale(40, 24, abi.SCALE_AREA)
    sc.reserved[0] = 1
    assert plan_status(seq, desc, sc, None, [good])[0] == E


def test_make_windows_composes_with_the_crop():
    seq = seq_of(1)
    wins = export.make_windows(seq, (4, 8, 2, 6), [(0, 0, 188, 64), (10, 20, 50, 30)], [False, True], 2)
    assert [tuple(w.crop) for w in wins] == [(4, 8, 2, 6), (14, 136, 22, 20)] and [w.flip for w in wins] == [0, 1]
    assert export.make_windows(seq, (0, 0, 0, 0), None, None, 3) is None
    assert [tuple(w.crop) for w in export.make_windows(seq, (4, 8, 2, 6), None, [True], 1)] == [(4, 8, 2, 6)]
    for bad in ([(0, 0, 190, 64)], [(-2, 0, 10, 10)], [(0, 0, 0, 10)], [(0, 40, 10, 30)]):
        with pytest.raises(ValueError):
            export.make_windows(seq, (4, 8, 2, 6), bad, None, 1)
    with pytest.raises(ValueError):
        export.make_windows(seq, (0, 0, 0, 0), [(0, 0, 10, 10)], None, 2)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_random_resized_crop(fmt):
    """seeded and reproducible; every window inside the picture and on the chroma grid; area fraction and aspect ratio within the
    requested ranges, widened by the rounding to whole samples and the snapping outwards (at most 1.5 samples per edge in all)"""
    import torch
    width, height, n = 1920, 1080, 400
    scale, ratio = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)
    a = export.random_resized_crop(n, width, height, scale, ratio, 0.5, torch.Generator().manual_seed(7), fmt)
    b = export.random_resized_crop(n, width, height, scale, ratio, 0.5, torch.Generator().manual_seed(7), fmt)
    c = export.random_resized_crop(n, width, height, scale, ratio, 0.5, torch.Generator().manual_seed(8), fmt)
    assert a == b and a != c
    windows, flips = a
    assert len(windows) == len(flips) == n and all(isinstance(f, bool) for f in flips)
    assert 0.35 * n < sum(flips) < 0.65 * n
    mx = 0 if fmt in (0, 3) else 1
    my = 1 if fmt == 1 else 0
    seq = seq_of(fmt, w=width, h=height)
    desc = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    for x, y, w, h in windows:
        assert 0 <= x and 0 <= y and w > 0 and h > 0 and x + w <= width and y + h <= height
        assert not (x & mx or w & mx or y & my or h & my)
        # the sampled (w0, h0) lies within 0.5 (rounding) + 2 (snapping) of (w, h) per axis, below them
        lo_w, lo_h = max(w - 2.5, 0.5), max(h - 2.5, 0.5)
        assert lo_w * lo_h <= scale[1] * width * height and (w + 0.5) * (h + 0.5) >= scale[0] * width * height
        assert lo_w / (h + 0.5) <= ratio[1] and (w + 0.5) / lo_h >= ratio[0]
    wins = export.make_windows(seq, (0, 0, 0, 0), windows[:16], flips[:16], 16)
    assert libhm_amd.export_windows_plan(seq, desc, abi.make_export_scale(224, 224), None, wins).width[0] == 224
    assert export.random_resized_crop(3, 64, 48, p_flip=0.0, generator=torch.Generator().manual_seed(1))[1] == [False] * 3
    assert export.random_resized_crop(3, 64, 48, p_flip=1.0, generator=torch.Generator().manual_seed(1))[1] == [True] * 3
    # no try can fit (every aspect ratio wider than the picture allows at this area): the central fallback
    w, f = export.random_resized_crop(2, 100, 1000, (0.9, 1.0), (2.0, 3.0), 0.0, torch.Generator().manual_seed(1), fmt)
    assert w == [(0, 474, 100, 52) if my else (0, 475, 100, 50)] * 2          # (w = 100, h = 100 / 2 at y = 475, snapped outwards)


@pytest.mark.parametrize("layout", [ref.PLANAR, ref.RGB])
def test_the_sum_bound_is_not_reached_within_the_limits(layout):
    """each window's own tables go through the 32-bit sum bound of the scaled export (scale_sums_fit), and a failure there would
    refuse the call with HMGPU_EUNSUPPORTED as the per-axis limits do.  Within those limits the bound cannot be reached (include/hmgpu.h,
    "scaled export": no sum overflows for any input at any D of 8 .. 16), so no refusal by it can be provoked: windows at the 32x and
    the 8x limit, 16-bit outputs, every filter, are all accepted"""
    seq = seq_of(3, bd=12, w=4096, h=2304)
    desc = abi.make_export_desc(layout, 16, 2, 0, (0, 0, 0, 0), 1, 1)
    for filt in (abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
        for out_w, out_h, windows in ((128, 72, [(0, 0, 4096, 2304), (2, 2, 4094, 2300), (1000, 1000, 129, 73)]),
                                      (64, 64, [(0, 0, 8, 8), (4088, 2296, 8, 8), (0, 0, 2048, 2048)]),
                                      (128, 64, [(0, 0, 4096, 8), (0, 0, 16, 2048)])):
            wins = [window_of(seq, w) for w in windows]
            assert plan_status(seq, desc, abi.make_export_scale(out_w, out_h, filt), None, wins)[0] == abi.HMGPU_OK
