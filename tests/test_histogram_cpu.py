"""The host-only half of the picture histograms (include/hmgpu.h "picture histograms"): the ctypes mirrors against the header's sizes,
hmgpu_histogram_plan_for -- geometry, depths, bins and the RGB constants for every chroma format, and every refusal with its status
--, the model's own fixed points and the helpers of libhm_amd.histogram on CPU tensors.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, histogram
from tests import histogram_ref as href

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED


def make_seq(w=416, h=240, fmt=1, bd=10, bdc=None, log2_ctu=6):
    seq = abi.make_seq(w, h, bd, bd if bdc is None else bdc, log2_ctu=log2_ctu)
    seq.chroma_format = fmt
    return seq


def plan_status(seq, desc):
    plan = abi.HistogramPlan()
    st = libhm_amd.lib().hmgpu_histogram_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    return st, plan


def export_coef(seq, matrix, full_range, depth=0, crop=(0, 0, 0, 0)):
    plan = abi.ExportPlan()
    desc = abi.make_export_desc(abi.EXPORT_RGB, (depth, 0), 2, 0, crop, matrix, full_range)
    assert libhm_amd.lib().hmgpu_export_plan_for(C.byref(seq), C.byref(desc), C.byref(plan)) == OK
    return list(plan.coef)


# ------------------------------------------------------------------------------------------------ layout
def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(hmgpu_histogram_desc),sizeof(hmgpu_histogram_result),sizeof(hmgpu_histogram_plan),'
                   'offsetof(hmgpu_histogram_result,min),offsetof(hmgpu_histogram_result,reserved),offsetof(hmgpu_histogram_plan,coef));'
                   'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert sizes == [C.sizeof(abi.HistogramDesc), C.sizeof(abi.HistogramResult), C.sizeof(abi.HistogramPlan),
                     abi.HistogramResult.min.offset, abi.HistogramResult.reserved.offset, abi.HistogramPlan.coef.offset]
    assert C.sizeof(abi.HistogramResult) == 64 and abi.HistogramResult.min.offset == 24
    assert [f for f, _ in abi.HistogramResult._fields_][:5] == list(histogram.FIELDS)
    st, plan = plan_status(make_seq(), abi.make_histogram_desc())
    assert st == OK and plan.record_bytes == 4 * C.sizeof(abi.HistogramResult) == 256


# ------------------------------------------------------------------------------------------------ plan values
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("depths", [(8, 8), (10, 10), (12, 12), (10, 8), (8, 12)], ids=lambda d: "bd%d_%d" % d)
def test_plan_geometry_depths_and_bins(fmt, depths):
    seq = make_seq(fmt=fmt, bd=depths[0], bdc=depths[1])
    csx, csy = (0 if fmt == 3 else 1), (1 if fmt in (0, 1) else 0)
    for crop in ((0, 0, 0, 0), (6, 10, 2, 14)):
        W, H = 416 - crop[0] - crop[1], 240 - crop[2] - crop[3]
        for log2_bins in (0, 4, 8, 9, 12):
            for hist in (1, 0):
                st, plan = plan_status(seq, abi.make_histogram_desc(15, log2_bins, hist, 0, 1, 0, crop))
                assert st == OK, (fmt, depths, crop, log2_bins)
                assert plan.record_bytes == 256 and not any(plan.reserved)
                for c in range(4):
                    if fmt == 0 and c in (1, 2):
                        assert [getattr(plan, f)[c] for f in ("channels", "width", "height", "depth", "log2_bins", "hist_bytes")] == [0] * 6
                        continue
                    chroma = c in (1, 2)
                    D = depths[1] if chroma else depths[0]
                    b = D if not log2_bins else min(log2_bins, D)
                    assert (plan.channels[c], plan.width[c], plan.height[c]) == (1, W >> csx if chroma else W, H >> csy if chroma else H)
                    assert (plan.depth[c], plan.log2_bins[c], plan.hist_bytes[c]) == (D, b, (4 << b) if hist else 0)
    # maxRGB at a depth of its own: its bins follow that depth, the other channels their coding depth
    st, plan = plan_status(seq, abi.make_histogram_desc(15, 0, 1, 9))
    assert st == OK and (plan.depth[3], plan.log2_bins[3], plan.hist_bytes[3]) == (9, 9, 2048) and plan.depth[0] == depths[0]


def test_channel_subsets_and_monochrome():
    for mask in range(1, 16):
        st, plan = plan_status(make_seq(fmt=2), abi.make_histogram_desc(mask))
        assert st == OK and [plan.channels[c] for c in range(4)] == [(mask >> c) & 1 for c in range(4)]
        assert [plan.width[c] for c in range(4)] == [w if (mask >> c) & 1 else 0 for c, w in enumerate((416, 208, 208, 416))]
        assert any(plan.coef) == bool(mask & 8)                         # coef is 0 when channel 3 is off
    st, plan = plan_status(make_seq(fmt=0), abi.make_histogram_desc(15))
    assert st == OK and [plan.channels[c] for c in range(4)] == [1, 0, 0, 1]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_coef_is_the_rgb_export_s(fmt):
    for depths in ((8, 8), (10, 10), (10, 8), (12, 12)):
        seq = make_seq(fmt=fmt, bd=depths[0], bdc=depths[1])
        for matrix in (1, 5, 9) + ((0,) if fmt == 3 else ()):
            for full in (0, 1):
                for depth in (0, 8, 12):
                    st, plan = plan_status(seq, abi.make_histogram_desc(8, 0, 1, depth, matrix, full, (2, 4, 6, 8)))
                    assert st == OK, (fmt, depths, matrix, full, depth)
                    assert list(plan.coef) == export_coef(seq, matrix, full, depth, (2, 4, 6, 8))
                    assert plan.depth[3] == (depth or depths[0])
        # without channel 3 the colour fields are not read: any value passes and coef stays 0
        st, plan = plan_status(seq, abi.make_histogram_desc(1, 0, 1, 99, 77, 5))
        assert st == OK and not any(plan.coef)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    seq = make_seq()
    ok = dict(channels=15, log2_bins=0, histogram=1, rgb_bit_depth=0, matrix=1, full_range=0, crop=(0, 0, 0, 0))

    def status(seq=seq, **kw):
        a = dict(ok)
        a.update(kw)
        return plan_status(seq, abi.make_histogram_desc(**a))[0]
    assert status() == OK
    # no channel; only chroma on 4:0:0; bits above channel 3
    for mask in (0, 16, -1):
        assert status(channels=mask) == EINVAL, mask
    for mask in (2, 4, 6):
        assert status(seq=make_seq(fmt=0), channels=mask) == EINVAL
    assert status(seq=make_seq(fmt=0), channels=7) == OK
    # a crop that splits chroma samples, a negative and an empty one
    for crop in ((1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 5), (-2, 0, 0, 0), (416, 0, 0, 0), (0, 0, 120, 120)):
        assert status(crop=crop) == EINVAL, crop
    assert status(seq=make_seq(fmt=2), crop=(0, 0, 1, 3)) == OK
    assert status(seq=make_seq(fmt=2), crop=(1, 0, 0, 0)) == EINVAL
    assert status(seq=make_seq(fmt=3), crop=(3, 1, 5, 7)) == OK
    # bins
    for v in (1, 2, 3, 13, -1, 16):
        assert status(log2_bins=v) == EINVAL, v
    for v in (0, 4, 12):
        assert status(log2_bins=v) == OK, v
    for v in (-1, 2):
        assert status(histogram=v) == EINVAL
    # the depth of maxRGB: 8 .. 12; above 12 the bins do not fit the LDS
    for v in (13, 14, 16):
        assert status(rgb_bit_depth=v) == EUNSUPPORTED, v
    for v in (1, 7, -1):
        assert status(rgb_bit_depth=v) == EINVAL, v
    # the matrix: one the export does not know; the identity outside 4:4:4; full_range
    for v in (2, 4, 7, 10, 14):
        assert status(matrix=v) == EUNSUPPORTED, v
    for fmt in (0, 1, 2):
        assert status(seq=make_seq(fmt=fmt), matrix=0) == EINVAL
    assert status(seq=make_seq(fmt=3), matrix=0) == OK
    assert status(full_range=2) == EINVAL
    # reserved words
    for k in range(6):
        d = abi.make_histogram_desc(**ok)
        d.reserved[k] = 1
        assert plan_status(seq, d)[0] == EINVAL, k
    # the sequence itself, and null arguments
    assert status(seq=make_seq(fmt=4)) == EINVAL
    assert status(seq=make_seq(bd=13)) == EINVAL
    L = libhm_amd.lib()
    d, plan = abi.make_histogram_desc(**ok), abi.HistogramPlan()
    assert L.hmgpu_histogram_plan_for(None, C.byref(d), C.byref(plan)) == EINVAL
    assert L.hmgpu_histogram_plan_for(C.byref(seq), None, C.byref(plan)) == EINVAL
    assert L.hmgpu_histogram_plan_for(C.byref(seq), C.byref(d), None) == EINVAL
    # a refused description leaves a zeroed plan
    plan.width[0] = 77
    d.channels = 0
    assert L.hmgpu_histogram_plan_for(C.byref(seq), C.byref(d), C.byref(plan)) == EINVAL and plan.width[0] == 0 and plan.record_bytes == 0


def test_a_luma_plane_of_2_to_the_31_samples_is_unsupported():
    """every count stays below 2^31, so the int32 views of the histograms cannot wrap"""
    assert plan_status(make_seq(w=65536, h=32768), abi.make_histogram_desc(7))[0] == EUNSUPPORTED
    assert plan_status(make_seq(w=65536, h=32768), abi.make_histogram_desc(6))[0] == EUNSUPPORTED      # the luma plane, whatever is selected
    st, plan = plan_status(make_seq(w=65536, h=32768), abi.make_histogram_desc(7, 0, 1, 0, 1, 0, (0, 0, 0, 2)))
    assert st == OK and plan.width[0] * plan.height[0] == 65536 * 32766 < 2 ** 31


def test_entry_points_refuse_without_a_context():
    L = libhm_amd.lib()
    d = abi.make_histogram_desc()
    pics = abi.handle_array([0])
    for n in (0, 1, 17):
        assert L.hmgpu_histogram_check(None, n, pics, C.byref(d), None, None, None, 256) == EINVAL
        assert L.hmgpu_pictures_histogram(None, n, pics, C.byref(d), None, None, None, 256, 0, None) == EINVAL


def test_python_argument_handling():
    assert histogram.channels_mask(("y", "cb", "cr")) == 7 and histogram.channels_mask(("Y", "maxrgb")) == 9
    assert histogram.channels_mask((1, 3)) == 10 and histogram.channels_mask(5) == 5
    for bad in (("yy",), (4,), (-1,)):
        with pytest.raises(ValueError):
            histogram.channels_mask(bad)
    assert [histogram.log2_bins(b) for b in (None, 16, 256, 4096)] == [0, 4, 8, 12]
    for bad in (8, 100, 8192, 0):
        with pytest.raises(ValueError):
            histogram.log2_bins(bad)
    d = histogram.describe(("y", "maxrgb"), 256, (2, 4, 6, 8), None, None, 8, False)
    assert (d.channels, d.log2_bins, d.histogram, d.rgb_bit_depth, d.matrix, d.full_range, tuple(d.crop)) == (9, 8, 0, 8, 1, 0, (2, 4, 6, 8))
    plan = libhm_amd.histogram_plan(make_seq(), ("y", "cb"), bins=256)
    assert [plan.hist_bytes[c] for c in range(4)] == [1024, 1024, 0, 0]
    with pytest.raises(libhm_amd.HmgpuError) as e:
        libhm_amd.histogram_plan(make_seq(), ("maxrgb",), rgb_bit_depth=13)
    assert e.value.status == EUNSUPPORTED


# ------------------------------------------------------------------------------------------------ the model
def test_model_fixed_points():
    rng = np.random.RandomState(2)
    v = rng.randint(0, 1024, size=(37, 53))
    v[0, 0], v[-1, -1] = 0, 1023
    full = href.channel(v, 10)
    assert full["hist"].sum() == full["samples"] == 37 * 53 and len(full["hist"]) == 1024
    # the moments recomputed from a full-depth histogram equal the record
    codes = [int(c) for c in range(1024)]
    h = [int(x) for x in full["hist"]]
    assert sum(c * n for c, n in zip(codes, h)) == full["sum"] and sum(c * c * n for c, n in zip(codes, h)) == full["sum_sq"]
    assert (full["min"], full["max"]) == (0, 1023) == (min(c for c, n in zip(codes, h) if n), max(c for c, n in zip(codes, h) if n))
    # the reduced histogram is the full one summed in groups; the record does not change
    for log2_bins in (4, 8, 12):
        red = href.channel(v, 10, log2_bins)
        b = min(log2_bins, 10)
        assert np.array_equal(red["hist"], full["hist"].reshape(1 << b, -1).sum(1)) and red["hist"].sum() == red["samples"]
        assert all(red[f] == full[f] for f in href.FIELDS)
    # maxRGB of grey is luma through the matrix: R = G = B
    seq = make_seq(fmt=3, bd=8)
    coef = export_coef(seq, 1, 0)
    y = rng.randint(16, 236, size=(4, 6))
    grey = [y, np.full_like(y, 128), np.full_like(y, 128)]
    from tests import export_ref
    rgb = export_ref.export_rgb(grey, 3, (8, 8), 8, coef)
    assert np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[1], rgb[2])
    assert np.array_equal(href.max_rgb(grey, 3, (8, 8), coef), rgb[0])
    pic = href.picture(grey, 3, (8, 8), channels=(0, 3), coef=coef)
    assert pic[1] == href.ZERO and pic[2] == href.ZERO and pic[3]["samples"] == 24 and pic[0]["sum"] == int(y.sum())


# ------------------------------------------------------------------------------------------------ the helpers, on CPU tensors
def _result(hists):
    """a one-channel result as histogram.histogram builds it, from full-depth histograms (lists of counts)"""
    import torch
    h = torch.tensor(hists, dtype=torch.int32)
    codes = torch.arange(h.shape[1], dtype=torch.int64)
    hl = h.long()
    return {"hist": h, "samples": hl.sum(1), "sum": (hl * codes).sum(1), "sum_sq": (hl * codes * codes).sum(1)}


def test_percentile_mean_variance_on_a_hand_made_histogram():
    hist = [0] * 16
    hist[2], hist[5], hist[9] = 2, 5, 3                                 # ten values: 2 2 5 5 5 5 5 9 9 9
    ch = _result([hist, [0] * 15 + [4]])
    assert histogram.percentile(ch, 0.0).tolist() == [2, 15]
    assert histogram.percentile(ch, 0.2).tolist() == [2, 15]           # cumulative 2 >= 0.2 * 10
    assert histogram.percentile(ch, 0.21).tolist() == [5, 15]
    assert histogram.percentile(ch, 0.5).tolist() == [5, 15]
    assert histogram.percentile(ch, 0.69).tolist() == [5, 15]          # (0.7 * 10 is not 7 in binary64: the boundary itself is q = 0.5 above)
    assert histogram.percentile(ch, 0.71).tolist() == [9, 15]
    assert histogram.percentile(ch, 1.0).tolist() == [9, 15]
    with pytest.raises(ValueError):
        histogram.percentile(ch, 1.5)
    vals = np.array([2, 2, 5, 5, 5, 5, 5, 9, 9, 9], dtype=np.float64)
    assert abs(float(histogram.mean(ch)[0]) - vals.mean()) < 1e-12 and float(histogram.mean(ch)[1]) == 15.0
    assert abs(float(histogram.variance(ch)[0]) - vals.var()) < 1e-12 and float(histogram.variance(ch)[1]) == 0.0


def test_distance_is_0_for_equal_and_1_for_disjoint_histograms():
    a = _result([[4, 0, 4, 0], [1, 2, 3, 4], [8, 0, 0, 0]])
    b = _result([[0, 7, 0, 7], [2, 4, 6, 8], [4, 4, 0, 0]])            # disjoint; the same distribution at twice the count; half moved
    assert histogram.distance(a, b).tolist() == [1.0, 0.0, 0.5]
    assert histogram.distance(a, a).tolist() == [0.0, 0.0, 0.0]


def test_light_level_of_a_one_bin_10_bit_histogram_is_pq_eotf_of_that_code():
    for code in (0, 64, 520, 769, 1023):
        hist = [0] * 1024
        hist[code] = 12345
        peak, avg = histogram.light_level(_result([hist]), 10)
        want = float(export.pq_eotf(code / 1023.0))
        assert abs(float(peak[0]) - want) <= 1e-12 * max(want, 1.0) and abs(float(avg[0]) - want) <= 1e-9 * max(want, 1.0), code
    # two bins: the peak is the higher one's light, the average the weighted mean; another curve through eotf=
    hist = [0] * 1024
    hist[100], hist[900] = 3, 1
    peak, avg = histogram.light_level(_result([hist]), 10)
    lo, hi = float(export.pq_eotf(100 / 1023.0)), float(export.pq_eotf(900 / 1023.0))
    assert abs(float(peak[0]) - hi) < 1e-9 and abs(float(avg[0]) - (3 * lo + hi) / 4) < 1e-9
    peak, avg = histogram.light_level(_result([hist]), 10, eotf=lambda e: 100.0 * e)
    assert abs(float(peak[0]) - 100.0 * 900 / 1023) < 1e-9 and abs(float(avg[0]) - 100.0 * (300 + 900) / 4 / 1023) < 1e-9
    with pytest.raises(ValueError):
        histogram.light_level(_result([[1] * 256]), 10)                # reduced bins: a bin is not a code value
    assert "MaxCLL" in histogram.light_level.__doc__ and "MaxFALL" in histogram.light_level.__doc__
