"""The host-only half of the picture metrics (include/hmgpu.h "picture metrics"): hmgpu_metrics_plan_for -- geometry for every chroma
format and every refusal --, hmgpu_metrics_psnr against HM's formula, the ctypes mirrors against the header's sizes, the argument
handling of libhm_amd.metrics and the model's own fixed points.  No device."""
import ctypes as C
import math

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, metrics
from tests import metrics_ref as mref


def make_seq(w=416, h=240, fmt=1, bd=10, bdc=None, log2_ctu=6):
    seq = abi.make_seq(w, h, bd, bd if bdc is None else bdc, log2_ctu=log2_ctu)
    seq.chroma_format = fmt
    return seq


def plan_status(seq, desc):
    plan = abi.MetricsPlan()
    st = libhm_amd.lib().hmgpu_metrics_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    return st, plan


# ------------------------------------------------------------------------------------------------ layout
def test_struct_sizes_match_the_header():
    assert C.sizeof(abi.MetricsResult) == 64
    assert C.sizeof(abi.MetricsDesc) == 4 * (4 + 4 + 7)
    assert C.sizeof(abi.MetricsPlan) == 4 * 16 + 8 * 3
    assert [f for f, _ in abi.MetricsResult._fields_][:8] == list(metrics.FIELDS)
    # the library's own idea of the record: result_bytes is 3 * sizeof(hmgpu_metrics_result)
    st, plan = plan_status(make_seq(), abi.make_metrics_desc(abi.METRICS_REF_PICTURES))
    assert st == abi.HMGPU_OK and plan.result_bytes == 3 * C.sizeof(abi.MetricsResult) == 192


# ------------------------------------------------------------------------------------------------ plan geometry
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("crop", [(0, 0, 0, 0), (6, 10, 2, 14), (2, 2, 2, 2), (400, 4, 220, 8), (408, 2, 0, 0)])
def test_plan_geometry(fmt, crop):
    seq = make_seq(fmt=fmt)
    csx, csy = mref.chroma_shifts(fmt)
    W, H = 416 - crop[0] - crop[1], 240 - crop[2] - crop[3]
    for ssim in (0, 1):
        for ref, bps in ((abi.METRICS_REF_PICTURES, 0), (abi.METRICS_REF_PLANES, 2)):
            st, plan = plan_status(seq, abi.make_metrics_desc(ref, 7, ssim, bps, crop))
            assert st == abi.HMGPU_OK, (fmt, crop)
            assert plan.result_bytes == 192
            for k in range(3):
                if k and fmt == 0:
                    assert (plan.channels[k], plan.width[k], plan.height[k], plan.row_bytes[k], plan.ssim_windows[k]) == (0, 0, 0, 0, 0)
                    continue
                w, h = (W >> csx, H >> csy) if k else (W, H)
                assert (plan.channels[k], plan.width[k], plan.height[k]) == (1, w, h)
                assert (plan.elem_bytes[k], plan.row_bytes[k]) == (bps, w * bps)
                assert plan.ssim_windows[k] == (mref.windows(w, h) if ssim else 0)


def test_planes_narrower_than_8_have_no_windows():
    # a 12x12 luma crop at 4:2:0: a 6x6 chroma plane; a luma plane 6 wide
    st, plan = plan_status(make_seq(), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (100, 304, 100, 128)))
    assert st == abi.HMGPU_OK
    assert (plan.width[0], plan.height[0], plan.ssim_windows[0]) == (12, 12, 4)
    assert (plan.width[1], plan.height[1], plan.ssim_windows[1], plan.ssim_windows[2]) == (6, 6, 0, 0)
    st, plan = plan_status(make_seq(fmt=3), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (0, 410, 0, 0)))
    assert st == abi.HMGPU_OK and [plan.width[k] for k in range(3)] == [6, 6, 6] and [plan.ssim_windows[k] for k in range(3)] == [0, 0, 0]
    st, plan = plan_status(make_seq(fmt=3), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (0, 408, 0, 232)))
    assert st == abi.HMGPU_OK and plan.ssim_windows[0] == 1


def test_component_subsets_and_monochrome():
    for mask in range(1, 8):
        st, plan = plan_status(make_seq(fmt=2), abi.make_metrics_desc(abi.METRICS_REF_PLANES, mask, 1, 2))
        assert st == abi.HMGPU_OK and [plan.channels[k] for k in range(3)] == [(mask >> k) & 1 for k in range(3)]
        assert [plan.width[k] for k in range(3)] == [w if (mask >> k) & 1 else 0 for k, w in enumerate((416, 208, 208))]
        assert [plan.height[k] for k in range(3)] == [h if (mask >> k) & 1 else 0 for k, h in enumerate((240, 240, 240))]
    # 4:0:0: the chroma bits are ignored, and alone they select nothing
    st, plan = plan_status(make_seq(fmt=0), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7))
    assert st == abi.HMGPU_OK and [plan.channels[k] for k in range(3)] == [1, 0, 0]
    assert plan_status(make_seq(fmt=0), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 6))[0] == abi.HMGPU_EINVAL


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    seq = make_seq()
    ok = dict(reference=abi.METRICS_REF_PLANES, components=7, ssim=1, ref_bytes_per_sample=2, crop=(0, 0, 0, 0))

    def status(seq=seq, **kw):
        a = dict(ok)
        a.update(kw)
        return plan_status(seq, abi.make_metrics_desc(**a))[0]
    assert status() == abi.HMGPU_OK
    # crop: negative, empty, half a chroma sample (4:2:0: odd in x or y; 4:2:2: odd in x only; 4:4:4 and 4:0:0: anything)
    for crop in ((-2, 0, 0, 0), (0, 0, 0, -2), (416, 0, 0, 0), (0, 0, 120, 120), (1, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 5)):
        assert status(crop=crop) == abi.HMGPU_EINVAL, crop
    assert status(seq=make_seq(fmt=2), crop=(0, 0, 1, 3)) == abi.HMGPU_OK
    assert status(seq=make_seq(fmt=2), crop=(1, 0, 0, 0)) == abi.HMGPU_EINVAL
    assert status(seq=make_seq(fmt=3), crop=(1, 3, 5, 7)) == abi.HMGPU_OK
    assert status(seq=make_seq(fmt=0), crop=(1, 3, 5, 7)) == abi.HMGPU_OK
    # components, ssim, reference
    for mask in (0, 8, -1):
        assert status(components=mask) == abi.HMGPU_EINVAL
    for v in (-1, 2):
        assert status(ssim=v) == abi.HMGPU_EINVAL
    for v in (-1, 2):
        assert status(reference=v) == abi.HMGPU_EINVAL
    # bytes per sample: 1 or 2 with planes, 0 with pictures; 1 only where every compared component is coded at <= 8 bits
    for v in (0, 3, 4, -1):
        assert status(ref_bytes_per_sample=v) == abi.HMGPU_EINVAL
    for v in (1, 2):
        assert status(reference=abi.METRICS_REF_PICTURES, ref_bytes_per_sample=v) == abi.HMGPU_EINVAL
    assert status(reference=abi.METRICS_REF_PICTURES, ref_bytes_per_sample=0) == abi.HMGPU_OK
    assert status(ref_bytes_per_sample=1) == abi.HMGPU_EINVAL                                   # depth 10
    assert status(seq=make_seq(bd=8), ref_bytes_per_sample=1) == abi.HMGPU_OK
    assert status(seq=make_seq(bd=8, bdc=10), ref_bytes_per_sample=1) == abi.HMGPU_EINVAL
    assert status(seq=make_seq(bd=8, bdc=10), ref_bytes_per_sample=1, components=1) == abi.HMGPU_OK
    assert status(seq=make_seq(bd=10, bdc=8), ref_bytes_per_sample=1, components=6) == abi.HMGPU_OK
    assert status(seq=make_seq(bd=10, bdc=8), ref_bytes_per_sample=1, components=3) == abi.HMGPU_EINVAL
    # reserved words
    for k in range(7):
        d = abi.make_metrics_desc(**ok)
        d.reserved[k] = 1
        assert plan_status(seq, d)[0] == abi.HMGPU_EINVAL, k
    # the sequence itself, and null arguments
    assert status(seq=make_seq(fmt=4)) == abi.HMGPU_EINVAL
    assert status(seq=make_seq(bd=13)) == abi.HMGPU_EINVAL
    L = libhm_amd.lib()
    d, plan = abi.make_metrics_desc(**ok), abi.MetricsPlan()
    assert L.hmgpu_metrics_plan_for(None, C.byref(d), C.byref(plan)) == abi.HMGPU_EINVAL
    assert L.hmgpu_metrics_plan_for(C.byref(seq), None, C.byref(plan)) == abi.HMGPU_EINVAL
    assert L.hmgpu_metrics_plan_for(C.byref(seq), C.byref(d), None) == abi.HMGPU_EINVAL
    # a refused description leaves a zeroed plan
    plan.width[0] = 77
    d.components = 0
    assert L.hmgpu_metrics_plan_for(C.byref(seq), C.byref(d), C.byref(plan)) == abi.HMGPU_EINVAL and plan.width[0] == 0 and plan.result_bytes == 0


def test_entry_points_refuse_without_a_context():
    """a null context is refused with HMGPU_EINVAL by both device entries, whatever n is, and nothing is dereferenced.  That is all a
    machine without a GPU can ask of them: the null context is refused before n or the references are looked at, so the n range and
    "both or neither reference" are tested where a context exists (tests/test_gpu_metrics.py, the refusals), and on the Python side
    in test_python_argument_handling below"""
    L = libhm_amd.lib()
    d = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
    pics = abi.handle_array([0])
    for n in (0, -1, 17):
        assert L.hmgpu_metrics_check(None, n, pics, C.byref(d), pics, None, None, None, None, 192) == abi.HMGPU_EINVAL
        assert L.hmgpu_pictures_metrics(None, n, pics, C.byref(d), pics, None, None, None, None, 192, 0, None) == abi.HMGPU_EINVAL


def test_planes_of_2_to_the_32_samples_are_unsupported():
    """a lane of the kernel keeps the first difference's y * w_c + x in 32 bits with all ones for "none", so a cropped component plane
    has fewer than 2^32 - 1 samples; chroma planes that are smaller pass where luma is not compared"""
    big = make_seq(w=65536, h=65536)
    pics = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
    assert plan_status(big, pics)[0] == abi.HMGPU_EUNSUPPORTED
    st, plan = plan_status(big, abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (0, 0, 0, 8)))
    assert st == abi.HMGPU_OK and plan.width[0] * plan.height[0] == 65536 * 65528 < 2 ** 32 - 1
    st, plan = plan_status(big, abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 6))
    assert st == abi.HMGPU_OK and (plan.channels[0], plan.width[1], plan.height[1]) == (0, 32768, 32768)


def test_python_argument_handling():
    with pytest.raises(ValueError):
        metrics.describe(None, None)                                   # neither reference
    with pytest.raises(ValueError):
        metrics.describe([0], [object()])                              # both
    with pytest.raises(ValueError):
        metrics.describe([0], None, components=(0, 3))
    d = metrics.describe([0], None, components=(0, 2), ssim=False, crop=(2, 4, 6, 8))
    assert (d.reference, d.components, d.ssim, d.ref_bytes_per_sample, tuple(d.crop)) == (abi.METRICS_REF_PICTURES, 5, 0, 0, (2, 4, 6, 8))
    plan = libhm_amd.metrics_plan(make_seq(), "planes", (0, 1), True, (0, 0, 0, 0), 2)
    assert [plan.row_bytes[k] for k in range(3)] == [832, 416, 0]
    with pytest.raises(libhm_amd.HmgpuError):
        libhm_amd.metrics_plan(make_seq(), "planes", ref_bytes_per_sample=1)


# ------------------------------------------------------------------------------------------------ PSNR
def test_psnr_matches_hm():
    L = libhm_amd.lib()
    rng = np.random.RandomState(3)
    cases = [(416 * 240, 0), (416 * 240, 1), (3840 * 2160, 123456789), (1, 1), (208 * 120, 2 ** 40), (2 ** 33, 2 ** 50 + 12345)]
    cases += [(int(rng.randint(1, 1 << 30)), int(rng.randint(1, 1 << 30)) << int(rng.randint(0, 20))) for _ in range(20)]
    for bd in (8, 10, 12, 16):
        for samples, sse in cases:
            r = abi.MetricsResult()
            r.samples, r.sse = samples, sse
            got = L.hmgpu_metrics_psnr(C.byref(r), bd)
            want = mref.psnr(samples, sse, bd)
            assert got == want or abs(got - want) <= 1e-12 * abs(want), (bd, samples, sse, got, want)
            if sse == 0:
                assert got == 999.99
    # 8-bit, one grey level off everywhere: 20 log10(255)
    r = abi.MetricsResult()
    r.samples = r.sse = 1000
    assert abs(L.hmgpu_metrics_psnr(C.byref(r), 8) - 20 * math.log10(255)) < 1e-12
    assert abs(L.hmgpu_metrics_psnr(C.byref(r), 10) - 20 * math.log10(1020)) < 1e-12          # maxval = 255 << 2, not 1023
    assert math.isnan(L.hmgpu_metrics_psnr(None, 8)) and math.isnan(L.hmgpu_metrics_psnr(C.byref(r), 7))


# ------------------------------------------------------------------------------------------------ the model's fixed points
def test_model_fixed_points():
    rng = np.random.RandomState(1)
    a = rng.randint(0, 1024, size=(37, 53))
    same = mref.plane(a, a, 10)
    assert same == {"samples": 37 * 53, "sse": 0, "sad": 0, "differing": 0, "first_diff": -1, "ssim_q32": 96 << 32, "ssim_windows": 96,
                    "max_abs": 0}
    b = a.copy()
    b[36, 52] += 3
    one = mref.plane(a, b, 10)
    assert (one["sse"], one["sad"], one["differing"], one["first_diff"], one["max_abs"]) == (9, 3, 1, 37 * 53 - 1, 3)
    assert one["ssim_q32"] == same["ssim_q32"]                         # the last column and row lie in no window (53 = 4 * 13 + 1)
    b = a.copy()
    b[0, 0] ^= 512
    assert mref.plane(a, b, 10)["first_diff"] == 0 and mref.plane(a, b, 10)["ssim_q32"] < same["ssim_q32"]
    # a direct evaluation of one window, sample by sample
    a8, b8 = rng.randint(0, 256, size=(8, 8)), rng.randint(0, 256, size=(8, 8))
    s1, s2, ss, s12 = int(a8.sum()), int(b8.sum()), int((a8 * a8 + b8 * b8).sum()), int((a8 * b8).sum())
    c1, c2 = mref.ssim_constants(8)
    assert (c1, c2) == (416, 235963)
    v = (float(2 * s1 * s2 + c1) * float(2 * (64 * s12 - s1 * s2) + c2)) / (float(s1 * s1 + s2 * s2 + c1) * float(64 * ss - s1 * s1 - s2 * s2 + c2))
    assert mref.ssim_q32(a8, b8, 8) == (int(np.rint(v * 4294967296.0)), 1)
    # every factor stays below 2^53 for a full-range uint16 reference against 12-bit samples
    s1, s2 = 64 * 4095, 64 * 65535
    assert 2 * s1 * s2 + mref.ssim_constants(12)[0] < 2 ** 53 and 64 * 64 * (4095 ** 2 + 65535 ** 2) + mref.ssim_constants(12)[1] < 2 ** 53
    assert mref.tolerance(0) == 1 and mref.tolerance(6000) == 6
