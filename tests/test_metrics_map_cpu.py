"""The host-only half of the picture metric maps (include/hmgpu.h "picture metric maps"): hmgpu_metrics_map_plan_for -- the block grid
for every chroma format and block size, every refusal and their order --, the ctypes mirrors against the header compiled with gcc, and
the model (tests/metrics_map_ref.py): its sum rule against tests/metrics_ref.py and its fixed points.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, metrics
from tests import metrics_map_ref as mmap
from tests import metrics_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_seq(w=416, h=240, fmt=1, bd=10, bdc=None, log2_ctu=6):
    seq = abi.make_seq(w, h, bd, bd if bdc is None else bdc, log2_ctu=log2_ctu)
    seq.chroma_format = fmt
    return seq


def plan_status(seq, desc, md):
    plan = abi.MetricsMapPlan()
    st = libhm_amd.lib().hmgpu_metrics_map_plan_for(C.byref(seq), C.byref(desc), None if md is None else C.byref(md), C.byref(plan))
    return st, plan


def map_desc(log2_block):
    md = abi.MetricsMapDesc()
    md.log2_block = log2_block
    return md


# ------------------------------------------------------------------------------------------------ layout
def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d\\n",'
                   'sizeof(hmgpu_metrics_map_desc),sizeof(hmgpu_metrics_map_plan),offsetof(hmgpu_metrics_map_plan,channels),'
                   'offsetof(hmgpu_metrics_map_plan,fields),offsetof(hmgpu_metrics_map_plan,row_bytes),(int)HMGPU_METRICS_MAP_FIELDS);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P = abi.MetricsMapPlan
    assert got == [C.sizeof(abi.MetricsMapDesc), C.sizeof(P), P.channels.offset, P.fields.offset, P.row_bytes.offset, abi.METRICS_MAP_FIELDS]
    assert got[0] == 32 and got[5] == 6 == len(metrics.MAP_FIELDS) == len(mmap.FIELDS)
    assert metrics.MAP_FIELDS == mmap.FIELDS
    assert (abi.METRICS_MAP_SSE, abi.METRICS_MAP_SAD, abi.METRICS_MAP_DIFFERING, abi.METRICS_MAP_MAX_ABS, abi.METRICS_MAP_SSIM_Q32,
            abi.METRICS_MAP_SSIM_WINDOWS) == tuple(range(6))


# ------------------------------------------------------------------------------------------------ plan geometry
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("crop", [(0, 0, 0, 0), (2, 6, 2, 4), (6, 10, 2, 14), (100, 304, 100, 128), (64, 0, 32, 0), (346, 2, 196, 4)],
                         ids=lambda c: "crop%d_%d_%d_%d" % c)
def test_plan_geometry(fmt, crop):
    """crops off the block grid and off the 4-sample window grid; (100, 304, 100, 128) leaves 12x12 luma samples"""
    seq = make_seq(fmt=fmt)
    csx, csy = mref.chroma_shifts(fmt)
    W, H = 416 - crop[0] - crop[1], 240 - crop[2] - crop[3]
    for log2 in (3, 4, 5, 6):
        B = 1 << log2
        for ssim in (0, 1):
            for ref, bps in ((abi.METRICS_REF_PICTURES, 0), (abi.METRICS_REF_PLANES, 2)):
                st, plan = plan_status(seq, abi.make_metrics_desc(ref, 7, ssim, bps, crop), map_desc(log2))
                assert st == abi.HMGPU_OK, (fmt, crop, B)
                assert (plan.blocks_x, plan.blocks_y) == (-(-W // B), -(-H // B)) == mmap.grid(W, H, B)
                assert plan.fields == (6 if ssim else 4) and plan.row_bytes == plan.blocks_x * 8
                assert not any(plan.reserved)
                for k in range(3):
                    if k and fmt == 0:
                        assert (plan.channels[k], plan.width[k], plan.height[k], plan.block_w[k], plan.block_h[k]) == (0, 0, 0, 0, 0)
                        continue
                    w, h = (W >> csx, H >> csy) if k else (W, H)
                    bw, bh = (B >> csx, B >> csy) if k else (B, B)
                    assert (plan.channels[k], plan.width[k], plan.height[k], plan.block_w[k], plan.block_h[k]) == (1, w, h, bw, bh)
                    assert (bw, bh) == mmap.block_size(fmt, B, k)
                    # every component has the luma grid
                    assert (-(-w // bw), -(-h // bh)) == (plan.blocks_x, plan.blocks_y)
                    s = metrics.map_samples(plan, k).numpy()
                    assert np.array_equal(s, mmap.samples(W, H, fmt, B, k)) and int(s.sum()) == w * h


def test_the_12x12_crop_has_a_6x6_chroma_plane_without_windows():
    crop = (100, 304, 100, 128)
    st, plan = plan_status(make_seq(), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, crop), map_desc(3))
    assert st == abi.HMGPU_OK
    assert (plan.blocks_x, plan.blocks_y, plan.width[0], plan.width[1], plan.height[2]) == (2, 2, 12, 6, 6)
    assert (plan.block_w[1], plan.block_h[1]) == (4, 4)
    rng = np.random.RandomState(5)
    a, b = rng.randint(0, 1024, size=(6, 6)), rng.randint(0, 1024, size=(6, 6))
    m = mmap.plane(a, b, 10, 4, 4, 2, 2)
    assert not m[4:].any() and m[2].tolist() == [[16, 8], [8, 4]]
    # the luma plane: four windows, all of them starting in block (0, 0) or right of / below it
    y = mmap.plane(rng.randint(0, 1024, size=(12, 12)), rng.randint(0, 1024, size=(12, 12)), 10, 8, 8, 2, 2)
    assert y[5].tolist() == [[4, 0], [0, 0]]
    # 4:2:0 at B = 8: a 4x4 chroma block holds at most one window
    c = mmap.plane(rng.randint(0, 1024, size=(120, 208)), rng.randint(0, 1024, size=(120, 208)), 10, 4, 4, 52, 30)
    assert c[5].max() == 1 and int(c[5].sum()) == mref.windows(208, 120)


def test_component_subsets_and_monochrome():
    for mask in range(1, 8):
        st, plan = plan_status(make_seq(fmt=2), abi.make_metrics_desc(abi.METRICS_REF_PLANES, mask, 1, 2), map_desc(3))
        assert st == abi.HMGPU_OK and [plan.channels[k] for k in range(3)] == [(mask >> k) & 1 for k in range(3)]
        assert [plan.block_w[k] for k in range(3)] == [v if (mask >> k) & 1 else 0 for k, v in enumerate((8, 4, 4))]
        assert [plan.block_h[k] for k in range(3)] == [v if (mask >> k) & 1 else 0 for k, v in enumerate((8, 8, 8))]   # 4:2:2: 4x8
        assert (plan.blocks_x, plan.blocks_y) == (52, 30)              # the luma grid, whether luma is compared or not
    st, plan = plan_status(make_seq(fmt=0), abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7), map_desc(4))
    assert st == abi.HMGPU_OK and [plan.channels[k] for k in range(3)] == [1, 0, 0]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_and_their_order():
    seq = make_seq()
    ok = dict(reference=abi.METRICS_REF_PLANES, components=7, ssim=1, ref_bytes_per_sample=2, crop=(0, 0, 0, 0))

    def status(seq=seq, log2=4, **kw):
        a = dict(ok)
        a.update(kw)
        return plan_status(seq, abi.make_metrics_desc(**a), map_desc(log2))[0]
    assert status() == abi.HMGPU_OK
    # the block size
    for log2 in (3, 4, 5, 6):
        assert status(log2=log2) == abi.HMGPU_OK
    for log2 in (-1, 0, 2, 7, 16):
        assert status(log2=log2) == abi.HMGPU_EINVAL, log2
    # the reserved words of the map description
    for k in range(7):
        md = map_desc(4)
        md.reserved[k] = 1
        assert plan_status(seq, abi.make_metrics_desc(**ok), md)[0] == abi.HMGPU_EINVAL, k
    # the refusals of the metrics description are its own (tests/test_metrics_cpu.py has the full list)
    for kw in (dict(crop=(-2, 0, 0, 0)), dict(crop=(1, 0, 0, 0)), dict(crop=(416, 0, 0, 0)), dict(components=0), dict(components=8), dict(ssim=2),
               dict(reference=2), dict(ref_bytes_per_sample=0), dict(ref_bytes_per_sample=1), dict(reference=abi.METRICS_REF_PICTURES),
               dict(seq=make_seq(fmt=4)), dict(seq=make_seq(bd=13)), dict(seq=make_seq(fmt=0), components=6)):
        assert status(**kw) == abi.HMGPU_EINVAL, kw
    for k in range(7):
        d = abi.make_metrics_desc(**ok)
        d.reserved[k] = 1
        assert plan_status(seq, d, map_desc(4))[0] == abi.HMGPU_EINVAL, k
    # order: the metrics description is judged first -- its HMGPU_EUNSUPPORTED (a plane of 2^32 samples) shows through a map description
    # that would be HMGPU_EINVAL, and through a missing one
    big = make_seq(w=65536, h=65536)
    pics = abi.make_metrics_desc(abi.METRICS_REF_PICTURES)
    for md in (map_desc(4), map_desc(9), None):
        assert plan_status(big, pics, md)[0] == abi.HMGPU_EUNSUPPORTED
    bad = map_desc(4)
    bad.reserved[6] = 1
    assert plan_status(big, pics, bad)[0] == abi.HMGPU_EUNSUPPORTED
    cropped = abi.make_metrics_desc(abi.METRICS_REF_PICTURES, 7, 1, 0, (0, 0, 0, 8))
    assert plan_status(big, cropped, map_desc(4))[0] == abi.HMGPU_OK
    assert plan_status(big, cropped, map_desc(9))[0] == abi.HMGPU_EINVAL
    assert plan_status(big, cropped, bad)[0] == abi.HMGPU_EINVAL
    # null arguments
    L = libhm_amd.lib()
    d, md, plan = abi.make_metrics_desc(**ok), map_desc(4), abi.MetricsMapPlan()
    assert L.hmgpu_metrics_map_plan_for(None, C.byref(d), C.byref(md), C.byref(plan)) == abi.HMGPU_EINVAL
    assert L.hmgpu_metrics_map_plan_for(C.byref(seq), None, C.byref(md), C.byref(plan)) == abi.HMGPU_EINVAL
    assert L.hmgpu_metrics_map_plan_for(C.byref(seq), C.byref(d), None, C.byref(plan)) == abi.HMGPU_EINVAL
    assert L.hmgpu_metrics_map_plan_for(C.byref(seq), C.byref(d), C.byref(md), None) == abi.HMGPU_EINVAL
    # a refused description leaves a zeroed plan
    plan.blocks_x = 77
    md.log2_block = 2
    assert L.hmgpu_metrics_map_plan_for(C.byref(seq), C.byref(d), C.byref(md), C.byref(plan)) == abi.HMGPU_EINVAL
    assert plan.blocks_x == 0 and plan.fields == 0 and plan.row_bytes == 0


def test_entry_points_refuse_without_a_context():
    L = libhm_amd.lib()
    d, md = abi.make_metrics_desc(abi.METRICS_REF_PICTURES), map_desc(4)
    pics = abi.handle_array([0])
    for n in (0, 1, 17):
        assert L.hmgpu_metrics_map_check(None, n, pics, C.byref(d), C.byref(md), pics, None, None, None, None, None, None, None) == abi.HMGPU_EINVAL
        assert L.hmgpu_pictures_metrics_map(None, n, pics, C.byref(d), C.byref(md), pics, None, None, None, None, None, None, None, 0,
                                            None) == abi.HMGPU_EINVAL


def test_python_argument_handling():
    assert [abi.make_metrics_map_desc(b).log2_block for b in (8, 16, 32, 64)] == [3, 4, 5, 6]
    for b in (0, 12, 4, 128, -16):
        with pytest.raises(libhm_amd.HmgpuError):
            libhm_amd.metrics_map_plan(make_seq(), b)
    plan = libhm_amd.metrics_map_plan(make_seq(), 32, "planes", (0, 2), False, (2, 6, 2, 4))
    assert (plan.blocks_x, plan.blocks_y, plan.fields, [plan.channels[k] for k in range(3)]) == (13, 8, 4, [1, 0, 1])
    assert not metrics.map_samples(plan, 1).any()


# ------------------------------------------------------------------------------------------------ the model
def test_the_models_windows_are_those_of_metrics_ref():
    rng = np.random.RandomState(11)
    for (h, w), bd in (((37, 53), 10), ((8, 8), 8), ((64, 72), 12), ((7, 40), 10)):
        a, b = rng.randint(0, 1 << bd, size=(h, w)), rng.randint(0, 1 << bd, size=(h, w))
        q = mmap.window_values(a, b, bd)
        assert (int(q.sum()), q.size) == mref.ssim_q32(a, b, bd)
        for j in range(q.shape[0]):
            for i in range(0, q.shape[1], 3):
                assert (int(q[j, i]), 1) == mref.ssim_q32(a[4 * j:4 * j + 8, 4 * i:4 * i + 8], b[4 * j:4 * j + 8, 4 * i:4 * i + 8], bd)


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_the_models_sum_rule(fmt):
    """summed over the blocks every field is the field of metrics_ref.plane -- exactly, ssim_q32 included: the same window values"""
    rng = np.random.RandomState(20 + fmt)
    csx, csy = mref.chroma_shifts(fmt)
    W, H = 150, 94
    shapes = [(H, W), (H >> csy, W >> csx), (H >> csy, W >> csx)]
    a = [rng.randint(0, 1024, size=s) for s in shapes]
    b = [np.clip(p + rng.randint(-40, 41, size=p.shape) * (rng.rand(*p.shape) < 0.3), 0, 1023) for p in a]
    for crop in ((0, 0, 0, 0), (2, 6, 2, 4) if fmt in (1, 2) else (3, 5, 1, 7)):
        ca, cb = mref.crop_planes(a, crop, fmt), mref.crop_planes(b, crop, fmt)
        for B in (8, 16, 32, 64):
            for ssim in (True, False):
                m = mmap.picture(a, b, fmt, (10, 10), B, ssim=ssim, crop=crop)
                assert m.shape == (3, 6 if ssim else 4) + mmap.grid(W - crop[0] - crop[1], H - crop[2] - crop[3], B)[::-1]
                for k in range(3):
                    if k and fmt == 0:
                        assert not m[k].any()
                        continue
                    want = mref.plane(ca[k], cb[k], 10, ssim)
                    for f, name in enumerate(mmap.FIELDS[:m.shape[1]]):
                        got = int(m[k, f].max()) if name == "max_abs" else int(m[k, f].sum())
                        assert got == want[name], (fmt, crop, B, k, name)
                    assert int(mmap.samples(W - crop[0] - crop[1], H - crop[2] - crop[3], fmt, B, k).sum()) == want["samples"]


def test_a_single_differing_sample_at_8_8():
    """B = 8: the sample is the first of block (1, 1), which alone holds its distortion; the windows that cover it start at (4, 4),
    (8, 4), (4, 8), (8, 8), (0 .. 8, 0 .. 8) -- top-left samples in blocks (0, 0), (1, 0), (0, 1) and (1, 1), and in no other"""
    rng = np.random.RandomState(2)
    a = rng.randint(0, 1024, size=(48, 64))
    b = a.copy()
    b[8, 8] ^= 256
    m = mmap.plane(a, b, 10, 8, 8, 8, 6)
    for f, v in ((0, 256 * 256), (1, 256), (2, 1), (3, 256)):
        want = np.zeros((6, 8), np.int64)
        want[1, 1] = v
        assert np.array_equal(m[f], want)
    below = m[4] < (m[5] << 32)
    want = np.zeros((6, 8), bool)
    want[0:2, 0:2] = True
    assert np.array_equal(below, want)
    assert np.array_equal(m[4][~want], m[5][~want] << 32)              # everywhere else: identical windows, exactly 2^32 each
    assert m[5][0, 0] == 4 and m[5][5, 7] == 1 and int(m[5].sum()) == mref.windows(64, 48)
