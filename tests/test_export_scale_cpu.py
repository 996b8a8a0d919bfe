"""Scaled device export, host side (no GPU): hmgpu_export_scaled_plan_for's validation and geometry, the resampling tables
hmgpu_export_scale_taps publishes against torch's own weights, the overflow bound of the integer arithmetic, and the numpy
restatement (tests/scale_ref.py) against torch's floating-point interpolation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import export_ref as ref
from tests import scale_ref as sref

FILTERS = [abi.SCALE_NEAREST, abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA]
TORCH_MODE = {abi.SCALE_NEAREST: dict(mode="nearest-exact"), abi.SCALE_BILINEAR: dict(mode="bilinear", antialias=True, align_corners=False),
              abi.SCALE_BICUBIC: dict(mode="bicubic", antialias=True, align_corners=False), abi.SCALE_AREA: dict(mode="area")}
EINVAL, EUNSUPPORTED = 1, 3


def seq_of(w, h, fmt, bd_y, bd_c=None):
    s = abi.make_seq(w, h, bd_y, bd_c if bd_c is not None else bd_y)
    s.chroma_format = fmt
    return s


def plan_status(seq, desc, scale):
    plan = abi.ExportPlan()
    st = libhm_amd.lib().hmgpu_export_scaled_plan_for(C.byref(seq), C.byref(desc), C.byref(scale), C.byref(plan))
    return st, plan


def torch_weights(n_in, n_out, filt):
    """torch's float64 weights, [out, in]: unit impulses through F.interpolate"""
    import torch
    import torch.nn.functional as F
    eye = torch.eye(n_in, dtype=torch.float64).reshape(n_in, 1, 1, n_in)
    return F.interpolate(eye, size=(1, n_out), **TORCH_MODE[filt]).reshape(n_in, n_out).numpy().T


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ref.PLANAR, ref.SEMIPLANAR, ref.RGB])
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("crop,size", [((0, 0, 0, 0), (60, 104)), ((4, 8, 2, 6), (300, 400)), ((0, 0, 0, 0), (31, 57))])
def test_plan_geometry(fmt, layout, filt, crop, size):
    """every plane resized; chroma planes by the format's subsampling; odd sizes only where no chroma plane is written"""
    seq = seq_of(208, 120, fmt, 10)
    desc = abi.make_export_desc(layout, 10, 2, 1, crop, 1, 0)
    scale = sref.scale_of(size, filt)
    st, plan = plan_status(seq, desc, scale)
    sx, sy = ref.chroma_shift(fmt)
    odd = (size[1] & ((1 << sx) - 1)) or (size[0] & ((1 << sy) - 1))
    if layout != ref.RGB and fmt != 0 and odd:
        assert st == EINVAL
        return
    assert st == 0
    base = libhm_amd.export_plan(seq, desc)
    assert plan.planes == base.planes
    h, w = size
    for k in range(plan.planes):
        cw, ch = (w, h) if k == 0 or layout == ref.RGB else (w >> sx, h >> sy)
        assert (plan.width[k], plan.height[k]) == (cw, ch)
        assert plan.row_bytes[k] == cw * 2 * (2 if layout == ref.SEMIPLANAR and k == 1 else 1)
    assert list(plan.coef[:11]) == list(base.coef[:11])
    assert plan.coef[11] == 16 - 10 and plan.coef[12] >= 1 and plan.coef[13] >= 1 and plan.coef[14] == plan.coef[15] == 0


@pytest.mark.parametrize("layout", [ref.PLANAR, ref.SEMIPLANAR])
def test_e_takes_the_larger_yuv_depth(layout):
    """YUV layouts with different luma and chroma output depths keep E = 16 - max of the two (one E per export)"""
    for fmt, bd in itertools.product((0, 1, 3), [(10, 8), (8, 12), (16, 9)]):
        seq = seq_of(208, 120, fmt, 10)
        desc = abi.make_export_desc(layout, bd, 2, 0, (0, 0, 0, 0), 1, 0)
        plan = libhm_amd.export_scaled_plan(seq, desc, sref.scale_of((60, 104), abi.SCALE_BICUBIC))
        assert plan.coef[11] == 16 - (bd[0] if fmt == 0 else max(bd)), (fmt, bd)


def test_refusals():
    seq = seq_of(208, 120, 1, 10)
    good = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    assert plan_status(seq, good, sref.scale_of((60, 104), abi.SCALE_BICUBIC))[0] == 0
    for size in [(61, 104), (60, 103), (0, 104), (60, 0), (-2, 104)]:
        assert plan_status(seq, good, sref.scale_of(size, abi.SCALE_BILINEAR))[0] == EINVAL, size
    for filt in (-1, 4):
        assert plan_status(seq, good, sref.scale_of((60, 104), filt))[0] == EINVAL
    for k in range(5):
        s = sref.scale_of((60, 104), abi.SCALE_AREA)
        s.reserved[k] = 1
        assert plan_status(seq, good, s)[0] == EINVAL
    bad = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (1, 0, 0, 0), 1, 0)            # the descriptor is validated as unscaled
    assert plan_status(seq, bad, sref.scale_of((60, 104), abi.SCALE_AREA))[0] == EINVAL
    rgb = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    for size in [(3, 208), (120, 6), (961, 208), (120, 1666), (16386, 2048)]:       # beyond 32x down / 8x up / 16384
        assert plan_status(seq, rgb, sref.scale_of(size, abi.SCALE_BILINEAR))[0] == EUNSUPPORTED, size
    for size in [(4, 7), (960, 1664), (57, 31)]:                                    # at the limits, odd RGB sizes
        assert plan_status(seq, rgb, sref.scale_of(size, abi.SCALE_BICUBIC))[0] == 0, size
    big = seq_of(4096, 2304, 1, 10)
    assert plan_status(big, rgb, sref.scale_of((16384, 16384), abi.SCALE_NEAREST))[0] == 0
    assert plan_status(big, rgb, sref.scale_of((16384, 16386), abi.SCALE_NEAREST))[0] == EUNSUPPORTED
    # the taps entry point: a chroma class that does not exist, too few taps
    scale = sref.scale_of((60, 104), abi.SCALE_BICUBIC)
    f, c = np.zeros(104, np.int32), np.zeros(104, np.int32)
    w = np.zeros((104, 64), np.int16)
    args = lambda ch, taps: (C.byref(seq), C.byref(rgb), C.byref(scale), ch, 0, taps, f.ctypes.data_as(C.POINTER(C.c_int32)),
                             c.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_int16)))
    assert libhm_amd.lib().hmgpu_export_scale_taps(*args(0, 64)) == 0
    assert libhm_amd.lib().hmgpu_export_scale_taps(*args(1, 64)) == EINVAL
    assert libhm_amd.lib().hmgpu_export_scale_taps(*args(0, 1)) == EINVAL


# (in, out) along one axis: reductions up to 32x, enlargements up to 8x, equal size, odd sizes
AXES = [(208, 208), (208, 104), (208, 57), (208, 7), (3840, 120), (2160, 68), (1920, 224), (1080, 224), (120, 960), (13, 104), (97, 143),
        (1, 1), (5, 1), (32, 1)]


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n_in,n_out", AXES)
def test_tables(filt, n_in, n_out):
    """sum 16384, inside the plane, the identity at equal size, within one Q14 unit of torch's float64 weights"""
    seq = seq_of(n_in, 8, 0, 8)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    first, count, w = libhm_amd.export_scale_taps(seq, desc, sref.scale_of((8, n_out), filt), 0, 0)
    assert (w.astype(np.int64).sum(axis=1) == 16384).all()
    assert (first >= 0).all() and (count >= 1).all() and (first + count <= n_in).all()
    for i in range(n_out):
        assert (w[i, count[i]:] == 0).all() and w[i, 0] != 0 and w[i, count[i] - 1] != 0
    if n_in == n_out:
        assert (first == np.arange(n_in)).all() and (count == 1).all() and (w[:, 0] == 16384).all()
    if filt == abi.SCALE_NEAREST:
        assert_nearest(n_in, n_out, first)
        return
    got = sref.matrix((first, count, w), n_in) / 16384.0
    assert np.abs(got - torch_weights(n_in, n_out, filt)).max() <= 1.0 / 16384 + 1e-12


def nearest_table(n_in, n_out):
    seq = seq_of(n_in, 8, 0, 8)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    return libhm_amd.export_scale_taps(seq, desc, sref.scale_of((8, n_out), abi.SCALE_NEAREST), 0, 0)


def assert_nearest(n_in, n_out, first, against_torch=True):
    """one tap at the exact source index floor((2i + 1) * in / (2 * out)); torch's nearest-exact agrees except at exact ties, where
    its float32 arithmetic may give the index one below"""
    i = np.arange(n_out, dtype=np.int64)
    exact = np.minimum((2 * i + 1) * n_in // (2 * n_out), n_in - 1)
    assert np.array_equal(first, exact), (n_in, n_out, np.nonzero(first != exact)[0][:5])
    if against_torch:
        t = torch_weights(n_in, n_out, abi.SCALE_NEAREST).argmax(axis=1)
        off = np.nonzero(t != exact)[0]
        tie = (2 * off + 1) * n_in % (2 * n_out) == 0
        assert tie.all() and (t[off] == exact[off] - 1).all(), (n_in, n_out, off[:5])


def test_nearest_exhaustive_and_against_torch():
    """every (in, out) up to 160 within the limits against the exact index; random pairs up to 4096 also against torch"""
    for n_in in range(1, 161):
        for n_out in range(1, 161):
            if n_in <= 32 * n_out and n_out <= 8 * n_in:
                first, count, w = nearest_table(n_in, n_out)
                assert (count == 1).all() and (w[:, 0] == 16384).all()
                assert_nearest(n_in, n_out, first, against_torch=False)
    rng = np.random.default_rng(11)
    pairs = [(678, 123), (1920, 224), (3840, 120), (2160, 68), (128, 107), (310, 35)]
    while len(pairs) < 400:
        n_in, n_out = int(rng.integers(1, 4097)), int(rng.integers(1, 2049))
        if n_in <= 32 * n_out and n_out <= 8 * n_in:
            pairs.append((n_in, n_out))
    for n_in, n_out in pairs:
        assert_nearest(n_in, n_out, nearest_table(n_in, n_out)[0])


def test_chroma_tables_follow_the_plane():
    """the chroma class of 4:2:0 / 4:2:2 resamples the chroma plane's own sizes, with a crop"""
    desc = abi.make_export_desc(ref.PLANAR, 8, 1, 0, (4, 8, 2, 6), 1, 0)
    for fmt in (1, 2, 3):
        seq = seq_of(208, 120, fmt, 8)
        sx, sy = ref.chroma_shift(fmt)
        scale = sref.scale_of((56, 100), abi.SCALE_BICUBIC)
        for ax, (n_in, n_out) in enumerate([(196 >> sx, 100 >> sx), (112 >> sy, 56 >> sy)]):
            first, count, w = libhm_amd.export_scale_taps(seq, desc, scale, 1, ax)
            assert len(first) == n_out and (first + count <= n_in).all()
            assert np.abs(sref.matrix((first, count, w), n_in) / 16384.0 - torch_weights(n_in, n_out, abi.SCALE_BICUBIC)).max() <= 1.0 / 16384 + 1e-12


def sums_bound(tx, ty, depth, e):
    """the extremes of every 32-bit sum of the integer arithmetic over all inputs 0 .. 2^depth - 1"""
    wx, wy = tx[2].astype(np.int64), ty[2].astype(np.int64)
    v = (1 << depth) - 1
    hmax = (np.clip(wx, 0, None).sum(axis=1) * v).max() + (1 << (13 - e))
    hmin = (np.clip(wx, None, 0).sum(axis=1) * v).min() + (1 << (13 - e))
    tmax, tmin = hmax >> (14 - e), hmin >> (14 - e)
    pos, neg = np.clip(wy, 0, None).sum(axis=1), -np.clip(wy, None, 0).sum(axis=1)
    vmax = (pos * tmax + neg * max(-tmin, 0)).max() + (1 << (13 + e))
    vmin = (-(pos * max(-tmin, 0) + neg * tmax)).min() + (1 << (13 + e))
    return max(hmax, vmax), min(hmin, vmin)


def row_sums(n_in, n_out, filt):
    """the largest row sum of positive weights and of negative weights' magnitudes of one table"""
    seq = seq_of(n_in, 8, 0, 8)
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    w = libhm_amd.export_scale_taps(seq, desc, sref.scale_of((8, n_out), filt), 0, 0)[2].astype(np.int64)
    return np.clip(w, 0, None).sum(axis=1).max(), -np.clip(w, None, 0).sum(axis=1).min()


@pytest.mark.parametrize("filt", FILTERS)
def test_no_overflow_for_every_small_table(filt):
    """every table with in, out <= 128 within the limits: the largest positive and negative row sums over all of them, taken as the
    horizontal and the vertical table at once (every sum grows with them), keep both passes inside 32 bits at every depth"""
    pos = neg = 0
    for n_in in range(1, 129):
        for n_out in range(1, 129):
            if n_in <= 32 * n_out and n_out <= 8 * n_in:
                p, n = row_sums(n_in, n_out, filt)
                pos, neg = max(pos, p), max(neg, n)
    for depth in range(8, 17):
        e, v = 16 - depth, (1 << depth) - 1
        hmax, hmin = pos * v + (1 << (13 - e)), -neg * v + (1 << (13 - e))
        tmax, tmin = hmax >> (14 - e), hmin >> (14 - e)
        vmax = pos * tmax + neg * max(-tmin, 0) + (1 << (13 + e))
        vmin = -(pos * max(-tmin, 0) + neg * tmax) + (1 << (13 + e))
        assert hmax < 2 ** 31 and hmin >= -2 ** 31 and vmax < 2 ** 31 and vmin >= -2 ** 31, (depth, pos, neg)


@pytest.mark.parametrize("filt", FILTERS)
def test_no_overflow_within_the_limits(filt):
    """larger tables, sampled: the ends of the range (32x reduction, 8x enlargement) and ratios between, every output depth; the
    host also evaluates this bound for the tables of each shape and refuses one that would overflow"""
    ratios = [(32 * n, n) for n in (1, 3, 7, 60)] + [(n, 8 * n) for n in (1, 3, 7, 300)] + \
             [(i, j) for i in (31, 64, 100, 129, 1920, 3840) for j in (5, 9, 17, 40, 77, 130, 224, 1080) if j <= 8 * i and i <= 32 * j]
    for (n_in, n_out), depth in itertools.product(ratios, range(8, 17)):
        seq = seq_of(n_in, n_in, 3, 8)
        desc = abi.make_export_desc(ref.RGB, depth, 2 if depth > 8 else 1, 0, (0, 0, 0, 0), 1, 0)
        scale = sref.scale_of((n_out, n_out), filt)
        plan = libhm_amd.export_scaled_plan(seq, desc, scale)
        e = plan.coef[11]
        assert e == 16 - depth
        t = libhm_amd.export_scale_taps(seq, desc, scale, 0, 0)
        hi, lo = sums_bound(t, t, depth, e)
        assert hi < 2 ** 31 and lo >= -2 ** 31, (n_in, n_out, depth)


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("layout", [ref.PLANAR, ref.RGB])
@pytest.mark.parametrize("size", [(36, 100), (50, 70), (180, 300)])
def test_restatement_tracks_torch(filt, layout, size):
    """the integer restatement stays within one code value of torch interpolating the unscaled export in float64"""
    import torch
    import torch.nn.functional as F
    w, h, fmt, bd = 200, 72, 1, (10, 10)
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 1 << bd[0], (h, w)).astype(np.int16)] + [rng.integers(0, 1 << bd[1], (h // 2, w // 2)).astype(np.int16) for _ in range(2)]
    seq = seq_of(w, h, fmt, bd[0])
    desc = abi.make_export_desc(layout, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    scale = sref.scale_of(size, filt)
    plan = libhm_amd.export_scaled_plan(seq, desc, scale)
    got = sref.export_scaled(planes, fmt, bd, desc, plan, sref.tables(seq, desc, scale))
    if layout == ref.RGB:
        src = [np.asarray(p) for p in ref.export_rgb(planes, fmt, bd, 8, list(plan.coef))]
    else:
        src = ref.export_yuv(planes, fmt, bd, (8, 8), ref.PLANAR)
    for k, (s, g) in enumerate(zip(src, got)):
        x = torch.from_numpy(np.asarray(s, np.float64))[None, None]
        f = F.interpolate(x, size=g.shape, **TORCH_MODE[filt])[0, 0].numpy()
        want = np.clip(np.round(f), 0, 255)
        assert np.abs(np.asarray(g, np.int64) - want).max() <= 1, (k, np.abs(np.asarray(g, np.int64) - want).max())
