"""The residual export without a GPU: the numpy model (tests/residual_ref.py) held against the C oracle's reconstruction and against
HM's own arrays, the plan function with every refusal, the dense model, and the struct mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, residual
from tests import golden_util as gu
from tests import residual_ref as rref
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def levels_of(p):
    return p.coeffs.arrays


def flat_planes(seq):
    """planes flat at half range (4:0:0 keeps 4:2:0-shaped chroma planes)"""
    return [np.full((seq.height, seq.width), 1 << (seq.bit_depth_luma - 1), dtype=np.int16),
            np.full((seq.height // 2, seq.width // 2), 1 << (seq.bit_depth_chroma - 1), dtype=np.int16),
            np.full((seq.height // 2, seq.width // 2), 1 << (seq.bit_depth_chroma - 1), dtype=np.int16)]


# ------------------------------------------------------------------------------------------------ 1. inter: reconstruction - flat prediction
# Levels of -3 .. 3 at QP 10 .. 20 keep the residual far inside +-2^(bd - 1) at every depth (checked below: at most 1 % of a plane's
# samples may sit at 0 or the maximum, where a clipped sum cannot tell two residuals apart).
@pytest.mark.parametrize("bd,log2_ctu,fmt,bi", [(8, 6, 1, False), (10, 5, 1, True), (12, 4, 1, True), (10, 6, 0, True), (8, 4, 1, False), (12, 6, 1, False)])
def test_inter_reconstruction_is_flat_prediction_plus_model(oracle, bd, log2_ctu, fmt, bi):
    """every reference plane flat at 1 << (bd - 1): the interpolation taps sum to 64 and weighted prediction is off, so every
    prediction is that constant and the oracle's reconstruction is clip(constant + residual) on every sample"""
    w, h = 416, 240
    p = synth.make_picture(w, h, bd, seed=0xE51D + bd + log2_ctu + fmt, bi=bi, intra_frac=0.0, num_refs=2, ref_handles=([0, 1], [1]),
                           chroma_format=fmt, log2_ctu=log2_ctu, coef_dist="dense", slice_qp_range=(10, 20), cbf_prob=0.6, sao=False,
                           tr_depth_max=3, part_probs=(0.4, 0.2, 0.2, 0.2))
    flat = flat_planes(p.seq)
    rec = [np.zeros_like(a) for a in flat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [flat, flat])
    model = rref.planes(p.seq, p.slices, p.meta_np, levels_of(p))
    sizes = set()
    for comp in range(1 if fmt == 0 else 3):
        maxv = (1 << bd) - 1
        want = np.clip(flat[comp].astype(np.int64) + model[comp], 0, maxv)
        assert np.array_equal(rec[comp], want), comp
        assert model[comp].any()
        clipped = np.mean((rec[comp] == 0) | (rec[comp] == maxv))
        assert clipped <= 0.01, (comp, clipped)
    for comp, a, off, size, z in rref.block_list(p.seq, p.meta_np):
        sizes.add((comp > 0, size))
    assert {s for c, s in sizes if not c} >= ({4, 8, 16, 32} if log2_ctu > 4 else {4, 8, 16})
    if fmt:
        assert {s for c, s in sizes if c} >= {4, 8}
        assert not model[1][~synth_block_cover(p, 1)].any()
    assert not model[0][~synth_block_cover(p, 0)].any()


def synth_block_cover(p, comp):
    """True where a block of coded_blocks() covers a sample of the component"""
    seq = p.seq
    ctu, parts = 1 << seq.log2_ctu_size, 1 << (2 * seq.log2_ctu_size - 4)
    cw = (seq.width + ctu - 1) // ctu
    zx, zy = rref._zxy(parts)
    s = 1 if comp else 0
    mask = np.zeros((seq.height >> s, seq.width >> s), dtype=bool)
    for c, a, off, size in synth.coded_blocks(p.meta_np, seq.chroma_format, seq.log2_ctu_size):
        if c != comp:
            continue
        z = off // 16 if c == 0 else off // 4
        x0, y0 = ((a % cw) * ctu + 4 * zx[z]) >> s, ((a // cw) * ctu + 4 * zy[z]) >> s
        mask[y0:y0 + size, x0:x0 + size] = True
    return mask


# ------------------------------------------------------------------------------------------------ 2. intra: the first TU of a slice
def _first_tu_blocks(p, model, rec, flat):
    """per slice and component: the coded block at the slice's first partition; the oracle's reconstruction there must be
    clip(constant + model).  Returns the (component, size, transform skip) of the blocks seen"""
    seq = p.seq
    ctu = 1 << seq.log2_ctu_size
    cw = (seq.width + ctu - 1) // ctu
    seen = []
    blocks = rref.block_list(seq, p.meta_np)
    for first, _ in p.slice_ranges:
        for comp, a, off, size, z in blocks:
            if a != first or z != 0:
                continue
            s = 1 if comp else 0
            x0, y0 = ((a % cw) * ctu) >> s, ((a // cw) * ctu) >> s
            bd = seq.bit_depth_chroma if comp else seq.bit_depth_luma
            want = np.clip(flat[comp][y0:y0 + size, x0:x0 + size].astype(np.int64) + model[comp][y0:y0 + size, x0:x0 + size], 0, (1 << bd) - 1)
            assert np.array_equal(rec[comp][y0:y0 + size, x0:x0 + size], want), (first, comp, size)
            assert model[comp][y0:y0 + size, x0:x0 + size].any()
            seen.append((comp, size))
    return seen


INTRA_CASES = [((1, 0, 0, 0, 0), 0.0, "plain"), ((0, 1, 0, 0, 0), 0.0, "plain"), ((0, 0, 1, 0, 0), 0.0, "plain"), ((0, 0, 0, 1, 0), 1.0, "plain"),
               ((0, 0.3, 0.4, 0.3, 0), 0.5, "lists"), ((0, 0.3, 0.4, 0.3, 0), 0.5, "rdpcm")]


@pytest.mark.parametrize("mode_probs,split,kind", INTRA_CASES)
def test_intra_first_tu_of_a_slice_is_flat_prediction_plus_model(oracle, mode_probs, split, kind):
    """an intra CU that opens a slice has no neighbour: every reference sample is substituted by 1 << (bd - 1) and the prediction of its
    first TU is flat whatever the mode.  CU sizes 64 .. 8 give first TUs of 32x32, 32 / 16, 16 / 8 and 4x4 (DST); one case with an intra
    scaling list on every list id, one with transform skip + implicit RDPCM (modes 10 / 26) + rotation"""
    w, h, bd = 416, 240, 8
    p = synth.make_picture(w, h, bd, seed=0x1A7A + int(10 * split) + len(kind), intra_frac=1.0, mode_probs=mode_probs, tr_split_prob=split,
                           cbf_prob=1.0, coef_dist="dense", slice_qp_range=(10, 20), sao=False, ref_handles=([0], [0]), num_slices=9)
    if kind == "lists":
        rng = np.random.RandomState(5)
        lists = abi.ScalingLists()
        for sz in range(4):
            for l in range(6):
                lists.dc[sz][l] = int(rng.randint(8, 40)) if sz >= 2 else 16
                for i in range(64):
                    lists.coef[sz][l][i] = int(rng.randint(8, 40)) if i < (16 if sz == 0 else 64) else 16
        p.keep = lists
        for sl in p.slices:
            sl.scaling_lists = C.pointer(lists)
    if kind == "rdpcm":
        p.seq.range_ext_flags = 3                                      # rotation + implicit RDPCM
        m = dict(p.meta_np)
        m["ts_y"] = np.ones_like(m["depth"]).astype(np.uint8)
        m["ts_u"] = np.ones_like(m["depth"]).astype(np.uint8)
        m["intra_dir_l"] = np.where((np.arange(m["depth"].shape[0]) % 2 == 0)[:, None], 10, 26).astype(np.uint8) * np.ones_like(m["depth"]).astype(np.uint8)
        p.meta_np = m
        p.meta = abi.MetaHolder(m)
    flat = flat_planes(p.seq)
    rec = [np.zeros_like(a) for a in flat]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [flat])
    model = rref.planes(p.seq, p.slices, p.meta_np, levels_of(p))
    seen = _first_tu_blocks(p, model, rec, flat)
    luma = {s for c, s in seen if c == 0}
    assert len(seen) >= 9 and luma, seen
    want = {(1, 0, 0, 0, 0): {32}, (0, 1, 0, 0, 0): {32}, (0, 0, 1, 0, 0): {16}, (0, 0, 0, 1, 0): {4}}.get(mode_probs)
    if want:
        assert luma >= want, (luma, want)
    if kind == "rdpcm":
        # the tools change the block: the same arrays without them give another residual
        p.seq.range_ext_flags = 0
        plain = rref.planes(p.seq, p.slices, p.meta_np, levels_of(p))
        assert any(not np.array_equal(a, b) for a, b in zip(plain, model))
    if kind == "lists":
        flatq = [abi.clone_slice(sl) for sl in p.slices]
        for sl in flatq:
            sl.scaling_lists = None
        assert any(not np.array_equal(a, b) for a, b in zip(rref.planes(p.seq, flatq, p.meta_np, levels_of(p)), model))


def test_intra_cases_cover_every_transform_size():
    """the sizes the intra cases above reach at a slice's first partition, over all of them: 4 (DST), 8, 16 and 32"""
    sizes = set()
    for mode_probs, split, kind in INTRA_CASES:
        p = synth.make_picture(416, 240, 8, seed=0x1A7A + int(10 * split) + len(kind), intra_frac=1.0, mode_probs=mode_probs, tr_split_prob=split,
                               cbf_prob=1.0, coef_dist="dense", slice_qp_range=(10, 20), sao=False, ref_handles=([0], [0]), num_slices=9)
        firsts = {a for a, _ in p.slice_ranges}
        sizes |= {size for comp, a, off, size, z in rref.block_list(p.seq, p.meta_np) if comp == 0 and z == 0 and a in firsts}
    assert sizes >= {4, 8, 16, 32}, sizes


# ------------------------------------------------------------------------------------------------ 3. / 4. HM's fixtures
def test_lossless_fixture_residual_is_the_levels():
    """cu_transquant_bypass everywhere: the residual of a coded block is its level block (no RDPCM / rotation in this stream)"""
    pics = gu.stream_pictures("ldp_lossless_main10_208x120")
    checked = 0
    for p in pics[:3]:
        assert p.meta_np["bypass"][p.meta_np["part_size"] != abi.SIZE_NONE].all() and p.seq.range_ext_flags & 7 == 0
        model = rref.planes(p.seq, p.slices, p.meta_np, p.coeffs.arrays)
        ctu, parts = p.ctu_size, p.parts
        zx, zy = rref._zxy(parts)
        for comp, a, off, size, z in rref.block_list(p.seq, p.meta_np):
            s = 1 if comp else 0
            x0, y0 = ((a % p.ctus_w) * ctu + 4 * zx[z]) >> s, ((a // p.ctus_w) * ctu + 4 * zy[z]) >> s
            lev = p.coeffs.arrays[comp].reshape(p.num_ctus, -1)[a, off:off + size * size].reshape(size, size)
            got = model[comp][y0:y0 + size, x0:x0 + size]
            assert np.array_equal(got, lev[:got.shape[0], :got.shape[1]])
            checked += 1
    assert checked > 50


@pytest.mark.parametrize("name", gu.STREAMS)
def test_model_is_zero_outside_the_coded_blocks_of_hm_fixtures(name):
    """the twelve HM metadata fixtures: nothing outside coded_blocks(); PCM CUs are zero although HM flags them; and on inter pictures
    whose pre-deblocking planes are kept, reconstruction - model stays inside the sample range (the model is a residual of that picture)"""
    pics = gu.stream_pictures(name)
    some = False
    for p in pics[:4]:
        model = rref.planes(p.seq, p.slices, p.meta_np, p.coeffs.arrays)
        for comp in range(3):
            cover = synth_block_cover(p, comp)
            assert not model[comp][~cover].any(), (name, p.index, comp)
            some |= bool(model[comp].any())
        ipcm = p.meta_np["ipcm"]
        if ipcm.any():
            zx, zy = rref._zxy(p.parts)
            a, z = np.nonzero(ipcm != 0)
            for ai, zi in zip(a[:200], z[:200]):
                x0, y0 = (ai % p.ctus_w) * p.ctu_size + 4 * zx[zi], (ai // p.ctus_w) * p.ctu_size + 4 * zy[zi]
                if x0 < p.width and y0 < p.height:
                    assert not model[0][y0:y0 + 4, x0:x0 + 4].any() and not model[1][y0 // 2:y0 // 2 + 2, x0 // 2:x0 // 2 + 2].any()
    assert some, name
    if name == "ldp_pcm_main8_208x120":
        assert any(p.meta_np["ipcm"].any() for p in pics)


# ------------------------------------------------------------------------------------------------ 5. the plan
def _seq(fmt=1, w=200, h=120, log2_ctu=6):
    s = abi.make_seq(w, h, 10, 10, log2_ctu=log2_ctu)
    s.chroma_format = fmt
    return s


def _status(seq, desc, scale=None, windows=None, n=None):
    try:
        residual.plan_for(seq, desc, scale, windows, n)
    except libhm_amd.HmgpuError as e:
        return e.status
    return abi.HMGPU_OK


def _win(seq, xywh, flip=False):
    x, y, w, h = xywh
    return abi.make_export_window((x, seq.width - x - w, y, seq.height - y - h), flip)


def test_plan_shapes():
    seq = _seq()
    p = libhm_amd.residual_plan(seq, "planes")
    assert list(p.channels) == [1, 1, 1] and list(p.width) == [200, 100, 100] and list(p.height) == [120, 60, 60]
    assert list(p.elem_bytes) == [2, 2, 2] and list(p.row_bytes) == [400, 200, 200]
    p = libhm_amd.residual_plan(seq, "planes", (0, 2), crop=(8, 16, 24, 0))
    assert list(p.channels) == [1, 0, 1] and list(p.width) == [176, 0, 88] and list(p.height) == [96, 0, 48]
    p = libhm_amd.residual_plan(_seq(0), "planes")
    assert list(p.channels) == [1, 0, 0] and list(p.width) == [200, 0, 0]
    for st, es in ((abi.SAMPLE_UINT, 2), (abi.SAMPLE_F16, 2), (abi.SAMPLE_BF16, 2), (abi.SAMPLE_F32, 4)):
        p = libhm_amd.residual_plan(seq, "dense", (0, 1, 2), size=(64, 48), windows=[(36, 20, 96, 64), (2, 6, 8, 8)], dtype=st)
        assert list(p.channels) == [3, 0, 0] and (p.width[0], p.height[0], p.elem_bytes[0], p.row_bytes[0]) == (48, 64, es, 48 * es)
    p = libhm_amd.residual_plan(seq, "dense", (1,), windows=[(0, 0, 96, 64), (104, 56, 96, 64)], flip=[False, True])
    assert list(p.channels) == [1, 0, 0] and (p.width[0], p.height[0]) == (96, 64)


def test_plan_refusals_match_the_header():
    seq = _seq()
    E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    planes = lambda **kw: abi.make_residual_desc(abi.RESIDUAL_PLANES, kw.pop("components", 7), kw.pop("sample_type", abi.SAMPLE_UINT), kw.pop("crop", (0, 0, 0, 0)))
    dense = lambda st=abi.SAMPLE_F16, comps=7, scale=(1.0, 1.0, 1.0): abi.make_residual_desc(abi.RESIDUAL_DENSE, comps, st, scale=scale)
    whole = [_win(seq, (0, 0, 200, 120))]
    nearest = abi.make_export_scale(64, 64, abi.SCALE_NEAREST)
    assert _status(seq, planes()) == abi.HMGPU_OK and _status(seq, dense(), nearest, whole) == abi.HMGPU_OK
    assert _status(seq, dense(abi.SAMPLE_UINT), nearest, whole) == abi.HMGPU_OK
    # 4:2:2 / 4:4:4: not supported, whatever else the call says; 4:0:0 is
    for fmt in (2, 3):
        assert _status(_seq(fmt), planes()) == U and _status(_seq(fmt), dense(), nearest, whole) == U
    assert _status(_seq(0), planes()) == abi.HMGPU_OK
    # a crop that is no multiple of 8, negative, or empty
    for crop in ((4, 0, 0, 0), (0, 12, 0, 0), (0, 0, 2, 0), (0, 0, 0, 4), (-8, 0, 0, 0), (104, 96, 0, 0)):
        assert _status(seq, planes(crop=crop)) == E, crop
    # component mask, form, reserved words, n
    assert _status(seq, planes(components=0)) == E and _status(seq, planes(components=8)) == E
    d = planes(); d.form = 2
    assert _status(seq, d) == E
    for k in range(6):
        d = planes(); d.reserved[k] = 1
        assert _status(seq, d) == E
        d = dense(); d.reserved[k] = 1
        assert _status(seq, d, nearest, whole) == E
    assert _status(seq, planes(), n=0) == E and _status(seq, planes(), n=17) == E and _status(seq, planes(), n=16) == abi.HMGPU_OK
    assert _status(seq, dense(), nearest, whole * 17) == E and _status(seq, dense(), nearest, whole, n=0) == E
    # PLANES takes neither a scale nor windows nor a float type; DENSE needs windows and no crop, a known type and finite scales
    assert _status(seq, planes(), nearest) == E and _status(seq, planes(), None, whole) == E and _status(seq, planes(sample_type=abi.SAMPLE_F16)) == E
    assert _status(seq, dense(), nearest, None, n=1) == E
    d = dense(); d.crop[0] = 8
    assert _status(seq, d, nearest, whole) == E
    assert _status(seq, dense(4), nearest, whole) == E
    assert _status(seq, dense(scale=(1.0, float("inf"), 1.0)), nearest, whole) == E
    assert _status(seq, dense(comps=1, scale=(1.0, float("nan"), 1.0)), nearest, whole) == abi.HMGPU_OK      # (a component that is not selected)
    # filters other than nearest: not supported; an unknown filter code or a reserved word of the scale: invalid
    for f in (abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
        assert _status(seq, dense(), abi.make_export_scale(64, 64, f), whole) == U
    assert _status(seq, dense(), abi.make_export_scale(64, 64, 7), whole) == E
    s = abi.make_export_scale(64, 64, abi.SCALE_NEAREST); s.reserved[2] = 1
    assert _status(seq, dense(), s, whole) == E
    # windows
    w = _win(seq, (0, 0, 96, 64)); w.flip = 2
    assert _status(seq, dense(), nearest, [w]) == E
    w = _win(seq, (0, 0, 96, 64)); w.reserved[1] = 1
    assert _status(seq, dense(), nearest, [w]) == E
    assert _status(seq, dense(), nearest, [_win(seq, (150, 0, 96, 64))]) == E
    assert _status(seq, dense(), nearest, [_win(seq, (3, 0, 96, 64))]) == E and _status(_seq(0), dense(), nearest, [_win(seq, (3, 1, 96, 64))]) == abi.HMGPU_OK
    assert _status(seq, dense(), None, [_win(seq, (0, 0, 96, 64)), _win(seq, (4, 4, 96, 60))]) == E
    assert _status(seq, dense(), None, [_win(seq, (0, 0, 96, 64)), _win(seq, (6, 2, 96, 64))]) == abi.HMGPU_OK
    # the limits of the scaled export, per window
    assert _status(seq, dense(), abi.make_export_scale(6, 2, 0), [_win(seq, (4, 2, 192, 64))]) == abi.HMGPU_OK
    assert _status(seq, dense(), abi.make_export_scale(6, 2, 0), [_win(seq, (4, 2, 194, 64))]) == U
    assert _status(seq, dense(), abi.make_export_scale(64, 64, 0), [_win(seq, (2, 6, 8, 8))]) == abi.HMGPU_OK
    assert _status(seq, dense(), abi.make_export_scale(66, 64, 0), [_win(seq, (2, 6, 8, 8))]) == U
    big = _seq(w=4096, h=2304)
    assert _status(big, dense(), abi.make_export_scale(16386, 64, 0), [_win(big, (0, 0, 4096, 2304))]) == U
    # the python layer's own refusals
    with pytest.raises(ValueError):
        libhm_amd.residual_plan(seq, "planes", size=(8, 8))
    with pytest.raises(ValueError):
        libhm_amd.residual_plan(seq, "nope")
    with pytest.raises(ValueError):
        libhm_amd.residual_plan(seq, "dense", scale=(2.0, 2.0, 2.0))          # a scale without a float type


# ------------------------------------------------------------------------------------------------ 6. the dense model
def _picture():
    return synth.make_picture(200, 120, 10, seed=77, bi=True, num_refs=2, intra_frac=0.3, ref_handles=([0, 1], [1]), tr_depth_max=2)


def test_dense_at_the_windows_own_size_is_the_planes_with_chroma_replicated():
    p = _picture()
    pl = rref.planes(p.seq, p.slices, p.meta_np, levels_of(p))
    d = rref.dense(pl, (0, 0, 200, 120), False, (120, 200))
    assert np.array_equal(d[0], pl[0])
    for c in (1, 2):
        assert np.array_equal(d[c], np.repeat(np.repeat(pl[c], 2, axis=0), 2, axis=1))
    assert all(a.any() for a in pl)
    # a window at its own size is the crop
    d = rref.dense(pl, (36, 20, 96, 64), False, (64, 96), components=(0, 2))
    assert np.array_equal(d[0], pl[0][20:84, 36:132]) and np.array_equal(d[1][::2, ::2], pl[2][10:42, 18:66])


@pytest.mark.parametrize("dtype", ["int16", "float32", "float16", "bfloat16"])
def test_flipping_twice_is_the_identity(dtype):
    p = _picture()
    pl = rref.planes(p.seq, p.slices, p.meta_np, levels_of(p))
    sc = (0.5, -0.37, 1.0 / 3.0)
    for window, size in (((36, 20, 96, 64), (64, 64)), ((2, 6, 8, 8), (64, 64)), ((0, 0, 200, 120), (37, 51))):
        a = rref.dense(pl, window, False, size, dtype=dtype, scale=sc)
        f = rref.dense(pl, window, True, size, dtype=dtype, scale=sc)
        assert np.array_equal(f[:, :, ::-1], a)
        assert a.shape == (3,) + size


def test_float_values_are_one_product():
    r = np.array([[-32768, -255, -1, 0, 1, 3, 1000, 32767]], dtype=np.int16)
    s = np.float32(1.0 / 3.0)
    f32 = rref.convert(r, s, "float32").view(np.float32)
    assert np.array_equal(f32, r.astype(np.float32) * s)
    assert np.array_equal(rref.convert(r, s, "float16").view(np.float16), (r.astype(np.float32) * s).astype(np.float16))
    bf = rref.convert(r, s, "bfloat16")
    back = (bf.astype(np.uint32) << 16).view(np.float32)
    assert np.all(np.abs(back - f32) <= np.abs(f32) * 2.0 ** -8)
    assert rref.convert(np.array([[0]], dtype=np.int16), np.float32(-2.0), "float32")[0, 0] == 0x80000000      # -0.0: the product alone


def test_dense_sampling_is_the_pixel_exports_nearest_table():
    """the luma position a dense sample takes is the one tap of the scaled pixel export's nearest table for the same window"""
    seq = _seq()
    for (x, y, w, h), (H, W) in (((0, 0, 200, 120), (64, 64)), ((36, 20, 96, 64), (64, 64)), ((2, 6, 8, 8), (64, 64)), ((4, 2, 192, 64), (2, 6))):
        desc = abi.make_export_desc(abi.EXPORT_RGB, 8, 1, 0, (x, 200 - x - w, y, 120 - y - h), 1, 0)
        sc = abi.make_export_scale(W, H, abi.SCALE_NEAREST)
        for axis, (out, size) in enumerate(((W, w), (H, h))):
            first, count, _ = libhm_amd.export_scale_taps(seq, desc, sc, 0, axis)
            assert (count == 1).all() and np.array_equal(first, rref.nearest(size, out))


# ------------------------------------------------------------------------------------------------ 7. the ABI
def test_residual_structs_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d\\n",'
                   'sizeof(hmgpu_residual_desc),sizeof(hmgpu_residual_plan),offsetof(hmgpu_residual_desc,crop),offsetof(hmgpu_residual_desc,scale),'
                   'offsetof(hmgpu_residual_desc,reserved),offsetof(hmgpu_residual_plan,elem_bytes),offsetof(hmgpu_residual_plan,row_bytes),'
                   'HMGPU_RESIDUAL_PLANES,HMGPU_RESIDUAL_DENSE);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.ResidualDesc), C.sizeof(abi.ResidualPlan), abi.ResidualDesc.crop.offset, abi.ResidualDesc.scale.offset,
                   abi.ResidualDesc.reserved.offset, abi.ResidualPlan.elem_bytes.offset, abi.ResidualPlan.row_bytes.offset,
                   abi.RESIDUAL_PLANES, abi.RESIDUAL_DENSE]
    L = libhm_amd.lib()
    for name in ("hmgpu_residual_plan_for", "hmgpu_pictures_export_residual", "hmgpu_pictures_residual_check", "hmgpu_residual_destination_check"):
        assert hasattr(L, name)
