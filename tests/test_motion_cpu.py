"""Motion and block export without a GPU: the numpy model (tests/motion_ref.py) against HM's own arrays and the decoder's
internal_info block lists, the z-scan map, hmgpu_motion_plan_for with every refusal, the dense model's self-checks, and the ABI mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec, motion
from tests import golden_util as gu
from tests import motion_ref as mref
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the model against HM
def _paint(records, w4, h4, fill, pick=lambda r: r[4]):
    """x / y / w / h records (luma samples) painted into a grid of 4x4 blocks"""
    g = np.full((h4, w4), fill, np.int64)
    for r in records:
        x, y, w, h = r[:4]
        g[y // 4:(y + h + 3) // 4, x // 4:(x + w + 3) // 4] = pick(r)
    return g


def _decoder_grids(name):
    """per POC: grids painted from the parse-only decoder's internal_info lists, and what the lists do not carry from Picture.array"""
    z = gu.load("stream_" + name)
    out = {}
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(p):
            g = p.geometry()
            w4, h4 = g["width"] // 4, g["height"] // 4
            info = {k: d.internal_info(p, k) for k in ("CU_PREDICTION_MODE", "PU_MV_0", "PU_MV_1", "PU_REFERENCE_POC_0", "PU_REFERENCE_POC_1",
                                                       "PU_UNI_BI_PREDICTION", "CTU_SLICE_INDEX")}
            grids = dict(mode=_paint(info["CU_PREDICTION_MODE"], w4, h4, -1),
                         mvx0=_paint(info["PU_MV_0"], w4, h4, 0), mvy0=_paint(info["PU_MV_0"], w4, h4, 0, lambda r: r[5]),
                         mvx1=_paint(info["PU_MV_1"], w4, h4, 0), mvy1=_paint(info["PU_MV_1"], w4, h4, 0, lambda r: r[5]),
                         ref0=_paint(info["PU_REFERENCE_POC_0"], w4, h4, -1), ref1=_paint(info["PU_REFERENCE_POC_1"], w4, h4, -1),
                         dir=_paint(info["PU_UNI_BI_PREDICTION"], w4, h4, 0), slice=_paint(info["CTU_SLICE_INDEX"], w4, h4, 0))
            grids["slices"] = [p.slice_params(i)[0] for i in range(p.num_slices())]
            grids["arrays"] = {k: p.array(k) for k in ("mv1", "ref_idx1")}
            out[p.poc] = grids
        d.decode_stream(z["bitstream"], on_output=on_output)
    return out


@pytest.mark.parametrize("name", gu.STREAMS)
def test_model_on_hm_arrays_equals_the_decoder_block_lists(name):
    """HM's TComDataCU arrays (the fixture) through the z-scan model against grids painted from the x / y / w / h records of the
    decoder's internal_info -- an independent route.  What the lists carry: the prediction mode, list 0's vector, and the reference
    INDEX of list 0 (libHM's "reference POC" kinds report the index), which the slice's own ref_poc table turns into the POC.  What
    they do not carry: list 1 of bi-predicted PUs (libHM reports list 1 only for PUs that use list 1 alone).  There the lists are
    compared where they speak, and the whole list-1 plane is compared against the parser's arrays (Picture.array), which
    tests/test_parser_streams.py holds against HM."""
    got = _decoder_grids(name)
    pics = gu.stream_pictures(name)
    assert sorted(got) == sorted(p.poc for p in pics)
    for p in pics:
        log2 = int(np.log2(p.ctu_size))
        m = mref.grid(p.meta_np, p.slices, p.width, p.height, log2)
        g = got[p.poc]
        where = "%s POC %d" % (name, p.poc)
        assert np.array_equal(m["block"][0], g["mode"]), where + ": mode"
        assert np.array_equal(m["mv"][0, 0], g["mvx0"]) and np.array_equal(m["mv"][0, 1], g["mvy0"]), where + ": list 0 vectors"
        types = np.array([int(s.slice_type) for s in g["slices"]])[g["slice"]]
        pocs = np.array([[int(s.ref_poc[0][i]) for i in range(16)] for s in g["slices"]])
        used0 = (g["mode"] == 0) & (g["ref0"] >= 0) & (types != abi.I_SLICE)
        want0 = np.where(used0, pocs[g["slice"], np.maximum(g["ref0"], 0)], mref.NO_REF)
        assert np.array_equal(m["ref_poc"][0], want0), where + ": list 0 reference POC"
        assert np.array_equal(m["used"][0], used0), where
        only1 = g["dir"] == 2                                    # list 1 alone: the lists carry it
        assert np.array_equal(m["mv"][1, 0][only1], g["mvx1"][only1]) and np.array_equal(m["mv"][1, 1][only1], g["mvy1"][only1]), where
        pocs1 = np.array([[int(s.ref_poc[1][i]) for i in range(16)] for s in g["slices"]])
        assert np.array_equal(m["ref_poc"][1][only1], pocs1[g["slice"], np.maximum(g["ref1"], 0)][only1]), where
        # the whole list-1 plane: the parser's arrays, with the header's rule applied by hand
        ctu, zz = mref.block_index(p.width, p.height, log2)
        ref1 = g["arrays"]["ref_idx1"].reshape(p.num_ctus, -1)[ctu, zz].astype(np.int64)
        mv1 = g["arrays"]["mv1"].reshape(p.num_ctus, -1, 2)[ctu, zz].astype(np.int64)
        used1 = (g["mode"] == 0) & (types == abi.B_SLICE) & (ref1 >= 0)
        assert np.array_equal(m["used"][1], used1), where + ": list 1 used"
        assert np.array_equal(m["mv"][1, 0], np.where(used1, mv1[..., 0], 0)) and np.array_equal(m["mv"][1, 1], np.where(used1, mv1[..., 1], 0)), where
        assert np.array_equal(m["ref_poc"][1], np.where(used1, pocs1[g["slice"], np.maximum(ref1, 0)], mref.NO_REF)), where


@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
def test_zscan_map_is_synths(log2_ctu):
    parts = 1 << (2 * log2_ctu - 4)
    zx, zy = synth._zxy(parts)
    assert np.array_equal(mref.zscan(zx, zy, log2_ctu - 2), np.arange(parts))
    # and the picture-wide index of a picture with partial CTUs on both borders
    w, h = 200, 120
    ctu, z = mref.block_index(w, h, log2_ctu)
    cw = (w + (1 << log2_ctu) - 1) >> log2_ctu
    by, bx = np.mgrid[0:h // 4, 0:w // 4]
    pw = 1 << (log2_ctu - 2)
    assert np.array_equal(ctu, (by // pw) * cw + bx // pw)
    assert np.array_equal(zx[z], bx % pw) and np.array_equal(zy[z], by % pw)


# ------------------------------------------------------------------------------------------------ 2. the plan
def _seq(fmt=1, w=200, h=120, log2_ctu=6):
    s = abi.make_seq(w, h, 10, 10, log2_ctu=log2_ctu)
    s.chroma_format = fmt
    return s


def _status(seq, desc, scale=None, windows=None, n=None):
    try:
        motion.plan_for(seq, desc, scale, windows, n)
    except libhm_amd.HmgpuError as e:
        return e.status
    return abi.HMGPU_OK


def _win(seq, xywh, flip=False):
    x, y, w, h = xywh
    return abi.make_export_window((x, seq.width - x - w, y, seq.height - y - h), flip)


@pytest.mark.parametrize("fmt", [1, 3, 0])
def test_plan_shapes_are_on_the_luma_grid(fmt):
    seq = _seq(fmt)
    for lists, L in ((1, 1), (2, 1), (3, 2)):
        p = libhm_amd.motion_plan(seq, "blocks", lists)
        assert p.lists == L
        assert list(p.channels) == [2 * L, 0, L, 4] and list(p.elem_bytes) == [2, 0, 4, 1]
        assert list(p.width) == [50, 0, 50, 50] and list(p.height) == [30, 0, 30, 30]
        assert list(p.row_bytes) == [100, 0, 200, 50]
    p = libhm_amd.motion_plan(seq, "blocks", (0, 1), crop=(8, 12, 4, 16))
    assert (p.width[0], p.height[0]) == (45, 25)
    for st, es in ((abi.SAMPLE_F16, 2), (abi.SAMPLE_BF16, 2), (abi.SAMPLE_F32, 4)):
        p = libhm_amd.motion_plan(seq, "dense", (1,), size=(64, 48), windows=[(36, 20, 96, 64), (2, 6, 8, 8)], dtype=st)
        assert list(p.channels) == [0, 2, 1, 4] and list(p.elem_bytes) == [0, es, 4, 1]
        assert list(p.width) == [0, 48, 48, 48] and list(p.height) == [0, 64, 64, 64] and list(p.row_bytes) == [0, 48 * es, 192, 48]
    p = libhm_amd.motion_plan(seq, "dense", (0, 1), windows=[(0, 0, 96, 64), (104, 56, 96, 64)], flip=[False, True])
    assert list(p.channels) == [2, 2, 2, 4] and (p.width[0], p.height[0]) == (96, 64)


def test_plan_refusals_match_the_header():
    seq = _seq()
    E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    blocks = lambda **kw: abi.make_motion_desc(abi.MOTION_BLOCKS, kw.pop("lists", 3), kw.pop("sample_type", abi.SAMPLE_UINT), kw.pop("crop", (0, 0, 0, 0)))
    dense = lambda st=abi.SAMPLE_F16, lists=3: abi.make_motion_desc(abi.MOTION_DENSE, lists, st)
    whole = [_win(seq, (0, 0, 200, 120))]
    nearest = abi.make_export_scale(64, 64, abi.SCALE_NEAREST)
    assert _status(seq, blocks()) == abi.HMGPU_OK and _status(seq, dense(), nearest, whole) == abi.HMGPU_OK
    # a crop that is no multiple of 4, negative, or empty
    for crop in ((2, 0, 0, 0), (0, 6, 0, 0), (0, 0, 1, 0), (0, 0, 0, 3), (-4, 0, 0, 0), (100, 100, 0, 0)):
        assert _status(seq, blocks(crop=crop)) == E, crop
    # lists mask, form, reserved words, n
    assert _status(seq, blocks(lists=0)) == E and _status(seq, blocks(lists=4)) == E
    d = blocks(); d.form = 2
    assert _status(seq, d) == E
    for k in range(5):
        d = blocks(); d.reserved[k] = 1
        assert _status(seq, d) == E
        d = dense(); d.reserved[k] = 1
        assert _status(seq, d, nearest, whole) == E
    assert _status(seq, blocks(), n=0) == E and _status(seq, blocks(), n=17) == E and _status(seq, blocks(), n=16) == abi.HMGPU_OK
    assert _status(seq, dense(), nearest, whole * 17) == E and _status(seq, dense(), nearest, whole, n=0) == E
    # BLOCKS takes neither a scale nor windows nor a float type; DENSE needs windows, a float type and no crop
    assert _status(seq, blocks(), nearest) == E and _status(seq, blocks(), None, whole) == E and _status(seq, blocks(sample_type=abi.SAMPLE_F16)) == E
    assert _status(seq, dense(abi.SAMPLE_UINT), nearest, whole) == E
    assert _status(seq, dense(), nearest, None, n=1) == E
    d = dense(); d.crop[0] = 4
    assert _status(seq, d, nearest, whole) == E
    # filters other than nearest: not supported; an unknown filter code or a reserved word of the scale: invalid
    for f in (abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
        assert _status(seq, dense(), abi.make_export_scale(64, 64, f), whole) == U
    assert _status(seq, dense(), abi.make_export_scale(64, 64, 7), whole) == E
    s = abi.make_export_scale(64, 64, abi.SCALE_NEAREST); s.reserved[2] = 1
    assert _status(seq, dense(), s, whole) == E
    # windows: flip bits other than bit 0, reserved words, outside the picture, odd origins in 4:2:0
    w = _win(seq, (0, 0, 96, 64)); w.flip = 2
    assert _status(seq, dense(), nearest, [w]) == E
    w = _win(seq, (0, 0, 96, 64)); w.reserved[1] = 1
    assert _status(seq, dense(), nearest, [w]) == E
    assert _status(seq, dense(), nearest, [_win(seq, (150, 0, 96, 64))]) == E
    assert _status(seq, dense(), nearest, [_win(seq, (3, 0, 96, 64))]) == E and _status(_seq(3), dense(), nearest, [_win(seq, (3, 1, 96, 64))]) == abi.HMGPU_OK
    # unscaled windows of unequal size
    assert _status(seq, dense(), None, [_win(seq, (0, 0, 96, 64)), _win(seq, (4, 4, 96, 60))]) == E
    assert _status(seq, dense(), None, [_win(seq, (0, 0, 96, 64)), _win(seq, (6, 2, 96, 64))]) == abi.HMGPU_OK
    # the limits of the scaled export, per window: 32x reduction, 8x enlargement, 16384 outputs per side
    assert _status(seq, dense(), abi.make_export_scale(6, 2, 0), [_win(seq, (4, 2, 192, 64))]) == abi.HMGPU_OK
    assert _status(seq, dense(), abi.make_export_scale(6, 2, 0), [_win(seq, (4, 2, 194, 64))]) == U
    assert _status(seq, dense(), abi.make_export_scale(6, 2, 0), [whole[0], _win(seq, (4, 2, 192, 66))]) == U
    assert _status(seq, dense(), abi.make_export_scale(64, 64, 0), [_win(seq, (2, 6, 8, 8))]) == abi.HMGPU_OK
    assert _status(seq, dense(), abi.make_export_scale(66, 64, 0), [_win(seq, (2, 6, 8, 8))]) == U
    big = _seq(w=4096, h=2304)
    assert _status(big, dense(), abi.make_export_scale(16386, 64, 0), [_win(big, (0, 0, 4096, 2304))]) == U
    # a sequence whose size is no multiple of 4 has no block grid
    assert _status(_seq(w=202), blocks()) == E


# ------------------------------------------------------------------------------------------------ 3. the dense model
def _picture(**kw):
    return synth.make_picture(200, 120, 10, seed=77, bi=True, num_refs=2, intra_frac=0.3, ref_handles=([0, 1], [1]), **kw)


def test_dense_at_the_windows_own_size_is_the_block_grid_upsampled():
    p = _picture()
    b = mref.blocks(p.meta_np, p.slices, 200, 120, 6)
    d = mref.dense(p.meta_np, p.slices, 200, 120, 6, (0, 0, 200, 120), None, False, abi.SAMPLE_F32)
    assert np.array_equal(d["sx"], np.arange(200)) and np.array_equal(d["sy"], np.arange(120))
    for l in range(2):
        up = np.repeat(np.repeat(b["mv"][l].astype(np.float32) / np.float32(4), 4, axis=1), 4, axis=2)
        assert np.array_equal(d["flow%d" % l].view(np.float32), up)
    assert np.array_equal(d["ref_poc"], np.repeat(np.repeat(b["ref_poc"], 4, axis=1), 4, axis=2))
    assert np.array_equal(d["block"], np.repeat(np.repeat(b["block"], 4, axis=1), 4, axis=2))
    assert (b["ref_poc"] == mref.NO_REF).any() and (b["block"][0] == 1).any() and (b["mv"] != 0).any()


@pytest.mark.parametrize("st", [abi.SAMPLE_F32, abi.SAMPLE_F16, abi.SAMPLE_BF16])
def test_flipping_twice_is_the_identity(st):
    p = _picture()
    for window, size in (((36, 20, 96, 64), (64, 64)), ((2, 6, 8, 8), (64, 64)), ((0, 0, 200, 120), (37, 51))):
        a = mref.dense(p.meta_np, p.slices, 200, 120, 6, window, size, False, st)
        f = mref.dense(p.meta_np, p.slices, 200, 120, 6, window, size, True, st)
        sign = np.uint32(1 << 31) if st == abi.SAMPLE_F32 else np.uint16(1 << 15)
        for l in range(2):
            dx, dy = f["flow%d" % l][0][:, ::-1], f["flow%d" % l][1][:, ::-1]
            nz = (a["flow%d" % l][0] & ~sign) != 0
            assert np.array_equal(np.where(nz, dx ^ sign, dx), a["flow%d" % l][0])       # dx back to its sign (zero has none)
            assert np.array_equal(dy, a["flow%d" % l][1])
        assert np.array_equal(f["ref_poc"][:, :, ::-1], a["ref_poc"]) and np.array_equal(f["block"][:, :, ::-1], a["block"])


def test_unused_lists_read_as_zero_whatever_the_arrays_hold():
    """a P slice whose list-1 arrays hold another picture's values, and an I slice whose list 0 does: the slice type decides"""
    p = _picture()
    m = dict(p.meta_np)
    as_p = abi.clone_slice(p.slices[0]); as_p.slice_type = abi.P_SLICE
    as_i = abi.clone_slice(p.slices[0]); as_i.slice_type = abi.I_SLICE
    gb, gp, gi = (mref.grid(m, [s], 200, 120, 6) for s in (p.slices[0], as_p, as_i))
    assert gb["used"][1].any() and not gp["used"][1].any() and not gi["used"].any()
    assert not gp["mv"][1].any() and (gp["ref_poc"][1] == mref.NO_REF).all() and np.array_equal(gp["mv"][0], gb["mv"][0])
    assert not gi["mv"].any() and (gi["ref_poc"] == mref.NO_REF).all()


def test_dense_sampling_is_the_pixel_exports_nearest_table():
    """the luma position a dense sample takes is the one tap of the scaled pixel export's nearest table for the same window"""
    seq = _seq()
    for (x, y, w, h), (H, W) in (((0, 0, 200, 120), (64, 64)), ((36, 20, 96, 64), (64, 64)), ((2, 6, 8, 8), (64, 64)), ((4, 2, 192, 64), (2, 6))):
        desc = abi.make_export_desc(abi.EXPORT_RGB, 8, 1, 0, (x, 200 - x - w, y, 120 - y - h), 1, 0)
        sc = abi.make_export_scale(W, H, abi.SCALE_NEAREST)
        for axis, (out, size) in enumerate(((W, w), (H, h))):
            first, count, _ = libhm_amd.export_scale_taps(seq, desc, sc, 0, axis)
            assert (count == 1).all() and np.array_equal(first, mref.nearest_index(out, size))


# ------------------------------------------------------------------------------------------------ 4. the ABI
def test_motion_structs_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n",'
                   'sizeof(hmgpu_motion_desc),sizeof(hmgpu_motion_plan),offsetof(hmgpu_motion_desc,crop),offsetof(hmgpu_motion_desc,reserved),'
                   'offsetof(hmgpu_motion_plan,elem_bytes),offsetof(hmgpu_motion_plan,row_bytes),HMGPU_MOTION_NO_REF==INT32_MIN,'
                   'HMGPU_MOTION_DSTS,HMGPU_MOTION_DENSE);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.MotionDesc), C.sizeof(abi.MotionPlan), abi.MotionDesc.crop.offset, abi.MotionDesc.reserved.offset,
                   abi.MotionPlan.elem_bytes.offset, abi.MotionPlan.row_bytes.offset, 1, abi.MOTION_DSTS, abi.MOTION_DENSE]
    assert abi.MOTION_NO_REF == -(1 << 31)
    L = libhm_amd.lib()
    for name in ("hmgpu_motion_plan_for", "hmgpu_pictures_export_motion", "hmgpu_motion_destination_check"):
        assert hasattr(L, name)
    assert hasattr(hmdec.lib(), "hmdec_pictures_export_motion")


# ------------------------------------------------------------------------------------------------ 5. Decoder.frames(motion=) arguments
def test_frames_refuses_motion_arguments_it_cannot_honour():
    """the checks come before anything is decoded or exported: a parse-only decoder shows them"""
    z = gu.load("stream_ra_main10_208x120")
    with hmdec.Decoder(parse_only=True) as d:
        for bad in (dict(form="dense", windows=[(0, 0, 96, 64)]), dict(form=abi.MOTION_DENSE, flip=[True]), dict(out={}), dict(form="nope")):
            with pytest.raises(ValueError):
                next(d.frames(z["bitstream"], batch=4, size=(32, 48), filter="nearest", motion=bad))
        with pytest.raises(ValueError):
            next(d.frames(z["bitstream"], motion=True))                          # motion needs batch=
