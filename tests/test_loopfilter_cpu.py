"""The loop-filter export without a GPU: the plan function for every format and CTU size with every refusal, the struct mirrors, the
dense rule of tests/loopfilter_ref.py held against a per-sample loop, and the invariants of the model on synthetic pictures (the
boundary strengths and SAO parameters from the C oracle)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec, loopfilter
from tests import loopfilter_ref as lref
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_plan_shapes(fmt, log2_ctu):
    import torch
    seq = abi.make_seq(520, 328, 10, 10, log2_ctu=log2_ctu)
    seq.chroma_format = fmt
    ctu = 1 << log2_ctu
    cw, ch = (520 + ctu - 1) // ctu, (328 + ctu - 1) // ctu
    p = libhm_amd.loopfilter_plan(seq, n=16)
    assert list(p.channels) == [13, 18, 0] and list(p.width) == [130, cw, 0] and list(p.height) == [82, ch, 0]
    assert list(p.elem_bytes) == [2, 1, 0] and list(p.row_bytes) == [260, cw, 0]
    p = libhm_amd.loopfilter_plan(seq, crop=(8, 16, 24, 0))
    assert list(p.width) == [124, cw, 0] and list(p.height) == [76, ch, 0]          # the crop cuts the edge grid only
    for dtype, es in ((None, 1), (torch.float16, 2), (torch.bfloat16, 2), (torch.float32, 4)):
        p = libhm_amd.loopfilter_plan(seq, "dense", dtype=dtype, scale=None if dtype is None else (1.0, 0.5, -2.0))
        assert list(p.channels) == [0, 0, 3] and list(p.width) == [0, 0, 520] and list(p.height) == [0, 0, 328]
        assert list(p.elem_bytes) == [0, 0, es] and list(p.row_bytes) == [0, 0, 520 * es]
        p = libhm_amd.loopfilter_plan(seq, "dense", size=(100, 200), windows=[(0, 0, 200, 100), (8, 2, 400, 300)], dtype=dtype)
        assert list(p.width) == [0, 0, 200] and list(p.height) == [0, 0, 100]


def test_plan_refusals_match_the_header():
    L = libhm_amd.lib()
    seq = abi.make_seq(520, 328, 10, 10)
    whole = [abi.make_export_window((0, 0, 0, 0))]

    def status(d, n=1, s=seq, sc=None, win=None):
        plan = abi.LoopfilterPlan()
        plan.channels[0] = 77
        st = L.hmgpu_loopfilter_plan_for(C.byref(s), C.byref(d), abi.ref(sc), n, abi.window_array(win), C.byref(plan))
        assert st == abi.HMGPU_OK or not any(bytes(plan))                 # a refused call leaves the plan zero
        return st
    ok = abi.make_loopfilter_desc
    dense = lambda **kw: ok(abi.LOOPFILTER_DENSE, **kw)
    assert status(ok()) == abi.HMGPU_OK and status(dense(), win=whole) == abi.HMGPU_OK
    for form in (-1, 2):                                                    # bad form
        assert status(ok(form)) == abi.HMGPU_EINVAL
    for n in (0, -1, 17):                                                   # n > 16
        assert status(ok(), n) == abi.HMGPU_EINVAL
    assert status(ok(), 16) == abi.HMGPU_OK
    for crop in ((4, 0, 0, 0), (0, 12, 0, 0), (0, 0, 2, 0), (0, 0, 0, 4), (-8, 0, 0, 0), (520, 0, 0, 0)):     # misaligned / impossible crop
        assert status(ok(crop=crop)) == abi.HMGPU_EINVAL
    assert status(ok(crop=(8, 8, 8, 8))) == abi.HMGPU_OK
    for k in range(7):
        d = ok()
        d.reserved[k] = 1
        assert status(d) == abi.HMGPU_EINVAL
    # the grids take neither a scale nor windows nor a float type
    assert status(ok(), sc=abi.make_export_scale(64, 64, abi.SCALE_NEAREST)) == abi.HMGPU_EINVAL
    assert status(ok(), win=whole) == abi.HMGPU_EINVAL
    assert status(ok(sample_type=abi.SAMPLE_F32)) == abi.HMGPU_EINVAL
    # the dense form: windows always, a crop never, nearest only, finite scales, a known element
    assert status(dense()) == abi.HMGPU_EINVAL
    assert status(dense(crop=(8, 0, 0, 0)), win=whole) == abi.HMGPU_EINVAL
    for f in (abi.SCALE_BILINEAR, abi.SCALE_BICUBIC):                       # filter not nearest
        assert status(dense(), sc=abi.make_export_scale(64, 64, f), win=whole) == abi.HMGPU_EUNSUPPORTED
    assert status(dense(), sc=abi.make_export_scale(64, 64, abi.SCALE_NEAREST), win=whole) == abi.HMGPU_OK
    for st in (abi.SAMPLE_F16, abi.SAMPLE_BF16, abi.SAMPLE_F32):
        assert status(dense(sample_type=st, scale=(1.0, float("nan"), 1.0)), win=whole) == abi.HMGPU_EINVAL
        assert status(dense(sample_type=st, scale=(1.0, 1.0, float("inf"))), win=whole) == abi.HMGPU_EINVAL
        assert status(dense(sample_type=st, scale=(0.0, -1.0, 3.5)), win=whole) == abi.HMGPU_OK
    assert status(dense(scale=(float("nan"),) * 3), win=whole) == abi.HMGPU_OK          # uint8: the scales are not read
    for st in (-1, 4, 99):
        assert status(dense(sample_type=st), win=whole) == abi.HMGPU_EINVAL
    two = [abi.make_export_window((0, 0, 0, 0)), abi.make_export_window((8, 0, 0, 0))]
    assert status(dense(), 2, win=two) == abi.HMGPU_EINVAL                  # unscaled windows of two sizes
    bad = abi.make_seq(520, 328, 10, 10)
    bad.chroma_format = 4
    assert status(ok(), s=bad) == abi.HMGPU_EINVAL
    assert status(ok(), s=abi.make_seq(516, 328, 10, 10)) == abi.HMGPU_EINVAL
    # null description, sequence, plan
    assert L.hmgpu_loopfilter_plan_for(C.byref(seq), None, None, 1, None, C.byref(abi.LoopfilterPlan())) == abi.HMGPU_EINVAL
    assert L.hmgpu_loopfilter_plan_for(None, C.byref(ok()), None, 1, None, C.byref(abi.LoopfilterPlan())) == abi.HMGPU_EINVAL
    assert L.hmgpu_loopfilter_plan_for(C.byref(seq), C.byref(ok()), None, 1, None, None) == abi.HMGPU_EINVAL
    with pytest.raises(ValueError):
        loopfilter.describe(seq, 1, "nope")
    with pytest.raises(ValueError):
        loopfilter.describe(seq, 1, "grids", size=(8, 8))                   # size belongs to the dense form
    with pytest.raises(ValueError):
        loopfilter.describe(seq, 1, "dense", scale=(1.0, 1.0, 1.0))         # a scale needs a float dtype


def test_loopfilter_structs_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\\n",'
                   'sizeof(hmgpu_loopfilter_desc),sizeof(hmgpu_loopfilter_plan),offsetof(hmgpu_loopfilter_desc,crop),offsetof(hmgpu_loopfilter_desc,scale),'
                   'offsetof(hmgpu_loopfilter_desc,reserved),offsetof(hmgpu_loopfilter_plan,elem_bytes),offsetof(hmgpu_loopfilter_plan,row_bytes),'
                   'HMGPU_LOOPFILTER_GRIDS,HMGPU_LOOPFILTER_DENSE,HMGPU_LOOPFILTER_DST_EDGE,HMGPU_LOOPFILTER_DST_SAO,HMGPU_LOOPFILTER_DST_DENSE,'
                   'HMGPU_LOOPFILTER_EDGE_CHANNELS,HMGPU_LOOPFILTER_SAO_CHANNELS,HMGPU_LF_FLAGS,HMGPU_LF_TC_CR_HOR);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.LoopfilterDesc), C.sizeof(abi.LoopfilterPlan), abi.LoopfilterDesc.crop.offset, abi.LoopfilterDesc.scale.offset,
                   abi.LoopfilterDesc.reserved.offset, abi.LoopfilterPlan.elem_bytes.offset, abi.LoopfilterPlan.row_bytes.offset,
                   abi.LOOPFILTER_GRIDS, abi.LOOPFILTER_DENSE, abi.LOOPFILTER_DST_EDGE, abi.LOOPFILTER_DST_SAO, abi.LOOPFILTER_DST_DENSE,
                   abi.LOOPFILTER_EDGE_CHANNELS, abi.LOOPFILTER_SAO_CHANNELS, abi.LF_FLAGS, abi.LF_TC_CR_HOR]
    assert lref.EDGE_CHANNELS == abi.LOOPFILTER_EDGE_CHANNELS and lref.SAO_CHANNELS == abi.LOOPFILTER_SAO_CHANNELS and lref.FLAGS == abi.LF_FLAGS
    assert (lref.BS, lref.QP, lref.TC, lref.BETA, lref.TC_CB, lref.TC_CR) == (abi.LF_BS_VER, abi.LF_QP_VER, abi.LF_TC_VER, abi.LF_BETA_VER,
                                                                             abi.LF_TC_CB_VER, abi.LF_TC_CR_VER)
    L = libhm_amd.lib()
    for name in ("hmgpu_loopfilter_plan_for", "hmgpu_pictures_export_loopfilter", "hmgpu_pictures_loopfilter_check",
                 "hmgpu_loopfilter_destination_check"):
        assert hasattr(L, name)
    assert hasattr(hmdec.lib(), "hmdec_pictures_export_loopfilter")
    assert C.sizeof(abi.LoopfilterDesc) == 64 and C.sizeof(abi.LoopfilterPlan) == 64
    assert len(loopfilter.edge_names) == 13 and len(loopfilter.sao_names) == 6 and len(loopfilter.sao_channels) == 6


# ------------------------------------------------------------------------------------------------ 2. the dense rule
def test_dense_rule_equals_the_per_sample_loop():
    """a 24x16 picture with 8-sample CTUs' worth of distinct values: every unit of the grid a different Bs pattern, so that a position
    off by one block or one edge shows"""
    seq = abi.make_seq(24, 16, 8, 8, log2_ctu=4)
    rng = np.random.RandomState(5)
    edge = np.zeros((13, 4, 6), dtype=np.int16)
    edge[lref.BS] = rng.randint(0, 3, size=(4, 6)) * (np.arange(6)[None, :] % 2 == 0)
    edge[lref.BS + 1] = rng.randint(0, 3, size=(4, 6)) * (np.arange(4)[:, None] % 2 == 0)
    edge[lref.BS][:, 0] = 2                                              # (a picture never has these: the rule must ignore column / row 0)
    edge[lref.BS + 1][0, :] = 2
    sao = np.zeros((3, 6, 1, 2), dtype=np.int8)
    sao[0, 0, 0] = [3, -1]
    for window, size, flip in (((0, 0, 24, 16), None, False), ((0, 0, 24, 16), None, True), ((3, 2, 18, 11), None, False),
                               ((2, 4, 22, 12), (7, 13), True), ((0, 0, 24, 16), (32, 48), False), ((20, 12, 4, 4), (4, 4), False)):
        got = lref.dense(seq, edge, sao, window, size, flip)
        want = lref.dense_brute(seq, edge, sao, window, size, flip)
        assert np.array_equal(got, want), (window, size, flip)
    full = lref.dense(seq, edge, sao, (0, 0, 24, 16))
    # the samples an edge at column 8 can reach are columns 4 .. 11; columns 0 .. 3 and 20 .. 23 face the picture border
    assert (full[0][:, :4] == 0).all() and (full[0][:, 20:] == 0).all() and (full[1][:4] == 0).all() and (full[1][12:] == 0).all()
    for r in range(16):
        assert (full[0][r, 4:12] == edge[lref.BS][r // 4, 2]).all() and (full[0][r, 12:20] == edge[lref.BS][r // 4, 4]).all()
    assert (full[2][:, :16] == 4).all() and (full[2][:, 16:] == 0).all()
    assert np.array_equal(lref.dense(seq, edge, sao, (0, 0, 24, 16), flip=True), full[:, :, ::-1])


# ------------------------------------------------------------------------------------------------ 3. the model on synthetic pictures
def _checks(p, edge):
    h4, w4 = edge.shape[1:]
    by, bx = np.meshgrid(np.arange(h4), np.arange(w4), indexing="ij")
    fmt = p.seq.chroma_format
    csx, csy = (1 if fmt in (1, 2) else 0), (1 if fmt == 1 else 0)
    e = edge.astype(np.int64)
    for d, off in ((0, bx % 2 != 0), (1, by % 2 != 0)):
        for c in (lref.BS, lref.QP, lref.TC, lref.BETA, lref.TC_CB, lref.TC_CR):
            assert (e[c + d][off] == 0).all(), (c, d)                          # a channel is non-zero only on its grid
        assert (((e[lref.FLAGS] >> (2 * d)) & 3)[off] == 0).all()
        bs = e[lref.BS + d]
        assert bs.min() >= 0 and bs.max() <= 2
        zero = bs == 0
        for c in (lref.QP, lref.TC, lref.BETA, lref.TC_CB, lref.TC_CR):
            assert (e[c + d][zero] == 0).all(), (c, d)                         # tc and beta are 0 where Bs is 0 ...
        assert (((e[lref.FLAGS] >> (2 * d)) & 3)[zero] == 0).all()
        # ... and exactly there: at QP 22 .. 37 with these offsets the beta index stays at 16 or above, where the table is non-zero
        assert (e[lref.BETA + d][~zero] > 0).all()
        step = (8 << csx) if d == 0 else (8 << csy)
        chroma_grid = ((bx if d == 0 else by) * 4) % step == 0
        for c in (lref.TC_CB, lref.TC_CR):
            assert (e[c + d][~((bs == 2) & chroma_grid)] == 0).all()            # chroma tc only where Bs is 2 on the chroma grid
            if fmt == 0:
                assert (e[c + d] == 0).all()
    assert (e[lref.FLAGS] >> 4 == 0).all()


@pytest.mark.parametrize("fmt,log2_ctu,bd,bdc", [(1, 6, 10, 10), (0, 6, 8, 8), (2, 5, 12, 10), (3, 4, 8, 8)])
def test_model_invariants(oracle, fmt, log2_ctu, bd, bdc):
    p = synth.make_picture(136, 72, bd, seed=0x1F + fmt, bi=True, intra_frac=0.3, cbf_prob=0.3, mv_coherence=0.6, chroma_format=fmt,
                           log2_ctu=log2_ctu, bit_depth_chroma=bdc, num_slices=3, lf_across_slices=0)
    edge, sao = lref.picture_model(oracle, p)
    assert edge.shape == (13, 18, 34) and edge.dtype == np.int16
    _checks(p, edge)
    for d in (0, 1):
        assert (edge[lref.BS + d] == 1).any() and (edge[lref.BS + d] == 2).any() and (edge[lref.TC + d] > 0).any()
    if fmt:
        assert (edge[lref.TC_CB:lref.TC_CR + 2] > 0).any()
    ctu = 1 << log2_ctu
    assert sao.shape == (3, 6, (72 + ctu - 1) // ctu, (136 + ctu - 1) // ctu) and sao.dtype == np.int8
    off = sao[:, 0] < 0
    assert (sao[:, 1:][np.broadcast_to(off[:, None], sao[:, 1:].shape)] == 0).all()           # an off CTB holds zeros
    assert (sao[:, 1][sao[:, 0] != lref.SAO_BO] == 0).all()                                 # BAND is BO's
    if fmt == 0:
        assert (sao[1:, 0] == -1).all()
    off_sao = lref.sao_grid(p.seq, None, enabled=False)
    assert (off_sao[:, 0] == -1).all() and (off_sao[:, 1:] == 0).all()


def test_chroma_qp_mapping():
    assert list(lref.chroma_qp(np.array([-3, 0, 29, 30, 43, 44, 57, 58, 63]), 1)) == [-3, 0, 29, 29, 37, 38, 51, 52, 57]
    assert list(lref.chroma_qp(np.array([-3, 0, 29, 30, 43, 51, 52, 58, 63]), 2)) == [-3, 0, 29, 30, 43, 51, 51, 51, 51]
    assert list(lref.chroma_qp(np.array([30, 57]), 3)) == [30, 51]
