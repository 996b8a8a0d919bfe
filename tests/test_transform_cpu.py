"""The transform export without a GPU: the numpy de-quantiser of tests/transform_ref.py held against the C oracle (flat scaling
element for element, scaling lists through the inverse transform), the plan function with every refusal, the struct mirrors, and the
model of levels and info grid held against hmdec_internal_info on HM-encoded streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec, transform
from oracle import hmoracle
from tests import golden_util as gu
from tests import transform_ref as tref
from tests.test_gpu_residual_decoder import KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def full_range_levels(rng, n):
    """int16 levels uniform over the full range, with both ends, zero and the small values in"""
    lev = rng.randint(-32768, 32768, size=(n, n)).astype(np.int16)
    lev.flat[:8] = [-32768, 32767, 0, 1, -1, 2, -2, 255]
    return lev


# ------------------------------------------------------------------------------------------------ 1. the restatement of xDeQuant
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_flat_dequant_equals_the_oracle_element_for_element(bd):
    lib = hmoracle.lib()
    rng = np.random.RandomState(bd)
    for log2 in (2, 3, 4, 5):
        n = 1 << log2
        for per in range(0, (51 + 6 * (bd - 8)) // 6 + 1):
            for rem in range(6):
                lev = full_range_levels(rng, n)
                want = np.zeros((n, n), dtype=np.int32)
                lib.hmo_dequant(_p(lev), _p(want), n * n, log2, bd, per, rem)
                got = tref.dequant(lev, log2, bd, per, rem)
                assert np.array_equal(got, want), (bd, log2, per, rem)


def _lists(seed):
    rng = np.random.RandomState(seed)
    lists = abi.ScalingLists()
    for sz in range(4):
        for l in range(6):
            lists.dc[sz][l] = int(rng.randint(1, 256)) if sz >= 2 else 16
            for i in range(64):
                lists.coef[sz][l][i] = int(rng.randint(1, 256)) if i < (16 if sz == 0 else 64) else 16
    return lists


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_list_dequant_through_the_inverse_transform_equals_the_oracle(bd):
    """for blocks that take the transform, hmo_itr of the model's coefficients with xIT's cast is the oracle's own TU function with lists:
    this ties the numpy list path (matrix, shift, clips) to the oracle's private one"""
    lib = hmoracle.lib()
    rng = np.random.RandomState(100 + bd)
    lists = _lists(bd)
    differ = False
    seen = set()
    for log2 in (2, 3, 4, 5):
        n = 1 << log2
        for list_id in range(6):
            m = tref.list_matrix(lists, log2 - 2, list_id)
            seen.add(m.tobytes())
            assert len(np.unique(m)) > 4
            for per, rem in ((0, 0), (2, 5), (4, 1), (6, 3), (9, 2), ((51 + 6 * (bd - 8)) // 6, 4)):
                for lev in (full_range_levels(rng, n), rng.randint(-40, 41, size=(n, n)).astype(np.int16)):
                    coef = tref.dequant(lev, log2, bd, per, rem, m)
                    differ = differ or not np.array_equal(coef, tref.dequant(lev, log2, bd, per, rem))
                    dst = 1 if (log2 == 2 and list_id == 0) else 0
                    block = hmoracle.itr(bd, coef[None].astype(np.int32), dst)[0]
                    want = np.zeros((n, n), dtype=np.int16)
                    lib.hmo_inverse_transform_tu_sl(_p(lev), _p(want), n, log2, bd, per, rem, dst, C.byref(lists), list_id)
                    assert np.array_equal(block.astype(np.int16), want), (bd, log2, list_id, per, rem)
    assert differ and len(seen) == 24                      # the lists act, and no two of them are the same matrix


def test_qp_param_follows_the_formats_chroma_table():
    for fmt in (1, 2, 3):
        for qp in range(-12, 52):
            for off in (-12, 0, 7, 12):
                per, rem = tref.qp_param(qp, 1, 10, off, fmt)
                base = min(max(qp + off, -12), 57)
                if base >= 0:
                    base = (hmoracle.qp_param(base, 1, 8, 0)[0] * 6 + hmoracle.qp_param(base, 1, 8, 0)[1]) if fmt == 1 else min(base, 51)
                assert per * 6 + rem == base + 12, (fmt, qp, off)
    assert tref.qp_param(45, 1, 8, 0, 1) != tref.qp_param(45, 1, 8, 0, 3)
    assert tref.qp_param(30, 0, 10, 5, 0) == (7, 0)


# ------------------------------------------------------------------------------------------------ 2. the plan
@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_plan_shapes(fmt):
    import torch
    seq = abi.make_seq(416, 240, 10, 10)
    seq.chroma_format = fmt
    cw, ch = (416 if fmt == 3 else 208), (120 if fmt in (0, 1) else 240)
    for dtype, es in ((None, 2), (torch.float16, 2), (torch.bfloat16, 2), (torch.float32, 4)):
        for value in ("levels", "coeffs"):
            p = libhm_amd.transform_plan(seq, value, dtype=dtype, scale=None if dtype is None else (0.5, 1.0, -2.0), n=16)
            assert list(p.channels) == [1, 0 if fmt == 0 else 1, 0 if fmt == 0 else 1, 6]
            assert list(p.width) == [416, 0 if fmt == 0 else cw, 0 if fmt == 0 else cw, 104]
            assert list(p.height) == [240, 0 if fmt == 0 else ch, 0 if fmt == 0 else ch, 60]
            assert list(p.elem_bytes) == [es, 0 if fmt == 0 else es, 0 if fmt == 0 else es, 1]
            assert list(p.row_bytes) == [416 * es, 0 if fmt == 0 else cw * es, 0 if fmt == 0 else cw * es, 104]
    p = libhm_amd.transform_plan(seq, components=(2,))
    assert list(p.channels) == [0, 0, 0 if fmt == 0 else 1, 6]


def test_plan_refusals_match_the_header():
    L = libhm_amd.lib()
    seq = abi.make_seq(416, 240, 10, 10)

    def status(d, n=1, s=seq):
        plan = abi.TransformPlan()
        plan.channels[0] = 77
        st = L.hmgpu_transform_plan_for(C.byref(s), C.byref(d), n, C.byref(plan))
        assert st == abi.HMGPU_OK or not any(bytes(plan))                 # a refused call leaves the plan zero
        return st
    ok = abi.make_transform_desc
    assert status(ok()) == abi.HMGPU_OK and status(ok(abi.TRANSFORM_COEFFS, 1, abi.SAMPLE_F32, (0.0, float("nan"), float("inf")))) == abi.HMGPU_OK
    for n in (0, -1, 17):
        assert status(ok(), n) == abi.HMGPU_EINVAL
    assert status(ok(), 16) == abi.HMGPU_OK
    for value in (-1, 2):
        assert status(ok(value)) == abi.HMGPU_EINVAL
    for comps in (0, 8, -1):
        assert status(ok(components=comps)) == abi.HMGPU_EINVAL
    for k in range(6):
        d = ok()
        d.reserved[k] = 1
        assert status(d) == abi.HMGPU_EINVAL
    for st in (abi.SAMPLE_F16, abi.SAMPLE_BF16, abi.SAMPLE_F32):
        assert status(ok(sample_type=st, scale=(1.0, float("nan"), 1.0))) == abi.HMGPU_EINVAL
        assert status(ok(sample_type=st, scale=(float("-inf"), 1.0, 1.0))) == abi.HMGPU_EINVAL
        assert status(ok(components=5, sample_type=st, scale=(1.0, float("nan"), 1.0))) == abi.HMGPU_OK      # Cb is not selected
    assert status(ok(scale=(float("nan"),) * 3)) == abi.HMGPU_OK                                              # int16: the scales are not read
    for st in (-1, 4, 99):
        assert status(ok(sample_type=st)) == abi.HMGPU_EUNSUPPORTED
    bad = abi.make_seq(416, 240, 10, 10)
    bad.chroma_format = 4
    assert status(ok(), s=bad) == abi.HMGPU_EINVAL
    bad = abi.make_seq(412, 240, 10, 10)
    assert status(ok(), s=bad) == abi.HMGPU_EINVAL
    assert L.hmgpu_transform_plan_for(None, C.byref(ok()), 1, C.byref(abi.TransformPlan())) == abi.HMGPU_EINVAL
    assert L.hmgpu_transform_plan_for(C.byref(seq), None, 1, C.byref(abi.TransformPlan())) == abi.HMGPU_EINVAL
    assert L.hmgpu_transform_plan_for(C.byref(seq), C.byref(ok()), 1, None) == abi.HMGPU_EINVAL
    with pytest.raises(ValueError):
        transform.describe("nope")
    with pytest.raises(ValueError):
        transform.describe(scale=(1.0, 1.0, 1.0))                          # a scale needs a float dtype


def test_transform_structs_match_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n",'
                   'sizeof(hmgpu_transform_desc),sizeof(hmgpu_transform_plan),offsetof(hmgpu_transform_desc,sample_type),offsetof(hmgpu_transform_desc,scale),'
                   'offsetof(hmgpu_transform_desc,reserved),offsetof(hmgpu_transform_plan,elem_bytes),offsetof(hmgpu_transform_plan,row_bytes),'
                   'HMGPU_TRANSFORM_LEVELS,HMGPU_TRANSFORM_COEFFS,HMGPU_TRANSFORM_DST_INFO,HMGPU_TRANSFORM_DSTS,HMGPU_TRANSFORM_INFO_CHANNELS);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.TransformDesc), C.sizeof(abi.TransformPlan), abi.TransformDesc.sample_type.offset, abi.TransformDesc.scale.offset,
                   abi.TransformDesc.reserved.offset, abi.TransformPlan.elem_bytes.offset, abi.TransformPlan.row_bytes.offset,
                   abi.TRANSFORM_LEVELS, abi.TRANSFORM_COEFFS, abi.TRANSFORM_DST_INFO, abi.TRANSFORM_DSTS, abi.TRANSFORM_INFO_CHANNELS]
    L = libhm_amd.lib()
    for name in ("hmgpu_transform_plan_for", "hmgpu_pictures_export_transform", "hmgpu_pictures_transform_check", "hmgpu_transform_destination_check"):
        assert hasattr(L, name)
    assert hasattr(hmdec.lib(), "hmdec_pictures_export_transform")
    assert C.sizeof(abi.TransformDesc) == 48 and C.sizeof(abi.TransformPlan) == 96


# ------------------------------------------------------------------------------------------------ 3. the model against hmdec_internal_info
@pytest.mark.parametrize("name", ["ldp_main8_416x240", "intra_444_ccp_main10_208x120", "ldb_422_main10_208x120"])
def test_levels_model_and_info_grid_agree_with_internal_info(name):
    """an independent route to the same facts: the block lists libhmdec builds by walking the transform trees on the host.  A list
    entry is a leaf of its tree when its size is the transform size the grid holds there.  TU_CBF_* against channel 2 (a 4:2:2 unit's
    bit stands for either square; the chroma flags of four 4x4 luma units ride with the first), TU_COEFF_TR_SKIP_* against channel 3,
    CU_INTRA_MODE_* against channels 4 / 5, the energy of every coded luma leaf against the painted block"""
    z = gu.load("stream_" + name)
    counts = dict(leaves=0, coded=0, chroma=0, intra=0, energy=0)
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(p):
            g = p.geometry()
            n, fmt = g["num_ctbs"], g["chroma_format"]
            meta = {mine: p.array(theirs).reshape(n, -1) for theirs, mine in KEYS}
            seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], range_ext_flags=g["range_ext"])
            seq.chroma_format = fmt
            levels = [p.array("coeff%d" % k).reshape(n, -1) for k in range(3)]
            planes = tref.levels_planes(seq, meta, levels)
            info = tref.info_grid(seq, meta)
            assert (info[0] >= 2).all()                                     # whole pictures: every block decoded
            sub = fmt in (1, 2)                                             # subsampled chroma: 4x4 luma units share a chroma block
            for c, (cbf_key, ts_key) in enumerate((("TU_CBF_Y", "TU_COEFF_TR_SKIP_Y"), ("TU_CBF_CB", "TU_COEFF_TR_SKIP_Cb"),
                                                   ("TU_CBF_CR", "TU_COEFF_TR_SKIP_Cr"))):
                ts = {(x, y, w): v for x, y, w, h, v, _ in d.internal_info(p, ts_key)}
                for x, y, w, h, v, _ in d.internal_info(p, cbf_key):
                    bx, by = x // 4, y // 4
                    if (1 << int(info[0, by, bx])) != w:
                        continue                                            # an inner node of the tree
                    if c and sub and w == 4 and (x % 8 or y % 8):
                        continue
                    pcm = bool(info[3, by, bx] & 16)
                    span = max(w, 8 if c and sub else 4) // 4             # (the chroma block of four 4x4 luma units lies under the 8x8 node)
                    cells = info[2, by:by + span, bx:bx + span]
                    coded = bool(((cells >> c) & 1).any())
                    assert coded == (bool(v) and not pcm and w <= 32), (name, p.poc, c, x, y, w)
                    assert bool(info[3, by, bx] & (1 << c)) == bool(ts[(x, y, w)]), (name, p.poc, c, x, y, w)
                    counts["leaves"] += 1
                    counts["coded" if c == 0 else "chroma"] += int(coded)
            for x, y, w, h, v, _ in d.internal_info(p, "TU_COEFF_ENERGY_Y"):
                bx, by = x // 4, y // 4
                if (1 << int(info[0, by, bx])) != w or not (info[2, by, bx] & 1):
                    continue
                e = int((planes[0][y:y + w, x:x + w].astype(np.int64) ** 2).sum())
                assert min(e, 0x7fffffff) == v, (name, p.poc, x, y, w)
                counts["energy"] += int(e > 0)
            for key, chan in (("CU_INTRA_MODE_LUMA", 4), ("CU_INTRA_MODE_CHROMA", 5)):
                for x, y, w, h, v, _ in d.internal_info(p, key):
                    assert int(info[chan, y // 4, x // 4]) == v, (name, p.poc, key, x, y)
                    counts["intra"] += 1
            pm = meta["pred_mode"]
            assert ((info[4] >= 0).sum() > 0) == bool((pm == abi.MODE_INTRA).any())
        d.decode_stream(z["bitstream"], on_output=on_output)
    assert all(v > 0 for v in counts.values()), counts
