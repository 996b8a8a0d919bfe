"""Batched tensor export, host side (no GPU): the new struct's size, hmgpu_export_tensor_plan_for's geometry and refusals,
export.affine's constants, and the numpy restatement (tests/export_batch_ref.py) against double precision."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_batch_ref as bref
from tests import export_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = [(abi.SAMPLE_F16, 2), (abi.SAMPLE_BF16, 2), (abi.SAMPLE_F32, 4)]


def seq_of(w, h, fmt, bd_y, bd_c=None):
    s = abi.make_seq(w, h, bd_y, bd_c if bd_c is not None else bd_y)
    s.chroma_format = fmt
    return s


def plan_status(seq, desc, scale, tensor):
    plan = abi.ExportPlan()
    st = libhm_amd.lib().hmgpu_export_tensor_plan_for(C.byref(seq), C.byref(desc), C.byref(scale) if scale is not None else None,
                                                      C.byref(tensor) if tensor is not None else None, C.byref(plan))
    return st, plan


def test_struct_size_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %d %d %d %d %d\\n",sizeof(hmgpu_export_tensor),'
                   'HMGPU_SAMPLE_UINT,HMGPU_SAMPLE_F16,HMGPU_SAMPLE_BF16,HMGPU_SAMPLE_F32,HMGPU_EXPORT_MAX_BATCH);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.ExportTensor), abi.SAMPLE_UINT, abi.SAMPLE_F16, abi.SAMPLE_BF16, abi.SAMPLE_F32, abi.EXPORT_MAX_BATCH]


def same_but_row_bytes(a, b):
    return (a.planes == b.planes and list(a.width) == list(b.width) and list(a.height) == list(b.height) and list(a.coef) == list(b.coef))


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", [ref.PLANAR, ref.RGB])
@pytest.mark.parametrize("depth,nbytes", [(8, 1), (10, 2)])
def test_plan_row_bytes_and_other_fields(fmt, layout, depth, nbytes):
    seq = seq_of(200, 72, fmt, 10)
    desc = abi.make_export_desc(layout, depth, nbytes, 0, (4, 8, 2, 6), 1, 0)
    for scale in (None, abi.make_export_scale(100, 36, abi.SCALE_BICUBIC)):
        base = libhm_amd.export_plan(seq, desc) if scale is None else libhm_amd.export_scaled_plan(seq, desc, scale)
        for st_type, size in FLOATS:
            st, plan = plan_status(seq, desc, scale, abi.make_export_tensor(st_type))
            assert st == abi.HMGPU_OK
            assert same_but_row_bytes(plan, base)
            assert [plan.row_bytes[k] for k in range(plan.planes)] == [size * plan.width[k] for k in range(plan.planes)]
        for tensor in (None, abi.make_export_tensor(abi.SAMPLE_UINT)):          # unsigned: the existing plan, row_bytes included
            st, plan = plan_status(seq, desc, scale, tensor)
            assert st == abi.HMGPU_OK and same_but_row_bytes(plan, base) and list(plan.row_bytes) == list(base.row_bytes)


def test_plan_refusals():
    E, U = abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
    seq = seq_of(200, 72, 1, 10)
    mk, mt = abi.make_export_desc, abi.make_export_tensor
    ok = mk(ref.RGB, 8, 1)
    assert plan_status(seq, ok, None, mt(abi.SAMPLE_F16))[0] == abi.HMGPU_OK
    assert plan_status(seq, ok, None, mt(4))[0] == E and plan_status(seq, ok, None, mt(-1))[0] == E        # unknown sample type
    for k in range(5):                                                                                   # reserved words
        for st_type in (abi.SAMPLE_UINT, abi.SAMPLE_F32):
            t = mt(st_type)
            t.reserved[k] = 1
            assert plan_status(seq, ok, None, t)[0] == E
    assert plan_status(seq, mk(ref.RGB, 10, 2, 1), None, mt(abi.SAMPLE_F16))[0] == E                       # msb_aligned with a float type
    assert plan_status(seq, mk(ref.RGB, 10, 2, 1), None, mt(abi.SAMPLE_UINT))[0] == abi.HMGPU_OK
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in range(3):
            s, b = [1.0] * 3, [0.0] * 3
            s[k] = bad
            assert plan_status(seq, ok, None, mt(abi.SAMPLE_BF16, s, b))[0] == E
            assert plan_status(seq, ok, None, mt(abi.SAMPLE_BF16, b, s))[0] == E
    assert plan_status(seq, mk(ref.RGB, 8, 2), None, mt(abi.SAMPLE_F16))[0] == E                           # 2 bytes where depth 8 needs 1
    assert plan_status(seq, mk(ref.RGB, 8, 2), None, None)[0] == abi.HMGPU_OK                              # (fine for unsigned)
    assert plan_status(seq, mk(ref.RGB, 10, 1), None, mt(abi.SAMPLE_F16))[0] == E                          # 1 byte where depth 10 needs 2
    assert plan_status(seq_of(200, 72, 1, 8), mk(ref.PLANAR, 0, 2), None, mt(abi.SAMPLE_F32))[0] == E      # 0 = coding depth 8: needs 1
    assert plan_status(seq_of(200, 72, 1, 8), mk(ref.PLANAR, 0, 1), None, mt(abi.SAMPLE_F32))[0] == abi.HMGPU_OK
    assert plan_status(seq, mk(ref.PLANAR, (8, 10), 2), None, mt(abi.SAMPLE_F32))[0] == abi.HMGPU_OK       # the deeper plane decides
    assert plan_status(seq, mk(ref.SEMIPLANAR, 8, 1), None, mt(abi.SAMPLE_F16))[0] == U                   # semi-planar floats
    assert plan_status(seq, mk(ref.SEMIPLANAR, 8, 1), abi.make_export_scale(100, 36), mt(abi.SAMPLE_F16))[0] == U
    assert plan_status(seq, mk(ref.SEMIPLANAR, 8, 1), None, mt(abi.SAMPLE_UINT))[0] == abi.HMGPU_OK
    # the descriptor's and the scale's own refusals stay: reserved fields there
    d = mk(ref.RGB, 8, 1)
    d.reserved[0] = 1
    assert plan_status(seq, d, None, mt(abi.SAMPLE_F16))[0] == E
    sc = abi.make_export_scale(100, 36)
    sc.reserved[0] = 1
    assert plan_status(seq, ok, sc, mt(abi.SAMPLE_F16))[0] == E


@pytest.mark.parametrize("depth", [8, 10, 12])
def test_affine_constants(depth):
    for mean, std in ((None, None), (bref.IMAGENET_MEAN, bref.IMAGENET_STD)):
        scale, bias = export.affine(depth, mean, std)
        m, s = mean or (0.0,) * 3, std or (1.0,) * 3
        for k in range(3):
            assert isinstance(scale[k], np.float32) and isinstance(bias[k], np.float32)
            assert scale[k] == np.float32(1.0 / (((1 << depth) - 1) * s[k]))
            assert bias[k] == np.float32(-m[k] / s[k])
    scale, bias = export.affine(depth)
    assert bias == (0.0,) * 3 and bref.affine_f32((1 << depth) - 1, scale[0], bias[0]) == np.float32(1.0)     # values in [0, 1]
    t = export.make_tensor(__import__("torch").float16, depth, bref.IMAGENET_MEAN, bref.IMAGENET_STD, scale=(2.0, 3.0, 4.0))
    assert list(t.scale) == [2.0, 3.0, 4.0] and list(t.bias) == [float(b) for b in export.affine(depth, bref.IMAGENET_MEAN, bref.IMAGENET_STD)[1]]


@pytest.mark.parametrize("mean,std", [(None, None), (bref.IMAGENET_MEAN, bref.IMAGENET_STD)])
def test_restatement_against_double(mean, std):
    """every v of a 10-bit plane: the two binary32 roundings stay within 4 * 2^-24 * (|v * scale| + |bias|) of double precision"""
    scale, bias = export.affine(10, mean, std)
    v = np.arange(1024, dtype=np.int64)
    for k in range(3):
        got = bref.affine_f32(v, scale[k], bias[k]).astype(np.float64)
        prod = v.astype(np.float64) * float(scale[k])
        want = prod + float(bias[k])
        assert np.all(np.abs(got - want) <= 4 * 2.0 ** -24 * (np.abs(prod) + abs(float(bias[k]))))


def test_restatement_uses_the_existing_references():
    """the integer planes are export_ref's / scale_ref's; the float bits follow from them plane by plane"""
    seq = seq_of(40, 16, 1, 10)
    rng = np.random.default_rng(1)
    planes = [rng.integers(0, 1024, (16, 40)).astype(np.int16)] + [rng.integers(0, 1024, (8, 20)).astype(np.int16) for _ in range(2)]
    desc = abi.make_export_desc(ref.RGB, 8, 1, 0, (0, 0, 0, 0), 1, 0)
    plan = libhm_amd.export_plan(seq, desc)
    ints = bref.integers(seq, planes, 1, (10, 10), desc)
    assert np.array_equal(np.stack(ints), ref.export_rgb(planes, 1, (10, 10), 8, list(plan.coef)))
    t = abi.make_export_tensor(abi.SAMPLE_F16, *export.affine(8, bref.IMAGENET_MEAN, bref.IMAGENET_STD))
    bits = bref.export_batch_ref(seq, planes, 1, (10, 10), desc, None, t)
    for k in range(3):
        want = ((ints[k].astype(np.float32) * np.float32(t.scale[k])) + np.float32(t.bias[k])).astype(np.float16)
        assert np.array_equal(bits[k], want.view(np.uint16))
    # the documented edges of float16: 65520 and above overflow to +inf, 65519 rounds to 65504, 2^-20 * v is subnormal below v = 64 and kept
    edge = bref.cast_bits(bref.affine_f32(np.array([65519, 65520, 65535]), 1.0, 0.0), abi.SAMPLE_F16)
    assert list(edge) == [0x7BFF, 0x7C00, 0x7C00]
    sub = bref.cast_bits(bref.affine_f32(np.array([1, 16, 1023]), 2.0 ** -20, 0.0), abi.SAMPLE_F16)
    assert list(sub) == [0x0010, 0x0100, 0x13FE]          # 16 and 256 units of 2^-24 (subnormal: v < 64), then a normal number
