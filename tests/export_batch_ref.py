"""numpy restatement of the batched tensor export (include/hmgpu.h "batched tensor export"): the integers of tests/export_ref.py /
tests/scale_ref.py, then for the float types a float32 multiply, a float32 add (two separate ufuncs: two roundings, no fma) and the
cast to the output type, round to nearest even (numpy's astype for float16, torch's CPU conversion for bfloat16)."""
import numpy as np

import libhm_amd
from libhm_amd import abi
from tests import export_ref as ref
from tests import scale_ref as sref

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def integers(seq, planes, fmt, bd, desc, scale=None):
    """the planes of integers v the export of `desc` (scaled when `scale` is given) writes: [R, G, B] or [Y, Cb, Cr] (Y for 4:0:0)"""
    if scale is not None:
        plan = libhm_amd.export_scaled_plan(seq, desc, scale)
        out = sref.export_scaled(planes, fmt, bd, desc, plan, sref.tables(seq, desc, scale))
    elif desc.layout == ref.RGB:
        plan = libhm_amd.export_plan(seq, desc)
        out = ref.export_rgb(planes, fmt, bd, desc.bit_depth[0] or bd[0], list(plan.coef), tuple(desc.crop), bool(desc.msb_aligned))
    else:
        out_bd = (desc.bit_depth[0] or bd[0], desc.bit_depth[1] or bd[1])
        out = ref.export_yuv(planes, fmt, bd, out_bd, desc.layout, tuple(desc.crop), bool(desc.msb_aligned))
    return [np.asarray(p, np.int64) for p in out]


def affine_f32(v, scale_k, bias_k):
    """fl(fl(float32(v) * scale) + bias) in binary32"""
    m = np.multiply(np.asarray(v).astype(np.float32), np.float32(scale_k), dtype=np.float32)
    return np.add(m, np.float32(bias_k), dtype=np.float32)


def cast_bits(f, sample_type):
    """the bit patterns of float32 `f` converted to the sample type: uint16 (float16, bfloat16) or uint32 (float32)"""
    f = np.ascontiguousarray(f, np.float32)
    if sample_type == abi.SAMPLE_F32:
        return f.view(np.uint32)
    with np.errstate(over="ignore"):
        if sample_type == abi.SAMPLE_F16:
            return f.astype(np.float16).view(np.uint16)
    import torch
    return torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def tensor_bits(ints, tensor):
    """per plane k: the bit patterns of convert(v * scale[k] + bias[k])"""
    with np.errstate(over="ignore"):
        return [cast_bits(affine_f32(v, tensor.scale[k], tensor.bias[k]), tensor.sample_type) for k, v in enumerate(ints)]


def export_batch_ref(seq, planes, fmt, bd, desc, scale, tensor):
    """what hmgpu_pictures_export writes for one picture, per plane: integers (tensor None / SAMPLE_UINT) or float bit patterns"""
    ints = integers(seq, planes, fmt, bd, desc, scale)
    if tensor is None or tensor.sample_type == abi.SAMPLE_UINT:
        return ints
    return tensor_bits(ints, tensor)
