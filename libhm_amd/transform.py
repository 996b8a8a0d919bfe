"""Transform export to torch tensors (hmgpu_pictures_export_transform, k_transform.hip): the argument handling shared by
Context.export_transform, hmdec.export_transform_batch and hmdec.Picture.transform.  No compute here.

The result is a dict: "y" [N, H, W], "cb" / "cr" [N, H >> csy, W >> csx] (4:0:0: "y" only) -- the quantised levels ("levels") or the
de-quantised transform coefficients ("coeffs") of every coded transform block at the block's position, 0 wherever no coded block lies
-- int16 or a float dtype (value = float32(v) * scale[c], converted), and "info" int8 [N, 6, H / 4, W / 4]: per 4x4 luma block the
log2 transform size, tr_idx, the mask of components that hold coefficients there, the transform-skip / bypass / PCM flags and the
intra modes (-1 in all channels where nothing was decoded).  There is no crop: slice the tensors.
"""
from . import abi
from . import export
from .residual import components_mask

VALUES = {"levels": abi.TRANSFORM_LEVELS, "coeffs": abi.TRANSFORM_COEFFS}
NAMES = ("y", "cb", "cr", "info")


def value_code(value):
    try:
        return value if isinstance(value, int) else VALUES[value.lower()]
    except KeyError:
        raise ValueError("unknown transform value %r (levels or coeffs)" % (value,))


def plan_for(seq, desc, n=1):
    """what an export with `desc` writes (hmgpu_transform_plan_for: host code, no GPU)"""
    import ctypes as C
    from . import HmgpuError, lib
    plan = abi.TransformPlan()
    st = lib().hmgpu_transform_plan_for(C.byref(seq), C.byref(desc), n, C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_transform_plan_for")
    return plan


def describe(value="levels", components=(0, 1, 2), dtype=None, scale=None):
    """the abi.TransformDesc of a call; dtype: None (int16), a torch float dtype or an abi.SAMPLE_* code"""
    st = abi.SAMPLE_UINT if dtype is None else dtype if isinstance(dtype, int) else export.sample_type(dtype)
    if scale is not None and st == abi.SAMPLE_UINT:
        raise ValueError("scale needs a float dtype")
    return abi.make_transform_desc(value_code(value), components_mask(components), st, (1.0, 1.0, 1.0) if scale is None else tuple(scale))


def transform_plan(seq, value="levels", components=(0, 1, 2), dtype=None, scale=None, n=1):
    """what Context.export_transform with these arguments writes per picture: an abi.TransformPlan -- per destination slot (Y, Cb, Cr,
    info) the channels, width, height, element size and row bytes"""
    return plan_for(seq, describe(value, components, dtype, scale), n)


def export_transform(call, seq, device, n, value="levels", components=(0, 1, 2), dtype=None, scale=None, out=None, enqueue=True):
    """allocate with torch on `device` (or take the tensors of the dict `out`: only its keys are written) and run
    call(desc, ptrs[4], pitches[4], plane_strides[4], batch_strides[4], stream) on torch's current stream."""
    import torch
    desc = describe(value, components, dtype, scale)
    plan = plan_for(seq, desc, n)
    elem = export.side_dtype(desc.sample_type, dtype)
    info = abi.TRANSFORM_DST_INFO
    names = {k: NAMES[k] for k in range(abi.TRANSFORM_DSTS) if plan.channels[k]}

    def shape(k):
        return (n, plan.channels[k], plan.height[k], plan.width[k]) if k == info else (n, plan.height[k], plan.width[k])
    with torch.cuda.device(device):
        out, ptrs, pitches, pstrides, bstrides = export.side_tensors(out, device, names, shape, lambda k: torch.int8 if k == info else elem,
                                                                     abi.TRANSFORM_DSTS)
        if enqueue:
            call(desc, ptrs, pitches, pstrides, bstrides, torch.cuda.current_stream(device).cuda_stream)
    return out


def c_args(ptrs, pitches, pstrides, bstrides):
    """the ctypes arguments (dst[3], dst_info, pitch[4], plane stride[4], batch stride[4]) of the C entry points"""
    ptrs = list(ptrs) + [None] * (4 - len(ptrs))
    return (abi.ptr_array(ptrs[:3]), abi.addr(ptrs[3]), abi.i64_array(pitches, 4), abi.i64_array(pstrides, 4), abi.i64_array(bstrides, 4))
