"""Picture metrics as torch tensors (hmgpu_pictures_metrics, k_metrics.hip): the argument handling shared by Context.metrics,
hmdec.metrics_batch and hmdec.Picture.metrics, and the host helpers psnr / ssim.  No kernels here.

The result is {"y": {...}, "cb": {...}, "cr": {...}}: per component the fields of hmgpu_metrics_result as int64 tensors of shape [n]
(samples, sse, sad, differing, first_diff, ssim_q32, ssim_windows, max_abs), views of one [n, 3, 8] int64 tensor (records()).  The
unsigned fields are stored as int64: first_diff of a component without a difference is -1 (UINT64_MAX).  The record of a component
that is not selected, or that the format lacks, is all zero.  Nothing synchronises: the tensors are written on torch's current stream.

Metric maps (hmgpu_pictures_metrics_map, k_metrics_map.hip; Context.metrics_map, hmdec.metrics_map_batch, hmdec.Picture.metrics_map) keep
the sums per block: the result is {"y": {"sse": [n, Hb, Wb], ...}, "cb": ..., "cr": ...} with the fields of MAP_FIELDS, views of one
[n, 3, F, Hb, Wb] int64 tensor (maps()), F = 6 with SSIM and 4 without.  The slices of a component that is not compared are zero.
map_samples, map_psnr, map_ssim and mismatch_blocks are torch on the device.
"""
import ctypes as C

from . import abi
from .residual import NAMES, components_mask

FIELDS = ("samples", "sse", "sad", "differing", "first_diff", "ssim_q32", "ssim_windows", "max_abs")
MAP_FIELDS = ("sse", "sad", "differing", "max_abs", "ssim_q32", "ssim_windows")         # HMGPU_METRICS_MAP_*


def describe(ref_pics=None, ref=None, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0), ref_bytes_per_sample=None):
    """the abi.MetricsDesc of a call; exactly one of ref_pics (picture handles) and ref (planes) is given"""
    if (ref_pics is None) == (ref is None):
        raise ValueError("metrics: exactly one of ref_pics= (pictures of the context) and ref= (planar tensors)")
    if ref_pics is not None:
        return abi.make_metrics_desc(abi.METRICS_REF_PICTURES, components_mask(components), 1 if ssim else 0, 0, crop)
    return abi.make_metrics_desc(abi.METRICS_REF_PLANES, components_mask(components), 1 if ssim else 0, ref_bytes_per_sample, crop)


def plan_for(seq, desc):
    """what a call with `desc` compares (hmgpu_metrics_plan_for: host code, no GPU): an abi.MetricsPlan"""
    from . import HmgpuError, lib
    plan = abi.MetricsPlan()
    st = lib().hmgpu_metrics_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_metrics_plan_for")
    return plan


def _ref_planes(ref, n, device):
    """(bytes per sample, pointers[3], pitches[3], batch strides[3]) of the planar reference tensors; None entries stay NULL"""
    import torch
    one = {torch.uint8: 1, torch.int16: 2}
    if hasattr(torch, "uint16"):
        one[torch.uint16] = 2
    ref = list(ref)
    if len(ref) > 3:
        raise ValueError("ref: at most three planes (Y, Cb, Cr)")
    es, ptrs, pitches, bstrides = None, [None] * 3, [0] * 3, [0] * 3
    for k, t in enumerate(ref):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != n or t.dtype not in one or t.get_device() != device:
            raise ValueError("ref[%d]: a uint8, uint16 or int16 tensor [%d, h, w] on device %d" % (k, n, device))
        if es not in (None, one[t.dtype]):
            raise ValueError("ref: planes of one element size")
        es = one[t.dtype]
        if t.stride(2) != 1:
            raise ValueError("ref[%d]: elements dense within a row (stride %s)" % (k, t.stride()))
        ptrs[k], pitches[k], bstrides[k] = t.data_ptr(), t.stride(1) * es, t.stride(0) * es
    if es is None:
        raise ValueError("ref: no plane given")
    return es, ptrs, pitches, bstrides


def metrics(call, seq, device, n, ref_pics=None, ref=None, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0)):
    """allocate the [n, 3, 8] result with torch on `device` and run
    call(desc, ref_pics or None, ptrs[3], pitches[3], batch strides[3], results pointer, results stride, stream) on torch's current
    stream.  ref: planar tensors [n, h_c, w_c] (uint8, uint16 or int16 storage of uint16 values); the entry of a component that is not
    compared may be None and is ignored."""
    import torch
    ptrs = pitches = bstrides = None
    es = None
    if ref is not None:
        mask = components_mask(components)
        ref = [t if (mask >> k) & 1 else None for k, t in enumerate(ref)]       # (a plane of a component that is not compared is left alone)
        es, ptrs, pitches, bstrides = _ref_planes(ref, n, device)
    desc = describe(ref_pics, ref, components, ssim, crop, es)
    plan = plan_for(seq, desc)
    if ref is not None:
        for k in range(3):
            if ptrs[k] is not None and plan.channels[k] and tuple(ref[k].shape[1:]) != (plan.height[k], plan.width[k]):
                raise ValueError("ref[%d]: shape [%d, %d, %d]" % (k, n, plan.height[k], plan.width[k]))
    with torch.cuda.device(device):
        res = torch.empty((n, 3, 8), dtype=torch.int64, device=torch.device("cuda", device))
        call(desc, ref_pics, ptrs, pitches, bstrides, res.data_ptr(), res.stride(0) * 8, torch.cuda.current_stream(device).cuda_stream)
    return {NAMES[k]: {f: res[:, k, i] for i, f in enumerate(FIELDS)} for k in range(3)}


def records(result):
    """the [n, 3, 8] int64 tensor the fields of a result are views of"""
    return result["y"]["samples"]._base


def c_args(ref_pics, ptrs, pitches, bstrides):
    """the ctypes arguments (ref_pics[], ref[3], pitch[3], batch stride[3]) of the C entry points: NULL for what is not given"""
    return (abi.handle_array(list(ref_pics)) if ref_pics is not None else None,
            abi.ptr_array(ptrs) if ptrs is not None else None,
            abi.i64_array(pitches) if pitches is not None else None,
            abi.i64_array(bstrides) if bstrides is not None else None)


def psnr(result, bit_depth):
    """HM's PSNR per picture (hmgpu_metrics_psnr) of one component of a result, e.g. psnr(out["y"], 10): a list of floats, 999.99 for
    identical planes.  Host code: copies the fields to the host, which waits for them."""
    from . import lib
    out = []
    for samples, sse in zip(result["samples"].tolist(), result["sse"].tolist()):
        r = abi.MetricsResult()
        r.samples, r.sse = samples & abi.METRICS_NO_DIFF, sse & abi.METRICS_NO_DIFF
        out.append(float(lib().hmgpu_metrics_psnr(C.byref(r), bit_depth)))
    return out


def ssim(result):
    """mean SSIM per picture of one component of a result: ssim_q32 / 2^32 / ssim_windows (nan without windows); host code"""
    return [q / 4294967296.0 / w if w else float("nan") for q, w in zip(result["ssim_q32"].tolist(), result["ssim_windows"].tolist())]


# ------------------------------------------------------------------------------------------------ metric maps
def map_plan_for(seq, desc, map_desc):
    """what a map call with `desc` and `map_desc` writes (hmgpu_metrics_map_plan_for: host code, no GPU): an abi.MetricsMapPlan"""
    from . import HmgpuError, lib
    plan = abi.MetricsMapPlan()
    st = lib().hmgpu_metrics_map_plan_for(C.byref(seq), C.byref(desc), abi.ref(map_desc), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_metrics_map_plan_for")
    return plan


def map_c_args(maps, pitches, fstrides, bstrides):
    """the ctypes arguments (maps[3], pitch[3], field stride[3], batch stride[3]) of the C entry points: NULL for what is not given"""
    return (abi.ptr_array(maps) if maps is not None else None,
            abi.i64_array(pitches) if pitches is not None else None,
            abi.i64_array(fstrides) if fstrides is not None else None,
            abi.i64_array(bstrides) if bstrides is not None else None)


def metrics_map(call, seq, device, n, ref_pics=None, ref=None, block=16, components=(0, 1, 2), ssim=True, crop=(0, 0, 0, 0)):
    """allocate the [n, 3, F, Hb, Wb] maps with torch on `device` and run
    call(desc, map desc, ref_pics or None, ptrs[3], pitches[3], batch strides[3], maps[3], map pitches[3], field strides[3], batch
    strides[3], stream) on torch's current stream; ref as for metrics().  The slices of the components that are not compared are
    zeroed here: the call writes nothing for them."""
    import torch
    ptrs = pitches = bstrides = None
    es = None
    if ref is not None:
        mask = components_mask(components)
        ref = [t if (mask >> k) & 1 else None for k, t in enumerate(ref)]
        es, ptrs, pitches, bstrides = _ref_planes(ref, n, device)
    desc = describe(ref_pics, ref, components, ssim, crop, es)
    md = abi.make_metrics_map_desc(block)
    plan = map_plan_for(seq, desc, md)
    if ref is not None:
        for k in range(3):
            if ptrs[k] is not None and plan.channels[k] and tuple(ref[k].shape[1:]) != (plan.height[k], plan.width[k]):
                raise ValueError("ref[%d]: shape [%d, %d, %d]" % (k, n, plan.height[k], plan.width[k]))
    with torch.cuda.device(device):
        out = torch.empty((n, 3, plan.fields, plan.blocks_y, plan.blocks_x), dtype=torch.int64, device=torch.device("cuda", device))
        maps = [None] * 3
        for k in range(3):
            if plan.channels[k]:
                maps[k] = out[:, k].data_ptr()
            else:
                out[:, k].zero_()
        call(desc, md, ref_pics, ptrs, pitches, bstrides, maps, [out.stride(3) * 8] * 3, [out.stride(2) * 8] * 3, [out.stride(0) * 8] * 3,
             torch.cuda.current_stream(device).cuda_stream)
    return {NAMES[k]: {f: out[:, k, i] for i, f in enumerate(MAP_FIELDS[:plan.fields])} for k in range(3)}


def maps(result):
    """the [n, 3, F, Hb, Wb] int64 tensor the fields of a map result are views of"""
    return result["y"]["sse"]._base


def map_samples(plan, c, device=None):
    """the samples of component c in every block of a map: an int64 tensor [Hb, Wb], the blocks of the last column and row partial
    (all zero for a component the plan does not compare)"""
    import torch
    bw, bh, w, h = plan.block_w[c], plan.block_h[c], plan.width[c], plan.height[c]
    bx = torch.arange(plan.blocks_x, dtype=torch.int64, device=device)
    by = torch.arange(plan.blocks_y, dtype=torch.int64, device=device)
    if not plan.channels[c]:
        return torch.zeros((plan.blocks_y, plan.blocks_x), dtype=torch.int64, device=device)
    cols = torch.clamp(w - bx * bw, min=0, max=bw)
    rows = torch.clamp(h - by * bh, min=0, max=bh)
    return rows[:, None] * cols[None, :]


def map_psnr(result, samples, bit_depth):
    """HM's PSNR per block of one component of a map result, e.g. map_psnr(out["y"], map_samples(plan, 0, device), 10): a float64
    tensor like result["sse"]; 999.99 where a block has no difference"""
    import torch
    sse = result["sse"]
    maxval = float(255 << (bit_depth - 8))
    ref = maxval * maxval * samples.to(sse.device).to(torch.float64)
    psnr = 10.0 * torch.log10(ref / sse.clamp(min=1).to(torch.float64))
    return torch.where(sse == 0, torch.full_like(psnr, 999.99), psnr)


def map_ssim(result):
    """mean SSIM per block of one component of a map result: ssim_q32 / 2^32 / ssim_windows as float64, NaN where no window starts"""
    import torch
    q, w = result["ssim_q32"].to(torch.float64), result["ssim_windows"]
    v = q / 4294967296.0 / w.clamp(min=1).to(torch.float64)
    return torch.where(w == 0, torch.full_like(v, float("nan")), v)


def mismatch_blocks(result):
    """the (i, by, bx) of every block of one component of a map result in which a sample differs: an int64 tensor [k, 3] -- every
    place where two decodes disagree, not only the first (torch.nonzero: waits for the maps)"""
    import torch
    return torch.nonzero(result["differing"] > 0)
