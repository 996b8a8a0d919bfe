"""Picture histograms as torch tensors (hmgpu_pictures_histogram, k_histogram.hip): the argument handling shared by Context.histogram,
hmdec.histogram_batch and hmdec.Picture.histogram, and the helpers that read a result -- mean, variance, percentile, distance,
light_level -- which are torch ops on the result tensors, no kernels.

The result is {"y": {...}, "cb": {...}, "cr": {...}, "maxrgb": {...}}: per channel "hist", an int32 tensor [n, 2^b_c] (absent with
histogram=False, and for a channel that is not computed), and the fields of hmgpu_histogram_result as tensors of shape [n], all views
of one [n, 4, 8] int64 tensor (records()): samples, sum, sum_sq as int64; min and max, which are 32-bit words of the record (the two
halves of its fourth int64), as int32 views of those words, so that no torch op runs to take them apart.  The record of a channel that
is not selected, or that the format lacks, is all zero.  Nothing synchronises: the tensors are written on torch's current stream.
"""
import ctypes as C

from . import abi

NAMES = ("y", "cb", "cr", "maxrgb")
FIELDS = ("samples", "sum", "sum_sq", "min", "max")


def channels_mask(channels):
    """the mask of hmgpu_histogram_desc.channels from names ("y", "cb", "cr", "maxrgb") or indices 0 .. 3, or a mask given as an int"""
    if isinstance(channels, int):
        return channels
    mask = 0
    for c in channels:
        if isinstance(c, str):
            if c.lower() not in NAMES:
                raise ValueError("channel %r: one of %s" % (c, ", ".join(NAMES)))
            c = NAMES.index(c.lower())
        if not 0 <= int(c) <= 3:
            raise ValueError("channel %r: 0 .. 3" % (c,))
        mask |= 1 << int(c)
    return mask


def log2_bins(bins):
    """desc.log2_bins of bins=: None for one bin per code value, else a power of two 16 .. 4096"""
    if bins is None:
        return 0
    b = int(bins)
    if b < 16 or b > 4096 or b & (b - 1):
        raise ValueError("bins=%r: None, or a power of two 16 .. 4096" % (bins,))
    return b.bit_length() - 1


def describe(channels=("y", "cb", "cr"), bins=None, crop=(0, 0, 0, 0), matrix=None, full_range=None, rgb_bit_depth=0, histogram=True):
    """the abi.HistogramDesc of a call; matrix / full_range None: BT.709, limited range (export.resolve_colour without a VUI)"""
    from . import export
    matrix, full_range = export.resolve_colour(matrix, full_range)
    return abi.make_histogram_desc(channels_mask(channels), log2_bins(bins), 1 if histogram else 0, rgb_bit_depth, matrix, full_range, crop)


def plan_for(seq, desc):
    """what a call with `desc` counts (hmgpu_histogram_plan_for: host code, no GPU): an abi.HistogramPlan"""
    from . import HmgpuError, lib
    plan = abi.HistogramPlan()
    st = lib().hmgpu_histogram_plan_for(C.byref(seq), C.byref(desc), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_histogram_plan_for")
    return plan


def histogram(call, seq, device, n, channels=("y", "cb", "cr"), bins=None, crop=(0, 0, 0, 0), matrix=None, full_range=None,
              rgb_bit_depth=0, histogram=True):
    """allocate the histograms and the [n, 4, 8] records with torch on `device` and run
    call(desc, hist pointers[4], hist strides[4], records pointer, records stride, stream) on torch's current stream"""
    import torch
    desc = describe(channels, bins, crop, matrix, full_range, rgb_bit_depth, histogram)
    plan = plan_for(seq, desc)
    with torch.cuda.device(device):
        dev = torch.device("cuda", device)
        rec = torch.empty((n, 4, 8), dtype=torch.int64, device=dev)
        hists = [torch.empty((n, 1 << plan.log2_bins[k]), dtype=torch.int32, device=dev) if histogram and plan.channels[k] else None
                 for k in range(4)]
        call(desc, [None if t is None else t.data_ptr() for t in hists], [0 if t is None else t.stride(0) * 4 for t in hists],
             rec.data_ptr(), rec.stride(0) * 8, torch.cuda.current_stream(device).cuda_stream)
    out = {}
    words = rec.view(torch.int32)                                       # [n, 4, 16]: min and max are the 32-bit words 6 and 7 of a record
    for k in range(4):
        out[NAMES[k]] = {f: rec[:, k, i] for i, f in enumerate(("samples", "sum", "sum_sq"))}
        out[NAMES[k]]["min"], out[NAMES[k]]["max"] = words[:, k, 6], words[:, k, 7]
        if hists[k] is not None:
            out[NAMES[k]]["hist"] = hists[k]
    return out


def records(result):
    """the [n, 4, 8] int64 tensor the fields of a result are views of (min | max << 32 in field 3)"""
    return result["y"]["samples"]._base


def c_args(ptrs, strides):
    """the ctypes arguments (hist[4], hist_batch_stride_bytes[4]) of the C entry points: NULL for what is not given"""
    return (abi.ptr_array(ptrs, 4) if ptrs is not None else None, abi.i64_array(strides, 4) if strides is not None else None)


# ------------------------------------------------------------------------------------------------ reading a result
def mean(ch):
    """the mean value per picture of one channel of a result, float64 [n], from the integer moments"""
    return ch["sum"].double() / ch["samples"].double()


def variance(ch):
    """the (population) variance per picture of one channel, float64 [n]: (samples * sum_sq - sum^2) / samples^2.  The numerator is
    formed in float64: exact to 2^-53 relative per product, which for near-flat pictures of many samples can cancel -- use the
    histogram for those"""
    n, s, q = ch["samples"].double(), ch["sum"].double(), ch["sum_sq"].double()
    return (q / n - (s / n) ** 2).clamp_min(0.0)


def percentile(ch, q):
    """per picture the least bin whose cumulative count is >= q * samples (q in 0 .. 1), int64 [n]; with one bin per code value that
    bin is the value.  q = 0 gives the least occupied bin."""
    import torch
    if not 0.0 <= q <= 1.0:
        raise ValueError("q in 0 .. 1")
    hist = ch["hist"].long()
    cum = hist.cumsum(1)
    total = cum[:, -1:]
    need = torch.ceil(q * total.double()).long().clamp_min(1)
    return (cum < need).sum(1)


def distance(a, b):
    """half the L1 distance of the normalised histograms of two channels, per picture, float64 [n] in 0 .. 1: 0 for equal
    distributions, 1 for disjoint ones -- the usual scene-cut score between neighbouring pictures"""
    ha, hb = a["hist"].double(), b["hist"].double()
    if ha.shape != hb.shape:
        raise ValueError("distance: histograms of the same shape")
    return 0.5 * (ha / ha.sum(1, keepdim=True) - hb / hb.sum(1, keepdim=True)).abs().sum(1)


def light_level(ch, depth, eotf=None):
    """(peak, average) in cd/m2 per picture, float64 [n], of a channel whose histogram has one bin per code value of `depth` bits:
    peak = eotf(v / (2^depth - 1)) of the highest nonzero bin, average = sum hist[v] * eotf(v / (2^depth - 1)) / samples.  eotf maps
    the non-linear value 0 .. 1 to cd/m2 (default export.pq_eotf, ST 2084).  On the maxRGB channel of a PQ picture these are the
    per-picture terms of CTA-861.3: MaxCLL is the maximum of the peaks over a stream, MaxFALL the maximum of the averages.  Needs
    full-depth bins (bins=None): with reduced bins a bin is not a code value."""
    import numpy as np
    import torch
    from . import export
    hist = ch["hist"]
    if hist.shape[1] != 1 << depth:
        raise ValueError("light_level: a histogram with one bin per code value of %d bits (bins=None), not %d bins" % (depth, hist.shape[1]))
    codes = np.arange(1 << depth, dtype=np.float64) / float((1 << depth) - 1)
    light = torch.from_numpy(np.asarray((eotf or export.pq_eotf)(codes), dtype=np.float64)).to(hist.device)
    idx = torch.arange(1 << depth, device=hist.device)
    top = ((hist > 0) * idx).max(1).values
    return light[top], (hist.double() * light).sum(1) / hist.double().sum(1)
