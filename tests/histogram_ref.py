"""numpy restatement of the picture histograms (include/hmgpu.h "picture histograms"): np.bincount of the cropped planes, shifted for
reduced bins; the moments in Python integers; maxRGB from export_ref.export_rgb with the plan's coef, maximum over R, G, B."""
import numpy as np

from tests import export_ref

NAMES = ("y", "cb", "cr", "maxrgb")
FIELDS = ("samples", "sum", "sum_sq", "min", "max")
ZERO = {"samples": 0, "sum": 0, "sum_sq": 0, "min": 0, "max": 0, "hist": None, "depth": 0, "log2_bins": 0}


def bins_of(depth, log2_bins):
    """b_c: the depth for log2_bins 0, else the smaller of the two"""
    return depth if not log2_bins else min(log2_bins, depth)


def channel(values, depth, log2_bins=0):
    """one channel's record and histogram of an integer array of values 0 .. 2^depth - 1"""
    v = np.asarray(values).astype(np.int64).ravel()
    b = bins_of(depth, log2_bins)
    # Python integers from int64 sums, which are exact here: v < 2^16 and fewer than 2^31 values, so sum v^2 < 2^63
    assert v.size < 1 << 31 and (v.size == 0 or (0 <= int(v.min()) and int(v.max()) < 1 << 16))
    return {"samples": int(v.size), "sum": int(v.sum(dtype=np.int64)), "sum_sq": int((v * v).sum(dtype=np.int64)), "min": int(v.min()),
            "max": int(v.max()),
            "hist": np.bincount(v >> (depth - b), minlength=1 << b).astype(np.int64), "depth": depth, "log2_bins": b}


def max_rgb(planes, fmt, bit_depths, coef, crop=(0, 0, 0, 0), rgb_bit_depth=0):
    """[H, W]: max(R, G, B) of the RGB export at rgb_bit_depth bits (0: the luma depth)"""
    out_bd = rgb_bit_depth or bit_depths[0]
    return export_ref.export_rgb(planes, fmt, bit_depths, out_bd, [int(c) for c in coef], crop).max(axis=0)


def picture(planes, fmt, bit_depths, channels=(0, 1, 2), log2_bins=0, crop=(0, 0, 0, 0), coef=None, rgb_bit_depth=0):
    """the four channels of one picture: planes the uncropped [Y, Cb, Cr]; a channel that is not computed is ZERO"""
    cp = export_ref.crop_planes(planes, fmt, crop)
    out = []
    for c in range(4):
        if c not in channels or (fmt == 0 and c in (1, 2)):
            out.append(dict(ZERO))
        elif c == 3:
            out.append(channel(max_rgb(planes, fmt, bit_depths, coef, crop, rgb_bit_depth), rgb_bit_depth or bit_depths[0], log2_bins))
        else:
            out.append(channel(cp[c], bit_depths[1 if c else 0], log2_bins))
    return out
