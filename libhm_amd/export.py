"""Device export to torch tensors: layout names, output dtypes and the colour policy shared by Context.export and
hmdec.Picture.export.  No compute here: the conversion is k_export.hip behind hmgpu_picture_export.

Colour policy (the one place it is decided): an RGB export takes `matrix` / `full_range` from the caller; where the caller leaves
them None they come from the picture's VUI (matrix_coefficients, video_full_range_flag).  A stream without a colour description
(matrix 2, "unspecified") is treated as BT.709 (matrix 1); without video_signal_type it is limited range (E.3.1's default).  Codes
the kernel does not implement (anything but 0, 1, 5, 6, 9) are refused with HMGPU_EUNSUPPORTED rather than guessed.

Tensor output (export_batch, dtype=): float16 / bfloat16 / float32 elements take fl(fl(v * scale_k) + bias_k) of the integer v the
export writes, with (scale, bias) from `affine`: v / (2^D - 1) normalised by a per-plane mean and std.
"""
import collections
import ctypes as C

import numpy as np

from . import abi

LAYOUTS = {"planar": abi.EXPORT_PLANAR, "yuv": abi.EXPORT_PLANAR, "semiplanar": abi.EXPORT_SEMIPLANAR, "nv12": abi.EXPORT_SEMIPLANAR,
           "rgb": abi.EXPORT_RGB}
UNSPECIFIED = 2
PIXELS = {"rgb": abi.PIXEL_RGB, "bgr": abi.PIXEL_BGR, "rgba": abi.PIXEL_RGBA, "bgra": abi.PIXEL_BGRA, "argb": abi.PIXEL_ARGB,
          "abgr": abi.PIXEL_ABGR}
FILTERS = {"nearest": abi.SCALE_NEAREST, "nearest-exact": abi.SCALE_NEAREST, "bilinear": abi.SCALE_BILINEAR, "bicubic": abi.SCALE_BICUBIC,
           "area": abi.SCALE_AREA}


def resolve_colour(matrix, full_range, vui_matrix=UNSPECIFIED, vui_full_range=0):
    """(matrix, full_range) for an RGB export: the caller's values, else the VUI's, with 'unspecified' read as BT.709"""
    if matrix is None:
        matrix = 1 if vui_matrix == UNSPECIFIED else vui_matrix
    if full_range is None:
        full_range = int(vui_full_range)
    return int(matrix), int(full_range)


def torch_dtype(bytes_per_sample):
    """uint8, or for 2-byte samples torch.uint16 where this torch has it, else int16 holding the same bits"""
    import torch
    if bytes_per_sample == 1:
        return torch.uint8
    return getattr(torch, "uint16", torch.int16)


def layout_code(layout):
    if isinstance(layout, int):
        return layout
    try:
        return LAYOUTS[layout.lower()]
    except KeyError:
        raise ValueError("unknown export layout %r (one of %s)" % (layout, ", ".join(sorted(LAYOUTS))))


def make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned=False, seq=None, chroma_format=None):
    """bit_depth: an int for every channel type, a (luma, chroma) pair, or None / 0 for the coding bit depths.  seq (float output):
    the container is the one the output depths need (1 byte when none exceeds 8), the coding depths taken from the sequence;
    chroma_format: the output format of a format export (plane_depths)"""
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    if seq is not None:
        nbytes = 2 if max(plane_depths(seq, layout_code(layout), bd, chroma_format)) > 8 else 1
    else:
        nbytes = 2 if msb_aligned or max(bd) > 8 or min(bd) == 0 else 1
    return abi.make_export_desc(layout_code(layout), bd, nbytes, msb_aligned, tuple(crop), matrix, full_range)


def plane_depths(seq, layout, bd, chroma_format=None):
    """the integer depth D of every output plane: RGB the luma output depth three times; YUV luma, chroma, chroma (4:0:0: luma).
    chroma_format: None, or the output format of a format export, which decides whether there is chroma"""
    y = bd[0] or seq.bit_depth_luma
    if layout == abi.EXPORT_RGB:
        return (y, y, y)
    if (seq.chroma_format if chroma_format is None else chroma_format) == 0:
        return (y,)
    c = bd[1] or seq.bit_depth_chroma
    return (y, c, c)


def affine(depth, mean=None, std=None):
    """(scale, bias), float32 triples, that map an integer sample v of `depth` bits (an int, or one per plane) to
    (v / (2^depth - 1) - mean_k) / std_k:  scale_k = 1 / ((2^D - 1) * std_k), bias_k = -mean_k / std_k, each computed in double and
    rounded once.  mean None: 0, std None: 1 (values in [0, 1])."""
    d = (depth,) * 3 if isinstance(depth, int) else tuple(depth) + (depth[-1],) * (3 - len(depth))
    mean = (0.0,) * 3 if mean is None else tuple(float(m) for m in mean)
    std = (1.0,) * 3 if std is None else tuple(float(v) for v in std)
    scale = tuple(np.float32(1.0 / (float((1 << d[k]) - 1) * std[k])) for k in range(3))
    bias = tuple(np.float32(-mean[k] / std[k]) for k in range(3))
    return scale, bias


def sample_type(dtype):
    """abi.SAMPLE_* of a torch float dtype"""
    import torch
    try:
        return {torch.float16: abi.SAMPLE_F16, torch.bfloat16: abi.SAMPLE_BF16, torch.float32: abi.SAMPLE_F32}[dtype]
    except KeyError:
        raise ValueError("dtype %r: None (unsigned integers), torch.float16, torch.bfloat16 or torch.float32" % (dtype,))


def side_dtype(code, dtype):
    """the torch element type of a side-information export whose description says abi.SAMPLE_* `code`: int16 for the integer type, else
    `dtype` itself -- a torch float dtype, or its abi.SAMPLE_* code"""
    import torch
    if code == abi.SAMPLE_UINT:
        return torch.int16
    return {abi.SAMPLE_F16: torch.float16, abi.SAMPLE_BF16: torch.bfloat16, abi.SAMPLE_F32: torch.float32}[dtype] if isinstance(dtype, int) else dtype


def make_tensor(dtype, depths, mean=None, std=None, scale=None, bias=None):
    """the abi.ExportTensor of a float dtype (None for dtype None): `affine` of the planes' depths, or an explicit scale / bias"""
    if dtype is None:
        if any(v is not None for v in (mean, std, scale, bias)):
            raise ValueError("mean / std / scale / bias need a float dtype")
        return None
    sc, bi = affine(depths, mean, std)
    if scale is not None:
        sc = tuple(scale)
    if bias is not None:
        bi = tuple(bias)
    return abi.make_export_tensor(sample_type(dtype), sc, bi)


def make_scale(size, filter="bilinear"):
    """size: (height, width) or None (no scaling)"""
    if size is None:
        return None
    if isinstance(filter, str):
        if filter.lower() not in FILTERS:
            raise ValueError("unknown filter %r (one of %s)" % (filter, ", ".join(sorted(FILTERS))))
        filter = FILTERS[filter.lower()]
    h, w = (int(v) for v in size)
    return abi.make_export_scale(w, h, filter)


def make_windows(seq, crop, windows, flip, n):
    """the abi.ExportWindow list of n pictures (None when neither windows nor flip is given).  windows: one (x, y, w, h) per picture
    in luma samples relative to `crop` (left, right, top, bottom), inside it; None: all of `crop`.  flip: one boolean per picture, or
    None.  The two are composed into absolute crops: the call then takes a descriptor whose own crop is 0."""
    if windows is None and flip is None:
        return None
    l, r, t, b = (int(v) for v in crop)
    cw, ch = seq.width - l - r, seq.height - t - b
    windows = [(0, 0, cw, ch)] * n if windows is None else [tuple(int(v) for v in w) for w in windows]
    flip = [False] * n if flip is None else [bool(f) for f in flip]
    if len(windows) != n or len(flip) != n:
        raise ValueError("windows / flip: one per picture (%d pictures, %d windows, %d flips)" % (n, len(windows), len(flip)))
    out = []
    for (x, y, w, h), f in zip(windows, flip):
        if x < 0 or y < 0 or w <= 0 or h <= 0 or x + w > cw or y + h > ch:
            raise ValueError("window %r leaves the %dx%d crop" % ((x, y, w, h), cw, ch))
        out.append(abi.make_export_window((l + x, seq.width - (l + x) - w, t + y, seq.height - (t + y) - h), f))
    return out


def dense_windows(seq, crop, windows, flip, n):
    """make_windows for the dense forms of the motion and residual exports, which always take windows: None is all of `crop`"""
    l, r, t, b = (int(v) for v in crop)
    return make_windows(seq, crop, windows if windows is not None else [(0, 0, seq.width - l - r, seq.height - t - b)] * n, flip, n)


def side_plan(entry, plan, seq, desc, scale=None, windows=None, n=None):
    """hmgpu_motion_plan_for / hmgpu_residual_plan_for (`entry`, host code, no GPU) into `plan`, an empty abi.MotionPlan /
    abi.ResidualPlan; windows: abi.ExportWindow per picture (dense); n: the number of pictures (default: one per window, else 1)"""
    from . import HmgpuError, lib
    windows = None if windows is None else list(windows)
    count = n if n is not None else (len(windows) if windows is not None else 1)
    st = getattr(lib(), entry)(C.byref(seq), C.byref(desc), abi.ref(scale), count, abi.window_array(windows), C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, entry)
    return plan


def side_tensors(out, device, names, shape, dtype, slots, rule="elements dense within a row"):
    """the result dict of a motion or residual export and its destinations.  names: slot -> key; shape(k) / dtype(k): of slot k's
    tensor.  out None: every tensor allocated on `device`; else a dict with some of the keys, each a tensor of that shape, dtype and
    device whose rows are dense (a 5-d tensor: its pairs of channels equally far apart).  Returns (out, pointers, pitches, plane
    strides, batch strides), bytes, `slots` long; a slot without a tensor: None / 0; a plane stride: 0 for [N, H, W]."""
    import torch
    if out is None:
        out = {name: torch.empty(shape(k), dtype=dtype(k), device=torch.device("cuda", device)) for k, name in names.items()}
    for key in out:
        if key not in names.values():
            raise ValueError("out: no tensor %r in this export (one of %s)" % (key, ", ".join(sorted(names.values()))))
    ptrs, pitches, pstrides, bstrides = [None] * slots, [0] * slots, [0] * slots, [0] * slots
    for k, name in names.items():
        t = out.get(name)
        if t is None:
            continue
        want = shape(k)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want or t.dtype != dtype(k) or t.get_device() != device:
            raise ValueError("out[%r]: a %s tensor of shape %s on device %d" % (name, dtype(k), want, device))
        st, es = t.stride(), t.element_size()
        if st[-1] != 1 or (len(want) == 5 and st[1] != 2 * st[2]):
            raise ValueError("out[%r]: %s (stride %s)" % (name, rule, st))
        ptrs[k], pitches[k], bstrides[k] = t.data_ptr(), st[-2] * es, st[0] * es
        pstrides[k] = st[-3] * es if len(want) > 3 else 0
    return out, ptrs, pitches, pstrides, bstrides


def random_resized_crop(n, width, height, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), p_flip=0.5, generator=None, chroma_format=1):
    """(windows, flips) for n pictures of width x height: torchvision's RandomResizedCrop sampling rule per picture -- up to ten
    tries of an area fraction uniform in `scale` and an aspect ratio log-uniform in `ratio`, the first that fits placed uniformly,
    else the central crop of the nearest allowed ratio -- and a flip with probability p_flip.  Each window (x, y, w, h) is then
    snapped outwards to whole chroma samples of chroma_format (0 .. 3) and clamped to the picture.  Deterministic for a seeded
    torch.Generator (CPU); feed the result to export_batch(windows=, flip=)."""
    import math
    import torch
    mx = 0 if chroma_format in (0, 3) else 1
    my = 1 if chroma_format == 1 else 0
    area = float(width * height)
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))

    def uniform(a, b):
        return float(torch.empty(1).uniform_(float(a), float(b), generator=generator).item())

    def randint(hi):
        return int(torch.randint(0, hi, (1,), generator=generator).item())

    windows, flips = [], []
    for _ in range(n):
        for _try in range(10):
            target = area * uniform(scale[0], scale[1])
            aspect = math.exp(uniform(log_ratio[0], log_ratio[1]))
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= width and 0 < h <= height:
                y, x = randint(height - h + 1), randint(width - w + 1)
                break
        else:
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            y, x = (height - h) // 2, (width - w) // 2
        x0, y0 = x & ~mx, y & ~my
        x1, y1 = min((x + w + mx) & ~mx, width), min((y + h + my) & ~my, height)
        windows.append((x0, y0, x1 - x0, y1 - y0))
        flips.append(bool(torch.rand(1, generator=generator).item() < p_flip))
    return windows, flips


# ------------------------------------------------------------------------------------------------ warp maps (include/hmgpu.h "affine warp export")
# A map is six Q16 ints m: source sample index (x, y) = (m0*ox + m1*oy + m2, m3*ox + m4*oy + m5) / 65536 for the output pixel
# (ox, oy); the source is the window of the slot.  Sizes are (height, width), as size= of the exports.
WARP_IDENTITY = (65536, 0, 0, 0, 65536, 0)


def _q16(v):
    """round half away from zero to Q16"""
    import math
    v = float(v) * 65536.0
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def one_map(warp):
    """warp= of the single-picture exports: None, one map of six ints, or a list / [1, 6] array of one map; returns None or [map]"""
    if warp is None:
        return None
    warp = list(warp)
    return [warp] if len(warp) == 6 and not hasattr(warp[0], "__len__") else warp


def affine_map(out_size, src_size, angle=0.0, scale=1.0, shear=(0.0, 0.0), translate=(0.0, 0.0), centre=None):
    """the inverse map of torchvision's affine parameterisation -- the picture sheared (degrees, x then y), scaled, rotated by
    `angle` degrees about `centre` (counter-clockwise positive, as F.rotate), then moved by translate=(tx, ty) output samples -- from
    the out_size (height, width) output onto the src_size source.  centre: (cx, cy) in source samples, a sample's centre at
    index + 0.5; None: the middle of the source, which lands in the middle of the output.  The inverse is computed in float64 with
    the half-sample centres folded in (source index = A (o + 0.5) + b - 0.5) and each value rounded half away from zero to Q16."""
    import math
    oh, ow = (float(v) for v in out_size)
    sh, sw = (float(v) for v in src_size)
    cx, cy = (sw / 2.0, sh / 2.0) if centre is None else (float(centre[0]), float(centre[1]))
    if not isinstance(shear, (tuple, list)):
        shear = (shear, 0.0)
    rot, sx, sy = -math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    inv = (d / scale, -b / scale, -c / scale, a / scale)
    px, py = 0.5 - ow / 2.0 - float(translate[0]), 0.5 - oh / 2.0 - float(translate[1])
    bx = inv[0] * px + inv[1] * py + cx - 0.5
    by = inv[2] * px + inv[3] * py + cy - 0.5
    return tuple(_q16(v) for v in (inv[0], inv[1], bx, inv[2], inv[3], by))


def random_affine(n, out_size, src_size, degrees=0.0, translate=None, scale=None, shear=None, generator=None):
    """n maps (affine_map) sampled as torchvision's RandomAffine.get_params samples them: angle uniform in degrees (a number d:
    (-d, d)); translate (a, b): tx, ty uniform within a, b times the output width, height and rounded; scale (lo, hi): uniform;
    shear: a number s (x in (-s, s)), (lo, hi) (x), or (xlo, xhi, ylo, yhi).  Deterministic for a seeded torch.Generator (CPU)."""
    import torch

    def uniform(lo, hi):
        return float(torch.empty(1).uniform_(float(lo), float(hi), generator=generator).item())

    deg = (-float(degrees), float(degrees)) if not isinstance(degrees, (tuple, list)) else tuple(degrees)
    if shear is not None and not isinstance(shear, (tuple, list)):
        shear = (-float(shear), float(shear))
    maps = []
    for _ in range(n):
        angle = uniform(deg[0], deg[1])
        tx = ty = 0.0
        if translate is not None:
            mx, my = float(translate[0]) * out_size[1], float(translate[1]) * out_size[0]
            tx, ty = float(round(uniform(-mx, mx))), float(round(uniform(-my, my)))
        sc = uniform(scale[0], scale[1]) if scale is not None else 1.0
        shx = shy = 0.0
        if shear is not None:
            shx = uniform(shear[0], shear[1])
            if len(shear) == 4:
                shy = uniform(shear[2], shear[3])
        maps.append(affine_map(out_size, src_size, angle, sc, (shx, shy), (tx, ty)))
    return maps


def orientation_map(k, vflip=False, hflip=False, src_size=None):
    """(map, out_size) of a display orientation: the src_size (height, width) source mirrored (vflip: top to bottom, hflip: left to
    right), then turned by k quarter turns counter-clockwise (torch.rot90's k).  Built in integers: every value is an exact multiple
    of 65536, so the export is a permutation of the source under either filter.  k = 1 with hflip is the transpose."""
    h, w = (int(v) for v in src_size)
    k %= 4
    # the source (x, y) in the mirrored picture as (a, b, c): a*ox + b*oy + c
    if k == 0:
        fx, fy, out = (1, 0, 0), (0, 1, 0), (h, w)
    elif k == 1:
        fx, fy, out = (0, -1, w - 1), (1, 0, 0), (w, h)
    elif k == 2:
        fx, fy, out = (-1, 0, w - 1), (0, -1, h - 1), (h, w)
    else:
        fx, fy, out = (0, 1, 0), (-1, 0, h - 1), (w, h)
    if hflip:
        fx = (-fx[0], -fx[1], w - 1 - fx[2])
    if vflip:
        fy = (-fy[0], -fy[1], h - 1 - fy[2])
    return tuple(65536 * v for v in fx + fy), out


def plane_shapes(plan, desc):
    """the shape of every plane tensor: [H, W], or [H, W, 2] for the CbCr plane of the semi-planar layout"""
    return [(plan.height[k], plan.width[k], 2) if desc.layout == abi.EXPORT_SEMIPLANAR and k == 1 else (plan.height[k], plan.width[k])
            for k in range(plan.planes)]


def _check_tensor(t, desc, device, dtype=None):
    import torch
    if dtype is not None:
        if t.dtype != dtype:
            raise ValueError("out: dtype %s, asked for %s" % (t.dtype, dtype))
    elif t.dtype != torch_dtype(desc.bytes_per_sample) and not (desc.bytes_per_sample == 2 and t.dtype == torch.int16):
        raise ValueError("out: dtype %s, the plan gives %s" % (t.dtype, torch_dtype(desc.bytes_per_sample)))
    if t.get_device() != device:
        raise ValueError("out: on device %d, the picture is on %d" % (t.get_device(), device))


def out_spans(out, plan, desc, device, n=None, dtype=None, stacked=False):
    """a caller's destination as (pointers, pitches in bytes, batch strides in bytes or None) per plane.  n None, one picture: RGB
    one [3, H, W] tensor or three planes, YUV a tuple of planes.  n pictures: the same with a leading dimension of n ([n, 3, H, W];
    planes [n, H, W], [n, Hc, Wc, 2]).  Each plane has the planned shape and dtype on the device and its samples dense within a
    row; rows, planes and batch entries may be any stride apart (e.g. a view batch[i]).  Reads only shapes, strides and pointers:
    no views are made.  stacked: the planar layout at 4:4:4 (a format export), Y, Cb and Cr as the channels of one tensor like R, G, B."""
    import torch
    shapes = plane_shapes(plan, desc)
    lead = () if n is None else (n,)
    b = len(lead)
    if stacked and not isinstance(out, torch.Tensor):
        raise ValueError("out: the planar layout at chroma_format 4:4:4 takes one %s tensor" % (lead + (3,) + shapes[0],))
    if isinstance(out, torch.Tensor):
        if desc.layout != abi.EXPORT_RGB and not stacked:
            raise ValueError("out: the planar / semi-planar layouts take a tuple of planes")
        h, w = shapes[0]
        if out.shape != lead + (3, h, w):
            raise ValueError("out: shape %s, the plan gives %s" % (tuple(out.shape), lead + (3, h, w)))
        _check_tensor(out, desc, device, dtype)
        st = out.stride()
        s0, s1, s2 = st[b:]
        if s2 != 1 or s1 < w or s0 < s1 * (h - 1) + w:
            raise ValueError("out: the planes' samples must be dense within a row, rows and planes apart (stride %s)" % (st,))
        es, base = out.element_size(), out.data_ptr()
        return [base + k * s0 * es for k in range(3)], [s1 * es] * 3, [st[0] * es] * 3 if b else None
    planes = tuple(out)
    if len(planes) != len(shapes):
        raise ValueError("out: %d planes, the plan gives %d" % (len(planes), len(shapes)))
    ptrs, pitches, bstrides = [], [], []
    for p, shape in zip(planes, shapes):
        if not isinstance(p, torch.Tensor) or p.shape != lead + shape:
            raise ValueError("out: a plane is not a tensor of shape %s" % (lead + shape,))
        _check_tensor(p, desc, device, dtype)
        st = p.stride()
        inner = (1,) if len(shape) == 2 else (2, 1)
        if st[b + 1:] != inner or st[b] < shape[1] * inner[0]:
            raise ValueError("out: a plane's samples must be dense within a row (stride %s)" % (st,))
        ptrs.append(p.data_ptr())
        pitches.append(st[b] * p.element_size())
        bstrides.append(st[0] * p.element_size())
    return ptrs, pitches, bstrides if b else None


def alloc_outputs(plan, desc, device, n=None, dtype=None, stacked=False):
    """torch tensors for what `plan` describes: RGB [3, H, W]; planar (Y, Cb, Cr) 2-D; semi-planar (Y [H, W], CbCr [Hc, Wc, 2]);
    with n, each with a leading dimension of n.  dtype None: the unsigned type of the container."""
    import torch
    dt = torch_dtype(desc.bytes_per_sample) if dtype is None else dtype
    dev = torch.device("cuda", device)
    lead = () if n is None else (n,)
    if desc.layout == abi.EXPORT_RGB or stacked:
        return torch.empty(lead + (3, plan.height[0], plan.width[0]), dtype=dt, device=dev)
    return tuple(torch.empty(lead + shape, dtype=dt, device=dev) for shape in plane_shapes(plan, desc))


def make_pixel(pixel, alpha, memory_format, layout, dtype, n):
    """the abi.ExportPixel of pixel= / alpha= / memory_format= (None when none is given: the planar call).  pixel: a name of PIXELS
    or an abi.PIXEL_* code; alpha: None (opaque: the largest code value, 1.0 for float elements), else the A element -- an integer
    code value for unsigned elements, a number for float ones; memory_format: None or torch.channels_last (the batch calls, no
    pixel: the bytes of pixel "rgb")"""
    import torch
    if pixel is None and memory_format is None:
        if alpha is not None:
            raise ValueError("alpha needs pixel=")
        return None
    if layout_code(layout) != abi.EXPORT_RGB:
        raise ValueError("pixel / memory_format need layout=\"rgb\"")
    if memory_format is not None:
        if memory_format != torch.channels_last:
            raise ValueError("memory_format: None or torch.channels_last")
        if pixel is not None or alpha is not None:
            raise ValueError("memory_format=torch.channels_last is a [N, 3, H, W] tensor: no pixel= / alpha= with it")
        if n is None:
            raise ValueError("memory_format belongs to the batch calls")
        return abi.make_export_pixel(abi.PIXEL_RGB)
    if isinstance(pixel, str):
        if pixel.lower() not in PIXELS:
            raise ValueError("unknown pixel order %r (one of %s)" % (pixel, ", ".join(sorted(PIXELS))))
        pixel = PIXELS[pixel.lower()]
    if alpha is None:
        return abi.make_export_pixel(pixel)
    if dtype is None:
        if int(alpha) != alpha:
            raise ValueError("alpha: an integer code value for unsigned elements")
        return abi.make_export_pixel(pixel, alpha=int(alpha))
    return abi.make_export_pixel(pixel, alpha_value=float(alpha))


def pixel_channels(px):
    return 3 if px.order in (abi.PIXEL_RGB, abi.PIXEL_BGR) else 4


def alloc_pixels(plan, desc, px, device, n=None, dtype=None, channels_last=False):
    """a torch tensor for the packed plan: [H, W, C], with n [N, H, W, C]; channels_last: that memory seen as [N, C, H, W]"""
    import torch
    dt = torch_dtype(desc.bytes_per_sample) if dtype is None else dtype
    lead = () if n is None else (n,)
    t = torch.empty(lead + (plan.height[0], plan.width[0], pixel_channels(px)), dtype=dt, device=torch.device("cuda", device))
    return t.permute(0, 3, 1, 2) if channels_last else t


def out_pixels(out, plan, desc, px, device, n=None, dtype=None):
    """a caller's packed destination as (pointer, pitch in bytes, batch stride in bytes or None).  n None: [H, W, C]; n pictures:
    [n, H, W, C], or [n, C, H, W] with channels-last strides.  The planned shape and dtype on the device, the pixels dense (the
    elements of a pixel and the pixels of a row side by side); rows and batch entries may be any stride apart (e.g. clip[:, t] of a
    [N, T, H, W, C] tensor).  Reads only shapes, strides and pointers: no views are made."""
    import torch
    h, w, c = plan.height[0], plan.width[0], pixel_channels(px)
    lead = () if n is None else (n,)
    b = len(lead)
    if not isinstance(out, torch.Tensor):
        raise ValueError("out: packed pixels take one tensor")
    st = out.stride()
    if out.shape == lead + (h, w, c):
        sy, sx, sc = st[b:]
    elif b and out.shape == lead + (c, h, w):
        sc, sy, sx = st[b:]
    else:
        raise ValueError("out: shape %s, the plan gives %s%s" % (tuple(out.shape), lead + (h, w, c), " or %s channels-last" % (lead + (c, h, w),) if b else ""))
    _check_tensor(out, desc, device, dtype)
    if sc != 1 or sx != c or sy < w * c or (b and st[0] < sy * (h - 1) + w * c):
        raise ValueError("out: the pixels must be dense within a row, rows and batch entries apart (stride %s)" % (st,))
    es = out.element_size()
    return out.data_ptr(), sy * es, st[0] * es if b else None


class Stages(collections.namedtuple("Stages", "scale tensor windows pixel lut chroma warp format yuvpack", defaults=(None,) * 9)):
    """the stages of one picture export, None where the call has none: scale an abi.ExportScale; tensor an abi.ExportTensor (float
    elements); windows one abi.ExportWindow per picture; pixel an abi.ExportPixel (packed pixels: one destination); lut a colour LUT
    of the context or decoder, or its raw handle; chroma an abi.ExportChroma; warp (abi.ExportWarp, abi.WarpMap array) of
    abi.warp_stage; format an abi.ExportFormat (the YUV layouts at another chroma format); yuvpack an abi.ExportYuvPack (YUV interleaved
    into words: one destination, with the format stage of the words' chroma format).  libhm_amd.export_stages_plan,
    Context.export_stages_into and hmdec's dispatcher choose the entry from it."""
    __slots__ = ()

    def shape_only(self):
        """without the colour and chroma stages, which change no plan: their rules are the export's own to report"""
        return self if self.lut is None and self.chroma is None else self._replace(lut=None, chroma=None)


def stage_extents(plan, pitches):
    """the batch strides of one picture exported as a batch of one: every plane's extent"""
    return [pitches[k] * (plan.height[k] - 1) + plan.row_bytes[k] for k in range(plan.planes)]


def export_tensors(call, seq, device, layout, bit_depth, crop, matrix, full_range, msb_aligned=False, on_stream=True, size=None,
                   filter="bilinear", out=None, n=None, dtype=None, mean=None, std=None, scale=None, bias=None, windows=None,
                   pixel=None, alpha=None, memory_format=None, lut=None, chroma=None, warp=None, format=None):
    """allocate with torch on `device` (or take `out`) and run `call(desc, stages, ptrs, pitches, bstrides, stream)` on torch's
    current stream.  stages (Stages): scale None (size None), else the abi.ExportScale of size (height, width) and filter; tensor
    None (dtype None), else the abi.ExportTensor of the float dtype and mean / std (or explicit scale / bias triples); windows None,
    or the abi.ExportWindow of every picture (make_windows: `crop` is already part of them, so the descriptor's own crop is 0);
    pixel from pixel / alpha / memory_format (make_pixel): packed pixels, ONE tensor [H, W, C] ([N, H, W, C]; channels-last
    [N, 3, H, W]), the lists of its call one long, bstrides of one picture the extent of its rows; lut and chroma as given; warp
    None, or (abi.ExportWarp, abi.WarpMap array) of abi.warp_stage: size and filter belong to it and the stages have no scale.
    format None, or the abi.ExportFormat of a format export (abi.format_stage): the planes of its chroma format; the planar layout at
    4:4:4 is ONE tensor [3, H, W] ([N, 3, H, W]) with Y, Cb and Cr as its channels.
    bstrides of planes: None for one picture (n None), else the bytes between the batch entries of every plane of the n pictures."""
    import torch
    from . import export_stages_plan
    if warp is not None:
        if layout_code(layout) != abi.EXPORT_RGB:
            raise ValueError("warp needs layout=\"rgb\"")
        size = None
    px = make_pixel(pixel, alpha, memory_format, layout, dtype, n)
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    fo = None if format is None else format.chroma_format
    desc = make_desc(layout, bit_depth, crop if windows is None else (0, 0, 0, 0), matrix, full_range, msb_aligned,
                     seq if dtype is not None else None, fo)
    stages = Stages(make_scale(size, filter), make_tensor(dtype, plane_depths(seq, desc.layout, bd, fo), mean, std, scale, bias), windows, px,
                    lut, chroma, warp, format)
    stacked = fo == 3 and desc.layout == abi.EXPORT_PLANAR
    plan = export_stages_plan(seq, desc, stages.shape_only(), n or 1)
    with torch.cuda.device(device):
        if px is not None:
            if out is None:
                out = alloc_pixels(plan, desc, px, device, n, dtype, memory_format is not None)
            ptr, pitch, bstride = out_pixels(out, plan, desc, px, device, n, dtype)
            ptrs, pitches, bstrides = [ptr], [pitch], [bstride] if bstride is not None else stage_extents(plan, [pitch])
        else:
            if out is None:
                out = alloc_outputs(plan, desc, device, n, dtype, stacked)
            ptrs, pitches, bstrides = out_spans(out, plan, desc, device, n, dtype, stacked)
        call(desc, stages, ptrs, pitches, bstrides, torch.cuda.current_stream(device).cuda_stream if on_stream else 0)
    return out


# ------------------------------------------------------------------------------------------------ packed YUV (include/hmgpu.h "packed YUV")
def yuvpack_shape(code, plan, row_align=1):
    """(shape, torch dtype, pitch in bytes) of one picture's tensor of words: [H, W, 2] / [H, W, 4] elements of 1 or 2 bytes, [H, W]
    int32 (Y410), [H, P / 4] int32 (V210) with P = row_bytes rounded up to row_align (a multiple of 4)"""
    import torch
    h, w, rb = plan.height[0], plan.width[0], plan.row_bytes[0]
    es = abi.YUVPACK_ELEMENT[code]
    dt = torch.int32 if es == 4 else torch_dtype(es)
    if code == abi.YUVPACK_V210:
        row_align = int(row_align)
        if row_align < 1 or row_align % 4:
            if row_align != 1:
                raise ValueError("row_align: 1 or a multiple of 4 bytes")
            row_align = 4
        p = (rb + row_align - 1) // row_align * row_align
        return (h, p // 4), dt, p
    if row_align != 1:
        raise ValueError("row_align belongs to yuv=\"v210\"")
    if code == abi.YUVPACK_Y410:
        return (h, w), dt, rb
    return (h, w, rb // (w * es)), dt, rb


def yuvpack_span(t, code, plan, device, n=None, row_align=1):
    """a caller's tensor of words as (pointer, pitch in bytes, batch stride in bytes or None): the shape and dtype of yuvpack_shape
    (16-bit: int16 as well), the words of a row dense, rows and batch entries any stride apart"""
    import torch
    shape, dt, _ = yuvpack_shape(code, plan, row_align)
    lead = () if n is None else (n,)
    b = len(lead)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != lead + shape:
        raise ValueError("a %s tensor of shape %s" % (dt, lead + shape))
    if t.dtype != dt and not (t.element_size() == 2 and t.dtype == torch.int16 and abi.YUVPACK_ELEMENT[code] == 2):
        raise ValueError("dtype %s, the words are %s" % (t.dtype, dt))
    if t.get_device() != device:
        raise ValueError("on device %d, the context is on %d" % (t.get_device(), device))
    st, es = t.stride(), t.element_size()
    inner = (1,) if len(shape) == 2 else (shape[2], 1)
    row = shape[1] * inner[0]
    if tuple(st[b + 1:]) != inner or (shape[0] > 1 and st[b] < row) or (b and n > 1 and st[0] < st[b] * (shape[0] - 1) + row):
        raise ValueError("the words of a row must be dense, rows and batch entries apart (stride %s)" % (st,))
    return t.data_ptr(), st[b] * es, st[0] * es if b else None


def yuvpack_only(**others):
    """yuv= of the Python exports goes with crop, windows, flip, alpha, chroma, chroma_down, chroma_loc, out, row_align and on_stream:
    any other keyword that was given (not None / False) is refused"""
    given = sorted(k for k, v in others.items() if v is not None and v is not False)
    if given:
        raise ValueError("yuv= does not go with %s" % ", ".join(given))


def yuvpack_stages(yuv, alpha, windows, chroma, chroma_down, chroma_loc):
    """(code, Stages) of yuv= / alpha= and the conversion keywords"""
    code = abi.yuvpack_code(yuv)
    fmt = abi.format_stage(abi.YUVPACK_CHROMA[code], chroma, chroma_down, chroma_loc)
    return code, Stages(windows=windows, format=fmt, yuvpack=abi.make_export_yuvpack(code, 0 if alpha is None else alpha))


def export_yuvpack(call, seq, device, yuv, alpha, crop, windows, chroma, chroma_down, chroma_loc, on_stream=True, out=None, n=None, row_align=1):
    """export_tensors for YUV interleaved into words: allocate the one tensor (or take `out`) and run `call`; windows: None, or the
    abi.ExportWindow of every picture (`crop` already part of them)"""
    import torch
    from . import export_stages_plan
    code, stages = yuvpack_stages(yuv, alpha, windows, chroma, chroma_down, chroma_loc)
    d = abi.YUVPACK_DEPTH[code]
    desc = abi.make_export_desc(abi.EXPORT_PLANAR, (d, d), 1 if d <= 8 else 2, False, tuple(crop) if windows is None else (0, 0, 0, 0), 1, 0)
    plan = export_stages_plan(seq, desc, stages, n or 1)
    with torch.cuda.device(device):
        if out is None:
            shape, dt, _ = yuvpack_shape(code, plan, row_align)
            out = torch.empty((() if n is None else (n,)) + shape, dtype=dt, device=torch.device("cuda", device))
        ptr, pitch, bstride = yuvpack_span(out, code, plan, device, n, row_align)
        call(desc, stages, [ptr], [pitch], [bstride] if bstride is not None else stage_extents(plan, [pitch]),
             torch.cuda.current_stream(device).cuda_stream if on_stream else 0)
    return out


# ------------------------------------------------------------------------------------------------ colour LUTs (host side: data for the device)
# The colour stage of the RGB exports (include/hmgpu.h "colour export") takes any table; what follows builds tables on the host in
# float64 -- from a .cube file, or from H.273 colour descriptions -- and rounds them once to the code values of the output depth.
def _round_codes(x, depth):
    """x in [0, 1] (clipped) to code values of `depth` bits, half away from zero"""
    m = float((1 << depth) - 1)
    return np.floor(np.clip(np.asarray(x, np.float64), 0.0, 1.0) * m + 0.5).astype(np.uint16)


def load_cube(path, depth=8):
    """(lattice, shaper) of a .cube text file for Context.colour_lut(lattice, shaper, depth): LUT_3D_SIZE L gives lattice
    [L, L, L, 3] indexed (b, g, r) -- the file's order, R fastest -- of code values of `depth` bits, rounded half away from zero; an
    optional LUT_1D_SIZE table (its rows before the 3D ones) is resampled to 2^depth entries per channel by linear interpolation in
    float64 and gives the shaper: positions 0 .. 65535 in front of a lattice, code values on its own (then lattice is None).
    DOMAIN_MIN / DOMAIN_MAX other than 0 / 1, a size outside 2 .. 65 or a wrong number of rows raise ValueError."""
    n1 = n3 = 0
    rows = []
    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            key = line.split()[0].upper()
            if key == "TITLE":
                continue
            if key == "LUT_1D_SIZE":
                n1 = int(line.split()[1])
            elif key == "LUT_3D_SIZE":
                n3 = int(line.split()[1])
            elif key in ("DOMAIN_MIN", "DOMAIN_MAX"):
                want = 0.0 if key == "DOMAIN_MIN" else 1.0
                if [float(v) for v in line.split()[1:]] != [want] * 3:
                    raise ValueError("%s: %s other than %g %g %g is not supported" % (path, key, want, want, want))
            elif key[0].isalpha():
                raise ValueError("%s: unknown keyword %s" % (path, key))
            else:
                vals = [float(v) for v in line.split()]
                if len(vals) != 3:
                    raise ValueError("%s: a table row holds three numbers: %r" % (path, line))
                rows.append(vals)
    if not n1 and not n3:
        raise ValueError("%s: neither LUT_1D_SIZE nor LUT_3D_SIZE" % path)
    if (n3 and not 2 <= n3 <= 65) or (n1 and n1 < 2):
        raise ValueError("%s: LUT_3D_SIZE 2 .. 65, LUT_1D_SIZE 2 or more" % path)
    if len(rows) != n1 + n3 ** 3:
        raise ValueError("%s: %d table rows, the sizes ask for %d" % (path, len(rows), n1 + n3 ** 3))
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    lattice = shaper = None
    if n1:
        x = np.arange(1 << depth, dtype=np.float64) / float((1 << depth) - 1)
        curve = np.stack([np.interp(x, np.linspace(0.0, 1.0, n1), rows[:n1, c]) for c in range(3)])
        shaper = _round_codes(curve, 16 if n3 else depth)
    if n3:
        lattice = _round_codes(rows[n1:], depth).reshape(n3, n3, n3, 3)
    return lattice, shaper


# H.273 colour_primaries: the chromaticities (x, y) of R, G, B; the white point of all three is D65
PRIMARIES = {1: ((0.640, 0.330), (0.300, 0.600), (0.150, 0.060)),       # BT.709
             9: ((0.708, 0.292), (0.170, 0.797), (0.131, 0.046)),       # BT.2020
             12: ((0.680, 0.320), (0.265, 0.690), (0.150, 0.060))}      # P3-D65
D65 = (0.3127, 0.3290)
SDR_GAMMA = (1, 6, 14, 15)            # transfer_characteristics shown with the BT.1886 display gamma 2.4
PQ, HLG, SRGB, LINEAR = 16, 18, 13, 8
HLG_LW, HLG_GAMMA = 1000.0, 1.2
_PQ_M1, _PQ_M2, _PQ_C1, _PQ_C2, _PQ_C3 = 2610.0 / 16384, 2523.0 / 4096 * 128, 3424.0 / 4096, 2413.0 / 4096 * 32, 2392.0 / 4096 * 32
_HLG_A = 0.17883277
_HLG_B, _HLG_C = 1.0 - 4.0 * _HLG_A, 0.5 - _HLG_A * np.log(4.0 * _HLG_A)


def rgb_to_xyz(primaries):
    """the 3x3 matrix from linear RGB of an H.273 colour_primaries code to XYZ, white D65 at Y = 1"""
    if primaries not in PRIMARIES:
        raise ValueError("colour_primaries %r: one of %s" % (primaries, sorted(PRIMARIES)))
    xyz = np.array([[x / y, 1.0, (1.0 - x - y) / y] for x, y in PRIMARIES[primaries]], np.float64).T
    white = np.array([D65[0] / D65[1], 1.0, (1.0 - D65[0] - D65[1]) / D65[1]], np.float64)
    return xyz * np.linalg.solve(xyz, white)[None, :]


def primaries_matrix(src, dst):
    """linear RGB of primaries `src` to linear RGB of `dst` through XYZ"""
    return np.linalg.solve(rgb_to_xyz(dst), rgb_to_xyz(src))


def pq_eotf(e):
    """ST 2084: the non-linear value 0 .. 1 to cd/m2 (absolute, 10000 at 1)"""
    p = np.power(np.clip(np.asarray(e, np.float64), 0.0, 1.0), 1.0 / _PQ_M2)
    return 10000.0 * np.power(np.maximum(p - _PQ_C1, 0.0) / (_PQ_C2 - _PQ_C3 * p), 1.0 / _PQ_M1)


def pq_inverse_eotf(l):
    y = np.power(np.clip(np.asarray(l, np.float64), 0.0, 10000.0) / 10000.0, _PQ_M1)
    return np.power((_PQ_C1 + _PQ_C2 * y) / (1.0 + _PQ_C3 * y), _PQ_M2)


def hlg_inverse_oetf(e):
    """BT.2100 HLG: the non-linear value 0 .. 1 to scene light 0 .. 1 (0.5 -> 1/12)"""
    e = np.clip(np.asarray(e, np.float64), 0.0, 1.0)
    return np.where(e <= 0.5, e * e / 3.0, (np.exp((np.maximum(e, 0.5) - _HLG_C) / _HLG_A) + _HLG_B) / 12.0)


def hlg_oetf(s):
    s = np.clip(np.asarray(s, np.float64), 0.0, 1.0)
    return np.where(s <= 1.0 / 12.0, np.sqrt(3.0 * s), _HLG_A * np.log(np.maximum(12.0 * s - _HLG_B, 1e-300)) + _HLG_C)


def to_display_light(rgb, primaries, transfer, white):
    """non-linear R'G'B' [..., 3] in 0 .. 1 of an H.273 transfer_characteristics code to display light in cd/m2"""
    rgb = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    if transfer in SDR_GAMMA:
        return white * np.power(rgb, 2.4)
    if transfer == SRGB:
        return white * np.where(rgb <= 0.04045, rgb / 12.92, np.power((rgb + 0.055) / 1.055, 2.4))
    if transfer == LINEAR:
        return white * rgb
    if transfer == PQ:
        return pq_eotf(rgb)
    if transfer == HLG:                                               # inverse OETF, then the OOTF on the scene luminance
        scene = hlg_inverse_oetf(rgb)
        ys = scene @ rgb_to_xyz(primaries)[1]
        return HLG_LW * np.power(np.maximum(ys, 1e-300), HLG_GAMMA - 1.0)[..., None] * scene
    raise ValueError("transfer_characteristics %r: one of 1, 6, 14, 15, 13, 8, 16, 18" % (transfer,))


def from_display_light(light, primaries, transfer, white):
    """the inverse of to_display_light, the result clipped to 0 .. 1"""
    light = np.maximum(np.asarray(light, np.float64), 0.0)
    if transfer in SDR_GAMMA:
        return np.power(np.clip(light / white, 0.0, 1.0), 1.0 / 2.4)
    if transfer == SRGB:
        v = np.clip(light / white, 0.0, 1.0)
        return np.where(v <= 0.0031308, v * 12.92, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    if transfer == LINEAR:
        return np.clip(light / white, 0.0, 1.0)
    if transfer == PQ:
        return pq_inverse_eotf(light)
    if transfer == HLG:
        d = light / HLG_LW
        yd = d @ rgb_to_xyz(primaries)[1]
        return hlg_oetf(np.power(np.maximum(yd, 1e-300), (1.0 - HLG_GAMMA) / HLG_GAMMA)[..., None] * d)
    raise ValueError("transfer_characteristics %r: one of 1, 6, 14, 15, 13, 8, 16, 18" % (transfer,))


def transfer_peak(transfer, white):
    """the luminance in cd/m2 of code value 1.0"""
    return 10000.0 if transfer == PQ else HLG_LW if transfer == HLG else float(white)


def bt2390_eetf(y, src_peak, dst_peak):
    """BT.2390's EETF on luminances y in cd/m2 (black at 0): the knee and Hermite roll-off in the PQ domain"""
    lw, mx = pq_inverse_eotf(src_peak), pq_inverse_eotf(dst_peak)
    if mx >= lw:
        return np.asarray(y, np.float64)
    e1 = pq_inverse_eotf(y) / lw
    max_lum = mx / lw
    ks = 1.5 * max_lum - 0.5
    t = np.clip((e1 - ks) / (1.0 - ks), 0.0, 1.0)
    p = (2 * t ** 3 - 3 * t ** 2 + 1) * ks + (t ** 3 - 2 * t ** 2 + t) * (1.0 - ks) + (-2 * t ** 3 + 3 * t ** 2) * max_lum
    return pq_eotf(np.where(e1 < ks, e1, p) * lw)


def colour_lut(src, dst, depth, size=33, white=203.0, peak=None, tone="clip"):
    """(lattice, shaper) for Context.colour_lut that takes non-linear R'G'B' of src = (colour_primaries, transfer_characteristics) to
    dst = (...), H.273 codes: primaries 1 (BT.709), 9 (BT.2020), 12 (P3-D65); transfers 1 / 6 / 14 / 15 (BT.1886 display gamma
    2.4, code 1.0 = `white` cd/m2), 13 (sRGB), 8 (linear), 16 (ST 2084, absolute), 18 (HLG: inverse OETF, then the BT.2100 OOTF with
    Lw = 1000 and gamma 1.2).  Node n of an axis stands for the value n / (size - 1); per node, in float64: display light in cd/m2,
    the gamut matrix through XYZ (D65), the tone rule, the destination's inverse curve, a clip to 0 .. 1, and code values of
    `depth` bits rounded half away from zero.  tone "clip": nothing before that clip; "bt2390": BT.2390's EETF from `peak` (None:
    the source's own, 10000 / 1000 / white) to the destination's peak on the luminance in destination primaries, R, G and B scaled
    by the ratio.  src == dst with tone "clip" is the identity lattice.  No shaper is built (None)."""
    if tone not in ("clip", "bt2390"):
        raise ValueError("tone %r: \"clip\" or \"bt2390\"" % (tone,))
    if not 2 <= size <= 65 or not 8 <= depth <= 16:
        raise ValueError("size 2 .. 65, depth 8 .. 16")
    (sp, st), (dp, dt) = (int(v) for v in src), (int(v) for v in dst)
    m_to, m_gamut = rgb_to_xyz(dp), primaries_matrix(sp, dp)          # (raises on unknown primaries)
    axis = np.arange(size, dtype=np.float64) / float(size - 1)
    b, g, r = np.meshgrid(axis, axis, axis, indexing="ij")
    rgb = np.stack([r, g, b], axis=-1)
    if (sp, st) == (dp, dt) and tone == "clip":
        return _round_codes(rgb, depth), None
    light = to_display_light(rgb, sp, st, white) @ m_gamut.T
    if tone == "bt2390":
        y = np.maximum(light @ m_to[1], 0.0)
        mapped = bt2390_eetf(y, float(peak) if peak is not None else transfer_peak(st, white), transfer_peak(dt, white))
        light = light * np.where(y > 0.0, mapped / np.maximum(y, 1e-300), 1.0)[..., None]
    return _round_codes(from_display_light(light, dp, dt, white), depth), None


def vui_source(primaries, transfer):
    """(colour_primaries, transfer_characteristics) of a picture's VUI as colour_lut's src; unspecified or unknown codes raise"""
    if primaries not in PRIMARIES or transfer not in SDR_GAMMA + (PQ, HLG, SRGB, LINEAR):
        raise ValueError("the stream's colour description (primaries %r, transfer %r) names no source for a colour LUT: give src=" % (primaries, transfer))
    return int(primaries), int(transfer)
