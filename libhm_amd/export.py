"""Device export to torch tensors: layout names, output dtypes and the colour policy shared by Context.export and
hmdec.Picture.export.  No compute here: the conversion is k_export.hip behind hmgpu_picture_export.

Colour policy (the one place it is decided): an RGB export takes `matrix` / `full_range` from the caller; where the caller leaves
them None they come from the picture's VUI (matrix_coefficients, video_full_range_flag).  A stream without a colour description
(matrix 2, "unspecified") is treated as BT.709 (matrix 1); without video_signal_type it is limited range (E.3.1's default).  Codes
the kernel does not implement (anything but 0, 1, 5, 6, 9) are refused with HMGPU_EUNSUPPORTED rather than guessed.

Tensor output (export_batch, dtype=): float16 / bfloat16 / float32 elements take fl(fl(v * scale_k) + bias_k) of the integer v the
export writes, with (scale, bias) from `affine`: v / (2^D - 1) normalised by a per-plane mean and std.
"""
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


def make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned=False, seq=None):
    """bit_depth: an int for every channel type, a (luma, chroma) pair, or None / 0 for the coding bit depths.  seq (float output):
    the container is the one the output depths need (1 byte when none exceeds 8), the coding depths taken from the sequence"""
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    if seq is not None:
        nbytes = 2 if max(plane_depths(seq, layout_code(layout), bd)) > 8 else 1
    else:
        nbytes = 2 if msb_aligned or max(bd) > 8 or min(bd) == 0 else 1
    return abi.make_export_desc(layout_code(layout), bd, nbytes, msb_aligned, tuple(crop), matrix, full_range)


def plane_depths(seq, layout, bd):
    """the integer depth D of every output plane: RGB the luma output depth three times; YUV luma, chroma, chroma (4:0:0: luma)"""
    y = bd[0] or seq.bit_depth_luma
    if layout == abi.EXPORT_RGB:
        return (y, y, y)
    if seq.chroma_format == 0:
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


def out_spans(out, plan, desc, device, n=None, dtype=None):
    """a caller's destination as (pointers, pitches in bytes, batch strides in bytes or None) per plane.  n None, one picture: RGB
    one [3, H, W] tensor or three planes, YUV a tuple of planes.  n pictures: the same with a leading dimension of n ([n, 3, H, W];
    planes [n, H, W], [n, Hc, Wc, 2]).  Each plane has the planned shape and dtype on the device and its samples dense within a
    row; rows, planes and batch entries may be any stride apart (e.g. a view batch[i]).  Reads only shapes, strides and pointers:
    no views are made."""
    import torch
    shapes = plane_shapes(plan, desc)
    lead = () if n is None else (n,)
    b = len(lead)
    if isinstance(out, torch.Tensor):
        if desc.layout != abi.EXPORT_RGB:
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


def alloc_outputs(plan, desc, device, n=None, dtype=None):
    """torch tensors for what `plan` describes: RGB [3, H, W]; planar (Y, Cb, Cr) 2-D; semi-planar (Y [H, W], CbCr [Hc, Wc, 2]);
    with n, each with a leading dimension of n.  dtype None: the unsigned type of the container."""
    import torch
    dt = torch_dtype(desc.bytes_per_sample) if dtype is None else dtype
    dev = torch.device("cuda", device)
    lead = () if n is None else (n,)
    if desc.layout == abi.EXPORT_RGB:
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


def export_tensors(call, seq, device, layout, bit_depth, crop, matrix, full_range, msb_aligned=False, on_stream=True, size=None,
                   filter="bilinear", out=None, n=None, dtype=None, mean=None, std=None, scale=None, bias=None, windows=None,
                   pixel=None, alpha=None, memory_format=None, pixel_call=None):
    """allocate with torch on `device` (or take `out`) and run `call(desc, scale, tensor, ptrs, pitches, bstrides, stream)` on torch's
    current stream.  scale: None (size None), else the abi.ExportScale of size (height, width) and filter; tensor: None (dtype None),
    else the abi.ExportTensor of the float dtype and mean / std (or explicit scale / bias triples); bstrides: None for one picture
    (n None), else the bytes between the batch entries of every plane of the n pictures.  windows: None, or the abi.ExportWindow of
    every picture (make_windows: `crop` is already part of them, so the descriptor's own crop is 0).
    pixel / alpha / memory_format (make_pixel): packed pixels, ONE tensor [H, W, C] ([N, H, W, C]; channels-last [N, 3, H, W]) through
    `pixel_call(desc, scale, tensor, pixel, ptr, pitch, bstride, stream)`; bstride of one picture: the extent of its rows."""
    import torch
    from . import export_pixels_plan, export_tensor_plan, export_windows_plan
    px = make_pixel(pixel, alpha, memory_format, layout, dtype, n)
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    desc = make_desc(layout, bit_depth, crop if windows is None else (0, 0, 0, 0), matrix, full_range, msb_aligned,
                     seq if dtype is not None else None)
    sc = make_scale(size, filter)
    tensor = make_tensor(dtype, plane_depths(seq, desc.layout, bd), mean, std, scale, bias)
    if px is not None:
        plan = export_pixels_plan(seq, desc, sc, tensor, windows, px)
        with torch.cuda.device(device):
            if out is None:
                out = alloc_pixels(plan, desc, px, device, n, dtype, memory_format is not None)
            ptr, pitch, bstride = out_pixels(out, plan, desc, px, device, n, dtype)
            if bstride is None:
                bstride = pitch * (plan.height[0] - 1) + plan.row_bytes[0]
            stream = torch.cuda.current_stream(device).cuda_stream if on_stream else 0
            pixel_call(desc, sc, tensor, px, ptr, pitch, bstride, stream)
        return out
    plan = export_tensor_plan(seq, desc, sc, tensor) if windows is None else export_windows_plan(seq, desc, sc, tensor, windows)
    with torch.cuda.device(device):
        if out is None:
            out = alloc_outputs(plan, desc, device, n, dtype)
        ptrs, pitches, bstrides = out_spans(out, plan, desc, device, n, dtype)
        stream = torch.cuda.current_stream(device).cuda_stream if on_stream else 0
        call(desc, sc, tensor, ptrs, pitches, bstrides, stream)
    return out
