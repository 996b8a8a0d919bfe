"""Device export to torch tensors: layout names, output dtypes and the colour policy shared by Context.export and
hmdec.Picture.export.  No compute here: the conversion is k_export.hip behind hmgpu_picture_export.

Colour policy (the one place it is decided): an RGB export takes `matrix` / `full_range` from the caller; where the caller leaves
them None they come from the picture's VUI (matrix_coefficients, video_full_range_flag).  A stream without a colour description
(matrix 2, "unspecified") is treated as BT.709 (matrix 1); without video_signal_type it is limited range (E.3.1's default).  Codes
the kernel does not implement (anything but 0, 1, 5, 6, 9) are refused with HMGPU_EUNSUPPORTED rather than guessed.
"""
from . import abi

LAYOUTS = {"planar": abi.EXPORT_PLANAR, "yuv": abi.EXPORT_PLANAR, "semiplanar": abi.EXPORT_SEMIPLANAR, "nv12": abi.EXPORT_SEMIPLANAR,
           "rgb": abi.EXPORT_RGB}
UNSPECIFIED = 2
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


def make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned=False):
    """bit_depth: an int for every channel type, a (luma, chroma) pair, or None / 0 for the coding bit depths"""
    bd = (0, 0) if bit_depth is None else (bit_depth, bit_depth) if isinstance(bit_depth, int) else tuple(bit_depth)
    nbytes = 2 if msb_aligned or max(bd) > 8 or min(bd) == 0 else 1
    return abi.make_export_desc(layout_code(layout), bd, nbytes, msb_aligned, tuple(crop), matrix, full_range)


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


def plane_shapes(plan, desc):
    """the shape of every plane tensor: [H, W], or [H, W, 2] for the CbCr plane of the semi-planar layout"""
    return [(plan.height[k], plan.width[k], 2) if desc.layout == abi.EXPORT_SEMIPLANAR and k == 1 else (plan.height[k], plan.width[k])
            for k in range(plan.planes)]


def _check_tensor(t, desc, device):
    import torch
    if t.dtype != torch_dtype(desc.bytes_per_sample) and not (desc.bytes_per_sample == 2 and t.dtype == torch.int16):
        raise ValueError("out: dtype %s, the plan gives %s" % (t.dtype, torch_dtype(desc.bytes_per_sample)))
    if t.get_device() != device:
        raise ValueError("out: on device %d, the picture is on %d" % (t.get_device(), device))


def out_spans(out, plan, desc, device):
    """a caller's destination (RGB: one [3, H, W] tensor or three planes; YUV: a tuple of planes) as (pointers, pitches in bytes)
    per plane.  Each plane has the planned shape and dtype on the device and its samples dense within a row; rows may be any stride
    apart (e.g. a view batch[i]).  Reads only shapes, strides and pointers: no views are made."""
    import torch
    shapes = plane_shapes(plan, desc)
    if isinstance(out, torch.Tensor):
        if desc.layout != abi.EXPORT_RGB:
            raise ValueError("out: the planar / semi-planar layouts take a tuple of planes")
        h, w = shapes[0]
        if out.shape != (3, h, w):
            raise ValueError("out: shape %s, the plan gives %s" % (tuple(out.shape), (3, h, w)))
        _check_tensor(out, desc, device)
        s0, s1, s2 = out.stride()
        if s2 != 1 or s1 < w or s0 < s1 * (h - 1) + w:
            raise ValueError("out: the planes' samples must be dense within a row, rows and planes apart (stride %s)" % ((s0, s1, s2),))
        es, base = out.element_size(), out.data_ptr()
        return [base + k * s0 * es for k in range(3)], [s1 * es] * 3
    planes = tuple(out)
    if len(planes) != len(shapes):
        raise ValueError("out: %d planes, the plan gives %d" % (len(planes), len(shapes)))
    ptrs, pitches = [], []
    for p, shape in zip(planes, shapes):
        if not isinstance(p, torch.Tensor) or p.shape != shape:
            raise ValueError("out: a plane is not a tensor of shape %s" % (shape,))
        _check_tensor(p, desc, device)
        st = p.stride()
        inner = (1,) if len(shape) == 2 else (2, 1)
        if st[1:] != inner or st[0] < shape[1] * inner[0]:
            raise ValueError("out: a plane's samples must be dense within a row (stride %s)" % (st,))
        ptrs.append(p.data_ptr())
        pitches.append(st[0] * p.element_size())
    return ptrs, pitches


def alloc_outputs(plan, desc, device):
    """torch tensors for what `plan` describes: RGB [3, H, W]; planar (Y, Cb, Cr) 2-D; semi-planar (Y [H, W], CbCr [Hc, Wc, 2]).
    Returns (result, per-plane tensors)."""
    import torch
    dt = torch_dtype(desc.bytes_per_sample)
    dev = torch.device("cuda", device)
    if desc.layout == abi.EXPORT_RGB:
        t = torch.empty((3, plan.height[0], plan.width[0]), dtype=dt, device=dev)
        return t, [t[0], t[1], t[2]]
    planes = []
    for k in range(plan.planes):
        if desc.layout == abi.EXPORT_SEMIPLANAR and k == 1:
            planes.append(torch.empty((plan.height[1], plan.width[1], 2), dtype=dt, device=dev))
        else:
            planes.append(torch.empty((plan.height[k], plan.width[k]), dtype=dt, device=dev))
    return tuple(planes), planes


def export_tensors(call, seq, device, layout, bit_depth, crop, matrix, full_range, msb_aligned=False, on_stream=True, size=None,
                   filter="bilinear", out=None):
    """allocate with torch on `device` (or take `out`) and run `call(desc, scale, ptrs, pitches, stream)` on torch's current stream;
    scale: None (size None), else the abi.ExportScale of size (height, width) and filter"""
    import torch
    from . import export_plan, export_scaled_plan
    desc = make_desc(layout, bit_depth, crop, matrix, full_range, msb_aligned)
    scale = make_scale(size, filter)
    plan = export_plan(seq, desc) if scale is None else export_scaled_plan(seq, desc, scale)
    with torch.cuda.device(device):
        if out is None:
            out, planes = alloc_outputs(plan, desc, device)
            ptrs = [p.data_ptr() for p in planes]
            pitches = [p.stride(0) * p.element_size() for p in planes]
        else:
            ptrs, pitches = out_spans(out, plan, desc, device)
        stream = torch.cuda.current_stream(device).cuda_stream if on_stream else 0
        call(desc, scale, ptrs, pitches, stream)
    return out
