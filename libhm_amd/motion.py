"""Motion and block export to torch tensors (hmgpu_pictures_export_motion, k_motion.hip): the argument handling shared by
Context.export_motion, hmdec.export_motion_batch and hmdec.Picture.motion.  No compute here.

form "blocks": the grid of 4x4 luma blocks -- {"mv": int16 [N, L, 2, H4, W4] (hor, ver in quarter luma samples), "ref_poc": int32
[N, L, H4, W4] (abi.MOTION_NO_REF where a list is unused), "block": int8 [N, 4, H4, W4] (mode -1 / 0 inter / 1 intra, log2 CU size,
part_size, QP)}.  form "dense": one value per output sample of export_batch(windows=, flip=, size=, filter="nearest") -- {"flow0" /
"flow1": float [N, 2, H, W] (dx, dy in output samples), "ref_poc": int32 [N, L, H, W], "block": int8 [N, 4, H, W]}.  L counts the
lists selected by `lists`, in list order.
"""
import ctypes as C

from . import abi
from . import export

FORMS = {"blocks": abi.MOTION_BLOCKS, "dense": abi.MOTION_DENSE}


def lists_mask(lists):
    """(0, 1) -> 3; an int is taken as the mask"""
    if isinstance(lists, int):
        return lists
    mask = 0
    for l in lists:
        if l not in (0, 1):
            raise ValueError("lists: 0 and / or 1")
        mask |= 1 << l
    return mask


def form_code(form):
    try:
        return form if isinstance(form, int) else FORMS[form.lower()]
    except KeyError:
        raise ValueError("unknown motion form %r (blocks or dense)" % (form,))


def plan_for(seq, desc, scale=None, windows=None, n=None):
    """what an export with `desc` writes (hmgpu_motion_plan_for: host code, no GPU); windows: abi.ExportWindow per picture (dense)"""
    from . import HmgpuError, lib
    plan = abi.MotionPlan()
    windows = None if windows is None else list(windows)
    w = None if windows is None else (abi.ExportWindow * max(len(windows), 1))(*windows)
    count = n if n is not None else (len(windows) if windows is not None else 1)
    st = lib().hmgpu_motion_plan_for(C.byref(seq), C.byref(desc), C.byref(scale) if scale is not None else None, count, w, C.byref(plan))
    if st != abi.HMGPU_OK:
        raise HmgpuError(st, "hmgpu_motion_plan_for")
    return plan


def tensor_names(form, mask):
    """destination slot (abi.MOTION_DST_*) -> key of the result dict"""
    if form == abi.MOTION_BLOCKS:
        return {abi.MOTION_DST_MV0: "mv", abi.MOTION_DST_REF: "ref_poc", abi.MOTION_DST_BLOCK: "block"}
    names = {abi.MOTION_DST_REF: "ref_poc", abi.MOTION_DST_BLOCK: "block"}
    for l in range(2):
        if (mask >> l) & 1:
            names[l] = "flow%d" % l
    return names


def _shape(form, plan, k, n):
    h, w = plan.height[k], plan.width[k]
    if form == abi.MOTION_BLOCKS and k == abi.MOTION_DST_MV0:
        return (n, plan.lists, 2, h, w)
    return (n, plan.channels[k], h, w)


def export_motion(call, seq, device, n, form="blocks", lists=(0, 1), size=None, windows=None, flip=None, dtype=None, out=None,
                  crop=(0, 0, 0, 0), enqueue=True):
    """allocate with torch on `device` (or take the tensors of the dict `out`: only its keys are written) and run
    call(desc, scale, windows, ptrs[4], pitches[4], plane_strides[4], batch_strides[4], stream) on torch's current stream.
    blocks: crop (left, right, top, bottom) in multiples of 4 luma samples.  dense: windows (x, y, w, h) per picture relative to crop,
    flip per picture, size (height, width) or None (windows of one size); dtype torch.float16 / bfloat16 / float32 (None: float32)."""
    import torch
    form = form_code(form)
    mask = lists_mask(lists)
    if form == abi.MOTION_BLOCKS:
        if size is not None or windows is not None or flip is not None or dtype is not None:
            raise ValueError("export_motion(form='blocks') takes crop only: size / windows / flip / dtype belong to form='dense'")
        desc = abi.make_motion_desc(form, mask, abi.SAMPLE_UINT, crop)
        sc, win = None, None
        dtypes = {abi.MOTION_DST_MV0: torch.int16}
    else:
        dtype = torch.float32 if dtype is None else dtype
        desc = abi.make_motion_desc(form, mask, export.sample_type(dtype))
        sc = export.make_scale(size, "nearest")
        l, r, t, b = (int(v) for v in crop)
        win = export.make_windows(seq, crop, windows if windows is not None else [(0, 0, seq.width - l - r, seq.height - t - b)] * n, flip, n)
        dtypes = {0: dtype, 1: dtype}
    dtypes[abi.MOTION_DST_REF], dtypes[abi.MOTION_DST_BLOCK] = torch.int32, torch.int8
    plan = plan_for(seq, desc, sc, win, n)
    names = tensor_names(form, mask)
    with torch.cuda.device(device):
        if out is None:
            dev = torch.device("cuda", device)
            out = {name: torch.empty(_shape(form, plan, k, n), dtype=dtypes[k], device=dev) for k, name in names.items()}
        ptrs, pitches, pstrides, bstrides = [None] * 4, [0] * 4, [0] * 4, [0] * 4
        for key in out:
            if key not in names.values():
                raise ValueError("out: no tensor %r in this export (one of %s)" % (key, ", ".join(sorted(names.values()))))
        for k, name in names.items():
            t = out.get(name)
            if t is None:
                continue
            shape = _shape(form, plan, k, n)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dtypes[k] or t.get_device() != device:
                raise ValueError("out[%r]: a %s tensor of shape %s on device %d" % (name, dtypes[k], shape, device))
            st, es = t.stride(), t.element_size()
            if st[-1] != 1 or (len(shape) == 5 and st[1] != 2 * st[2]):
                raise ValueError("out[%r]: elements dense within a row, channels equally far apart (stride %s)" % (name, st))
            ptrs[k], pitches[k], pstrides[k], bstrides[k] = t.data_ptr(), st[-2] * es, st[-3] * es, st[0] * es
        if enqueue:
            call(desc, sc, win, ptrs, pitches, pstrides, bstrides, torch.cuda.current_stream(device).cuda_stream)
    return out


def c_args(ptrs, pitches, pstrides, bstrides):
    """the ctypes arguments (dst_mv[2], dst_ref, dst_block, pitch[4], plane stride[4], batch stride[4]) of the C entry points"""
    mv = (C.c_void_p * 2)(ptrs[0], ptrs[1])
    return (mv, C.c_void_p(ptrs[2]), C.c_void_p(ptrs[3]), (C.c_int64 * 4)(*pitches), (C.c_int64 * 4)(*pstrides), (C.c_int64 * 4)(*bstrides))
