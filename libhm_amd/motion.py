"""Motion and block export to torch tensors (hmgpu_pictures_export_motion, k_motion.hip): the argument handling shared by
Context.export_motion, hmdec.export_motion_batch and hmdec.Picture.motion.  No compute here.

form "blocks": the grid of 4x4 luma blocks -- {"mv": int16 [N, L, 2, H4, W4] (hor, ver in quarter luma samples), "ref_poc": int32
[N, L, H4, W4] (abi.MOTION_NO_REF where a list is unused), "block": int8 [N, 4, H4, W4] (mode -1 / 0 inter / 1 intra, log2 CU size,
part_size, QP)}.  form "dense": one value per output sample of export_batch(windows=, flip=, size=, filter="nearest") -- {"flow0" /
"flow1": float [N, 2, H, W] (dx, dy in output samples), "ref_poc": int32 [N, L, H, W], "block": int8 [N, 4, H, W]}.  L counts the
lists selected by `lists`, in list order.
"""
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
    return export.side_plan("hmgpu_motion_plan_for", abi.MotionPlan(), seq, desc, scale, windows, n)


def describe(seq, n, form="blocks", lists=(0, 1), size=None, windows=None, flip=None, dtype=None, crop=(0, 0, 0, 0), strict=True):
    """(desc, abi.ExportScale or None, windows or None) of a call; dtype: None (float32), a torch float dtype or an abi.SAMPLE_* code;
    strict: blocks refuses the arguments of dense (else it leaves them aside)"""
    form = form_code(form)
    mask = lists_mask(lists)
    if form == abi.MOTION_BLOCKS:
        if strict and (size is not None or windows is not None or flip is not None or dtype is not None):
            raise ValueError("export_motion(form='blocks') takes crop only: size / windows / flip / dtype belong to form='dense'")
        return abi.make_motion_desc(form, mask, abi.SAMPLE_UINT, crop), None, None
    st = abi.SAMPLE_F32 if dtype is None else dtype if isinstance(dtype, int) else export.sample_type(dtype)
    return abi.make_motion_desc(form, mask, st), export.make_scale(size, "nearest"), export.dense_windows(seq, crop, windows, flip, n)


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
    desc, sc, win = describe(seq, n, form, lists, size, windows, flip, dtype, crop)
    form = desc.form
    vec = torch.int16 if form == abi.MOTION_BLOCKS else torch.float32 if dtype is None else dtype
    dtypes = {0: vec, 1: vec, abi.MOTION_DST_REF: torch.int32, abi.MOTION_DST_BLOCK: torch.int8}
    plan = plan_for(seq, desc, sc, win, n)
    with torch.cuda.device(device):
        out, ptrs, pitches, pstrides, bstrides = export.side_tensors(
            out, device, tensor_names(form, desc.lists), lambda k: _shape(form, plan, k, n), dtypes.get, 4,
            "elements dense within a row, channels equally far apart")
        if enqueue:
            call(desc, sc, win, ptrs, pitches, pstrides, bstrides, torch.cuda.current_stream(device).cuda_stream)
    return out


def c_args(ptrs, pitches, pstrides, bstrides):
    """the ctypes arguments (dst_mv[2], dst_ref, dst_block, pitch[4], plane stride[4], batch stride[4]) of the C entry points"""
    return (abi.ptr_array(ptrs[:2], 2), abi.addr(ptrs[2]), abi.addr(ptrs[3]), abi.i64_array(pitches, 4), abi.i64_array(pstrides, 4),
            abi.i64_array(bstrides, 4))
