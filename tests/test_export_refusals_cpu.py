"""Which refusal wins: the seven plan functions of the export side (host code, no GPU) fed inputs that break two rules at once.  The
expected status is the one of the rule the plan function checks first, and a refused plan is all zero.  Where an order depends on the
chroma format (a rule that 4:0:0 or 4:2:2 does not have), the same input is fed for more than one format."""
import ctypes as C

import pytest

import libhm_amd
from libhm_amd import abi

OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
F16 = abi.SAMPLE_F16


def _seq(fmt=1, width=64, height=48):
    s = abi.make_seq(width, height, 8)
    s.chroma_format = fmt
    return s


def _desc(layout=abi.EXPORT_PLANAR, reserved=0, **kw):
    d = abi.make_export_desc(layout, **kw)
    d.reserved[0] = reserved
    return d


def _scale(width=32, height=24, filter=abi.SCALE_BILINEAR, reserved=0):
    s = abi.make_export_scale(width, height, filter)
    s.reserved[0] = reserved
    return s


def _tensor(sample_type=F16, scale=(1.0, 1.0, 1.0), reserved=0):
    t = abi.make_export_tensor(sample_type, scale)
    t.reserved[0] = reserved
    return t


def _win(crop=(0, 0, 0, 0), flip=0, reserved=0):
    w = abi.make_export_window(crop)
    w.flip, w.reserved[1] = flip, reserved
    return w


def _pixel(order=abi.PIXEL_RGBA, alpha=-1, reserved=0):
    p = abi.make_export_pixel(order, alpha)
    p.reserved[0] = reserved
    return p


def _motion(form=abi.MOTION_DENSE, lists=3, sample_type=abi.SAMPLE_F32, crop=(0, 0, 0, 0), reserved=0):
    d = abi.make_motion_desc(form, lists, sample_type, crop)
    d.reserved[0] = reserved
    return d


def _resid(form=abi.RESIDUAL_DENSE, components=7, sample_type=abi.SAMPLE_F32, crop=(0, 0, 0, 0), scale=(1.0, 1.0, 1.0), reserved=0):
    d = abi.make_residual_desc(form, components, sample_type, crop, scale)
    d.reserved[0] = reserved
    return d


def _ref(x):
    return C.byref(x) if x is not None else None


def _wins(w):
    return (None, 1) if w is None else ((abi.ExportWindow * max(len(w), 1))(*w), len(w))


def _refused(plan_type, call, want):
    """the status, and -- for a refusal -- every byte of a plan that was all ones before the call"""
    plan = plan_type()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    st = call(C.byref(plan))
    assert st == want, "status %d, expected %d" % (st, want)
    if want != OK:
        assert bytes(plan) == bytes(C.sizeof(plan)), "a refused plan must be all zero"


RGB, SEMI = abi.EXPORT_RGB, abi.EXPORT_SEMIPLANAR
ODD_X, ODD_Y = (1, 1, 0, 0), (0, 0, 1, 1)      # crops that cut a chroma sample of 4:2:0 (ODD_X: of 4:2:2 too)
TINY = dict(width=1, height=24)                # 64 -> 1: beyond the 32x reduction limit (EUNSUPPORTED)


# ------------------------------------------------------------------------------------------------ hmgpu_export_plan_for
@pytest.mark.parametrize("fmt, desc, want", [
    (1, dict(layout=RGB, matrix=2), EUNSUPPORTED),                             # (alone: a matrix the export does not take)
    (1, dict(layout=RGB, matrix=2, reserved=1), EINVAL),                       # a reserved field before the matrix
    (1, dict(layout=RGB, matrix=2, crop=ODD_X), EINVAL),                       # the crop before the matrix
    (0, dict(layout=RGB, matrix=2, crop=ODD_X), EUNSUPPORTED),                 # 4:0:0 has no chroma sample to cut
    (2, dict(layout=RGB, matrix=2, crop=ODD_Y), EUNSUPPORTED),                 # nor has 4:2:2 vertically ...
    (2, dict(layout=RGB, matrix=2, crop=ODD_X), EINVAL),                       # ... but horizontally
    (1, dict(layout=RGB, matrix=2, full_range=2), EINVAL),                     # the range flag before the matrix
    (1, dict(layout=RGB, matrix=2, bit_depth=(7, 0)), EINVAL),                 # the output depth before the matrix
    (1, dict(layout=RGB, matrix=2, bytes_per_sample=3), EINVAL),
    (2, dict(layout=RGB, matrix=0), EINVAL),                                   # identity: 4:4:4 only
    (3, dict(layout=RGB, matrix=0, crop=ODD_X), OK),
    (1, dict(layout=7, matrix=2), EINVAL),
])
def test_export_plan(fmt, desc, want):
    s, d = _seq(fmt), _desc(**desc)
    _refused(abi.ExportPlan, lambda p: libhm_amd.lib().hmgpu_export_plan_for(C.byref(s), C.byref(d), p), want)


# ------------------------------------------------------------------------------------------------ hmgpu_export_scaled_plan_for
@pytest.mark.parametrize("fmt, desc, scale, want", [
    (1, dict(), TINY, EINVAL),                                                 # an odd output width before the ratio limit ...
    (0, dict(), TINY, EUNSUPPORTED),                                           # ... a rule 4:0:0 does not have ...
    (1, dict(layout=RGB), TINY, EUNSUPPORTED),                                 # ... nor RGB
    (1, dict(), dict(width=2, height=1), EINVAL),                              # an odd output height likewise ...
    (2, dict(), dict(width=2, height=1), EUNSUPPORTED),                        # ... which 4:2:2 allows: the ratio limit (48 -> 1)
    (1, dict(layout=RGB, matrix=2), dict(filter=9), EINVAL),                   # the scale's fields before the descriptor's plan
    (1, dict(layout=RGB, matrix=2), dict(reserved=1), EINVAL),
    (1, dict(layout=RGB, matrix=2), dict(width=0), EINVAL),
    (1, dict(layout=RGB, crop=ODD_X), TINY, EINVAL),                           # the descriptor's plan before the ratio limit
    (1, dict(layout=RGB, matrix=2), dict(width=31), EUNSUPPORTED),
    (1, dict(layout=RGB, bytes_per_sample=3), TINY, EINVAL),
])
def test_scaled_plan(fmt, desc, scale, want):
    s, d, sc = _seq(fmt), _desc(**desc), _scale(**scale)
    _refused(abi.ExportPlan, lambda p: libhm_amd.lib().hmgpu_export_scaled_plan_for(C.byref(s), C.byref(d), C.byref(sc), p), want)


# ------------------------------------------------------------------------------------------------ hmgpu_export_tensor_plan_for
@pytest.mark.parametrize("fmt, desc, scale, tensor, want", [
    (1, dict(layout=SEMI), None, dict(), EUNSUPPORTED),                        # (alone: no float NV12)
    (1, dict(layout=SEMI), None, dict(scale=(1.0, float("inf"), 1.0)), EINVAL),   # the tensor's own fields before the layout
    (1, dict(layout=SEMI), None, dict(reserved=1), EINVAL),
    (1, dict(layout=SEMI, bytes_per_sample=2), None, dict(), EINVAL),          # the container of the depth before the layout
    (1, dict(layout=SEMI, bytes_per_sample=2, bit_depth=10, msb_aligned=1), None, dict(), EINVAL),
    (1, dict(layout=RGB), TINY, dict(sample_type=9), EUNSUPPORTED),            # the scaled plan before the tensor
    (1, dict(layout=RGB, matrix=2), None, dict(sample_type=9), EUNSUPPORTED),  # the descriptor's plan before the tensor
    (1, dict(layout=RGB, matrix=2), None, dict(reserved=1), EUNSUPPORTED),
    (1, dict(layout=SEMI, crop=ODD_X), None, dict(), EINVAL),
    (1, dict(layout=SEMI), dict(filter=9), dict(), EINVAL),
    (0, dict(layout=SEMI), TINY, dict(sample_type=9), EUNSUPPORTED),
])
def test_tensor_plan(fmt, desc, scale, tensor, want):
    s, d, sc, t = _seq(fmt), _desc(**desc), _scale(**scale) if scale is not None else None, _tensor(**tensor)
    _refused(abi.ExportPlan, lambda p: libhm_amd.lib().hmgpu_export_tensor_plan_for(C.byref(s), C.byref(d), _ref(sc), C.byref(t), p), want)


# ------------------------------------------------------------------------------------------------ hmgpu_export_windows_plan_for
FULL, HALF, OTHER = (0, 0, 0, 0), (0, 32, 0, 24), (2, 30, 0, 24)              # 64x48, 32x24, 32x24 elsewhere
SMALL = (0, 62, 0, 24)                                                         # 2x24: 2 -> 32 is beyond the 8x enlargement limit
OVER = dict(width=32, height=1)                                                # 48 -> 1: EUNSUPPORTED for FULL; 24 -> 1 is allowed


@pytest.mark.parametrize("fmt, desc, scale, tensor, wins, want", [
    (1, dict(layout=RGB, crop=(2, 0, 0, 0), matrix=2), None, None, [dict()], EINVAL),            # the descriptor's crop before its plan
    (1, dict(layout=RGB, crop=(2, 0, 0, 0)), None, dict(sample_type=9), [dict()], EINVAL),
    (1, dict(layout=RGB, crop=(2, 0, 0, 0)), OVER, None, [dict()], EINVAL),
    (1, dict(layout=RGB, matrix=2), None, None, [dict()] * 17, EINVAL),                          # the count before the plan
    (1, dict(layout=RGB, matrix=2), None, None, [], EINVAL),
    (1, dict(layout=RGB), OVER, None, [dict(crop=FULL), dict(crop=HALF, reserved=1)], EUNSUPPORTED),   # the first failing window ...
    (1, dict(layout=RGB), OVER, None, [dict(crop=HALF, reserved=1), dict(crop=FULL)], EINVAL),         # ... in order
    (1, dict(layout=RGB), OVER, None, [dict(crop=HALF), dict(crop=FULL), dict(crop=ODD_X)], EUNSUPPORTED),
    (1, dict(layout=RGB), OVER, None, [dict(crop=HALF), dict(crop=ODD_X), dict(crop=FULL)], EINVAL),
    (1, dict(layout=RGB), OVER, None, [dict(crop=ODD_X), dict(crop=HALF, reserved=1)], EINVAL),
    (0, dict(layout=RGB), OVER, None, [dict(crop=ODD_X), dict(crop=HALF, reserved=1)], EUNSUPPORTED),  # 4:0:0: no chroma sample to cut
    (1, dict(layout=RGB), OVER, None, [dict(crop=FULL), dict(crop=FULL, flip=2)], EUNSUPPORTED),       # equal windows: the first one's plan
    (1, dict(layout=RGB), None, None, [dict(crop=FULL), dict(crop=FULL, flip=2)], EINVAL),             # ... and every window's own fields
    (1, dict(layout=RGB, matrix=2), None, None, [dict(crop=HALF), dict(crop=FULL)], EUNSUPPORTED),     # the plan before "unscaled: one size"
    (1, dict(layout=RGB), None, None, [dict(crop=HALF), dict(crop=FULL)], EINVAL),
    (1, dict(layout=SEMI), dict(), dict(), [dict(crop=HALF), dict(crop=ODD_X)], EUNSUPPORTED),         # the first window's tensor refusal
    (1, dict(layout=SEMI), dict(), dict(reserved=1), [dict(crop=HALF), dict(crop=SMALL)], EINVAL),
    (1, dict(layout=RGB), dict(width=32, height=24), None, [dict(crop=HALF), dict(crop=OTHER)], OK),
])
def test_windows_plan(fmt, desc, scale, tensor, wins, want):
    s, d = _seq(fmt), _desc(**desc)
    sc, t = _scale(**scale) if scale is not None else None, _tensor(**tensor) if tensor is not None else None
    w, n = _wins([_win(**k) for k in wins])
    _refused(abi.ExportPlan, lambda p: libhm_amd.lib().hmgpu_export_windows_plan_for(C.byref(s), C.byref(d), _ref(sc), _ref(t), n, w, p), want)


# ------------------------------------------------------------------------------------------------ hmgpu_export_pixels_plan_for
@pytest.mark.parametrize("fmt, desc, scale, tensor, wins, pixel, want", [
    (1, dict(layout=SEMI), None, dict(), None, dict(), EUNSUPPORTED),                            # the planar call's plan before the layout rule
    (1, dict(layout=SEMI), None, None, None, dict(), EINVAL),                                    # (packed pixels are RGB)
    (1, dict(layout=RGB, matrix=2), None, None, None, dict(order=9), EUNSUPPORTED),              # ... and before the pixel's own fields
    (1, dict(layout=RGB), TINY, None, None, dict(order=9), EUNSUPPORTED),
    (1, dict(layout=RGB), TINY, None, None, dict(alpha=256), EUNSUPPORTED),
    (1, dict(layout=RGB), None, None, None, dict(alpha=256, reserved=1), EINVAL),
    (1, dict(layout=RGB, crop=(2, 0, 0, 0), matrix=2), None, None, None, dict(order=9), EUNSUPPORTED),   # without windows the crop is allowed
    (1, dict(layout=RGB, crop=(2, 0, 0, 0), matrix=2), None, None, [dict()], dict(order=9), EINVAL),     # with windows it is refused first
    (1, dict(layout=RGB), OVER, None, [dict(crop=FULL), dict(crop=HALF, reserved=1)], dict(order=9), EUNSUPPORTED),
    (1, dict(layout=RGB), OVER, None, [dict(crop=HALF, reserved=1), dict(crop=FULL)], dict(order=9), EINVAL),
    (1, dict(layout=RGB), None, dict(sample_type=9), None, dict(order=9), EINVAL),
    (1, dict(layout=RGB), None, None, None, dict(alpha=255), OK),
])
def test_pixels_plan(fmt, desc, scale, tensor, wins, pixel, want):
    s, d, px = _seq(fmt), _desc(**desc), _pixel(**pixel)
    sc, t = _scale(**scale) if scale is not None else None, _tensor(**tensor) if tensor is not None else None
    w, n = _wins(None if wins is None else [_win(**k) for k in wins])
    _refused(abi.ExportPlan, lambda p: libhm_amd.lib().hmgpu_export_pixels_plan_for(C.byref(s), C.byref(d), _ref(sc), _ref(t), n, w, C.byref(px), p), want)


# ------------------------------------------------------------------------------------------------ hmgpu_motion_plan_for / hmgpu_residual_plan_for
NEAR = dict(filter=abi.SCALE_NEAREST)
NEAR_OVER = dict(width=32, height=1, filter=abi.SCALE_NEAREST)

# what both side-information plans refuse in the same order (dense form): (fmt, desc, scale, windows, status)
SIDE = [
    (1, dict(), dict(), [dict()], EUNSUPPORTED),                                                 # (alone: nothing is interpolated)
    (1, dict(), dict(reserved=1), [dict()], EINVAL),                                             # the scale's fields before its filter rule
    (1, dict(), dict(width=0), [dict()], EINVAL),
    (1, dict(), dict(filter=9), [dict()], EINVAL),
    (1, dict(), dict(), [dict(reserved=1)], EUNSUPPORTED),                                       # the filter rule before the windows
    (1, dict(), dict(), [dict(crop=ODD_X)], EUNSUPPORTED),
    (1, dict(crop=(8, 0, 0, 0)), dict(), [dict()], EINVAL),                                      # the descriptor before the filter rule
    (1, dict(sample_type=9), dict(), [dict()], EINVAL),
    (1, dict(reserved=1), dict(), [dict()], EINVAL),
    (1, dict(), dict(), None, EINVAL),                                                           # dense without windows
    (1, dict(), dict(), [], EINVAL),
    (1, dict(), NEAR_OVER, [dict(crop=FULL), dict(crop=HALF, reserved=1)], EUNSUPPORTED),        # the first failing window in order
    (1, dict(), NEAR_OVER, [dict(crop=HALF, reserved=1), dict(crop=FULL)], EINVAL),
    (1, dict(), NEAR_OVER, [dict(crop=FULL), dict(crop=ODD_X)], EUNSUPPORTED),
    (1, dict(), NEAR_OVER, [dict(crop=ODD_X), dict(crop=FULL)], EINVAL),
    (1, dict(), NEAR_OVER, [dict(crop=ODD_Y)], EINVAL),                                          # whole chroma samples before the ratio limit
    (0, dict(), NEAR_OVER, [dict(crop=ODD_Y)], EUNSUPPORTED),                                    # 4:0:0 has none
    (0, dict(), NEAR_OVER, [dict(crop=ODD_X)], EUNSUPPORTED),
    (1, dict(), NEAR_OVER, [dict(crop=(0, 64, 0, 0))], EINVAL),                                  # an empty window before the ratio limit
    (1, dict(), NEAR_OVER, [dict(crop=(-2, 0, 0, 0))], EINVAL),
    (1, dict(), None, [dict(crop=HALF), dict(crop=FULL), dict(crop=ODD_X)], EINVAL),             # unscaled: one size
    (1, dict(), None, [dict(crop=HALF), dict(crop=OTHER, flip=2)], EINVAL),
    (1, dict(), NEAR, [dict(crop=HALF), dict(crop=FULL, flip=1)], OK),
    (1, dict(), None, [dict(crop=HALF), dict(crop=OTHER, flip=1)], OK),
]


@pytest.mark.parametrize("fmt, desc, scale, wins, want", SIDE + [
    (2, dict(), NEAR_OVER, [dict(crop=ODD_Y)], EUNSUPPORTED),                                    # 4:2:2: whole chroma samples vertically
    (2, dict(), NEAR_OVER, [dict(crop=ODD_X)], EINVAL),
    (3, dict(), NEAR_OVER, [dict(crop=ODD_X)], EUNSUPPORTED),
    (1, dict(sample_type=abi.SAMPLE_UINT), dict(), [dict()], EINVAL),                            # dense vectors are float
    (1, dict(lists=4), dict(), [dict()], EINVAL),
    (1, dict(form=abi.MOTION_BLOCKS, sample_type=abi.SAMPLE_UINT), dict(), None, EINVAL),        # blocks take no scale, whatever its filter
    (1, dict(form=abi.MOTION_BLOCKS, sample_type=abi.SAMPLE_UINT, crop=(2, 0, 0, 0)), None, None, EINVAL),
    (1, dict(form=abi.MOTION_BLOCKS, sample_type=abi.SAMPLE_UINT, crop=(4, 0, 0, 0)), None, None, OK),
])
def test_motion_plan(fmt, desc, scale, wins, want):
    s, d, sc = _seq(fmt), _motion(**desc), _scale(**scale) if scale is not None else None
    w, n = _wins(None if wins is None else [_win(**k) for k in wins])
    _refused(abi.MotionPlan, lambda p: libhm_amd.lib().hmgpu_motion_plan_for(C.byref(s), C.byref(d), _ref(sc), n, w, p), want)


def test_motion_plan_sequence_before_everything():
    s, d, sc = _seq(1, 62, 48), _motion(), _scale()
    w, n = _wins([_win()])
    _refused(abi.MotionPlan, lambda p: libhm_amd.lib().hmgpu_motion_plan_for(C.byref(s), C.byref(d), C.byref(sc), n, w, p), EINVAL)


@pytest.mark.parametrize("fmt, desc, scale, wins, want", SIDE + [
    (2, dict(), NEAR, [dict()], EUNSUPPORTED),                                                   # (alone: 4:2:2 / 4:4:4 have no residual export)
    (2, dict(), dict(filter=9), [dict()], EINVAL),                                               # bad scale fields before the format
    (3, dict(), dict(reserved=1), [dict()], EINVAL),
    (2, dict(reserved=1), NEAR, [dict()], EINVAL),                                               # bad descriptor fields before the format
    (3, dict(components=0), NEAR, [dict()], EINVAL),
    (2, dict(form=5), NEAR, [dict()], EINVAL),
    (2, dict(sample_type=9), NEAR, [dict()], EUNSUPPORTED),                                      # the format before what depends on the form
    (2, dict(crop=(8, 0, 0, 0)), NEAR, [dict()], EUNSUPPORTED),
    (2, dict(), NEAR, None, EUNSUPPORTED),
    (2, dict(), NEAR, [dict(reserved=1)], EUNSUPPORTED),
    (2, dict(form=abi.RESIDUAL_PLANES, sample_type=abi.SAMPLE_UINT), NEAR, None, EUNSUPPORTED),
    (2, dict(), NEAR, [dict()] * 17, EINVAL),                                                    # the count before the format
    (1, dict(scale=(1.0, float("nan"), 1.0)), dict(), [dict()], EINVAL),                         # a component's scale before the filter rule
    (1, dict(scale=(1.0, float("nan"), 1.0), components=5), dict(), [dict()], EUNSUPPORTED),     # ... of a component the call exports
    (1, dict(scale=(1.0, float("nan"), 1.0), sample_type=abi.SAMPLE_UINT), dict(), [dict()], EUNSUPPORTED),
    (1, dict(form=abi.RESIDUAL_PLANES, sample_type=abi.SAMPLE_UINT), dict(), None, EINVAL),      # planes take no scale, whatever its filter
    (1, dict(form=abi.RESIDUAL_PLANES, sample_type=abi.SAMPLE_UINT, crop=(4, 0, 0, 0)), None, None, EINVAL),
    (1, dict(form=abi.RESIDUAL_PLANES, sample_type=abi.SAMPLE_UINT, crop=(8, 0, 0, 0)), None, None, OK),
])
def test_residual_plan(fmt, desc, scale, wins, want):
    s, d, sc = _seq(fmt), _resid(**desc), _scale(**scale) if scale is not None else None
    w, n = _wins(None if wins is None else [_win(**k) for k in wins])
    _refused(abi.ResidualPlan, lambda p: libhm_amd.lib().hmgpu_residual_plan_for(C.byref(s), C.byref(d), _ref(sc), n, w, p), want)


def test_residual_plan_sequence_before_everything():
    s, d, sc = _seq(2, 60, 48), _resid(), _scale(**NEAR)
    w, n = _wins([_win()])
    _refused(abi.ResidualPlan, lambda p: libhm_amd.lib().hmgpu_residual_plan_for(C.byref(s), C.byref(d), C.byref(sc), n, w, p), EINVAL)


# ------------------------------------------------------------------------------------------------ a wider entry reproduces the narrower one
# include/hmgpu.h: every wider plan entry validates what it shares with a narrower one "by the same code with the same statuses in the
# same order".  Each wider entry is given the stages of a narrower one plus valid descriptors of its own, over a grid of inputs that
# the narrower entry takes or refuses for every kind of reason: its answer is the narrower entry's refusal, else its own rule alone.
GRID_DESCS = [dict(layout=RGB), dict(layout=RGB, matrix=2), dict(), dict(layout=RGB, crop=ODD_X),
              dict(layout=RGB, bit_depth=(10, 10), bytes_per_sample=2)]
GRID_SCALES = [None, dict(), TINY, dict(filter=9)]
GRID_TENSORS = [None, dict(), dict(sample_type=9)]
GRID_WINS = [None, [dict(crop=HALF), dict(crop=FULL)], [dict(crop=ODD_X)], [dict(crop=FULL), dict(crop=FULL, flip=2)],
             [dict(crop=HALF), dict(crop=HALF, flip=1)]]
GRID_PIXELS = [None, dict(), dict(order=99), dict(alpha=300)]
TWO_SIZES = 1                                   # of GRID_WINS: the one list the warp entry, whose windows may differ in size, takes
WARP_W, WARP_H = 40, 30


def _plan_of(call):
    plan = abi.ExportPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    return call(C.byref(plan)), bytes(plan)


def _grid(fmt, scales):
    """(case, seq, desc, scale, tensor, windows, n, pixel, the narrower entry's status and plan)"""
    L = libhm_amd.lib()
    s = _seq(fmt)
    for di, dk in enumerate(GRID_DESCS):
        for si, sk in enumerate(scales):
            for ti, tk in enumerate(GRID_TENSORS):
                for wi, wk in enumerate(GRID_WINS):
                    for pi, pk in enumerate(GRID_PIXELS):
                        d = _desc(**dk)
                        sc, t = _scale(**sk) if sk is not None else None, _tensor(**tk) if tk is not None else None
                        w, n = _wins(None if wk is None else [_win(**k) for k in wk])
                        px = _pixel(**pk) if pk is not None else None
                        if px is not None:
                            base = _plan_of(lambda p: L.hmgpu_export_pixels_plan_for(C.byref(s), C.byref(d), _ref(sc), _ref(t), n, w, C.byref(px), p))
                        elif w is not None:
                            base = _plan_of(lambda p: L.hmgpu_export_windows_plan_for(C.byref(s), C.byref(d), _ref(sc), _ref(t), n, w, p))
                        else:
                            base = _plan_of(lambda p: L.hmgpu_export_tensor_plan_for(C.byref(s), C.byref(d), _ref(sc), _ref(t), p))
                        yield (fmt, di, si, ti, wi, pi), s, d, sc, t, w, n, px, base


def _own_rule(base, d, colour, chroma):
    """what a colour and / or chroma entry answers where the narrower entry answered `base`: the colour rule first"""
    st, plan = base
    zero = bytes(len(plan))
    if st != OK:
        return st, zero
    if d.layout != RGB:
        return EINVAL, zero
    if colour and (d.bit_depth[0] or 8) != 8:   # the LUT's depth is 8, the sequence's too
        return EINVAL, zero
    return OK, plan


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_colour_and_chroma_plans_reproduce_the_narrower_entry(fmt):
    L = libhm_amd.lib()
    ld, ch = abi.make_colour_lut_desc(8, 17, False), abi.make_export_chroma(abi.CHROMA_LINEAR, 0)
    bad, cases = [], 0
    for case, s, d, sc, t, w, n, px, base in _grid(fmt, GRID_SCALES):
        head = (C.byref(s), C.byref(d), _ref(sc), _ref(t), n, w, _ref(px))
        got = {"colour": _plan_of(lambda p: L.hmgpu_export_colour_plan_for(*head, C.byref(ld), p)),
               "chroma": _plan_of(lambda p: L.hmgpu_export_chroma_plan_for(*head, None, C.byref(ch), p)),
               "both": _plan_of(lambda p: L.hmgpu_export_chroma_plan_for(*head, C.byref(ld), C.byref(ch), p))}
        want = {"colour": _own_rule(base, d, True, False), "chroma": _own_rule(base, d, False, True), "both": _own_rule(base, d, True, True)}
        bad += [(case, k, got[k][0], want[k][0]) for k in got if got[k] != want[k]]
        cases += 1
    assert cases == 1200 and not bad, bad[:10]


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_warp_plan_reproduces_the_narrower_entry(fmt):
    L = libhm_amd.lib()
    ld, ch = abi.make_colour_lut_desc(8, 17, False), abi.make_export_chroma(abi.CHROMA_LINEAR, 0)
    wp = abi.make_export_warp(WARP_W, WARP_H)
    bad, cases = [], 0
    for case, s, d, sc, t, w, n, px, base in _grid(fmt, [None]):
        cases += 1
        if case[4] == TWO_SIZES:
            continue
        maps = abi.warp_map_array([(65536, 0, 0, 0, 65536, 0)] * n)
        for stages, colour in (((None, None), False), ((C.byref(ld), C.byref(ch)), True)):
            st, plan = _plan_of(lambda p: L.hmgpu_export_warp_plan_for(C.byref(s), C.byref(d), _ref(t), n, w, _ref(px), *stages,
                                                                       C.byref(wp), maps, p))
            want = _own_rule(base, d, colour, colour)
            if st != want[0] or (st != OK and plan != want[1]):
                bad.append((case, colour, st, want[0]))
            elif st == OK:
                got, was = abi.ExportPlan.from_buffer_copy(plan), abi.ExportPlan.from_buffer_copy(base[1])
                if got.planes != was.planes or any((got.width[k], got.height[k]) != (WARP_W, WARP_H) for k in range(got.planes)):
                    bad.append((case, colour, "plan"))
    assert cases == 300 and not bad, bad[:10]
