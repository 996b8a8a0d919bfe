"""The chroma stage of the RGB exports without a device: the numpy restatement (tests/export_chroma_ref.py) against values worked
out by hand, hmgpu_export_chroma against the header, the refusals of hmgpu_export_chroma_plan_for in their order, the plans of
HMGPU_CHROMA_REPLICATE against the existing plans, and the parser's chroma sample location."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec
from tests import export_chroma_ref as chref
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED
LOCS = range(6)
H_CENTRED, V_PHASE = (1, 3, 5), {0: "centred", 1: "centred", 2: "co-sited", 3: "co-sited", 4: "bottom", 5: "bottom"}


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("loc", LOCS)
@pytest.mark.parametrize("cs", [(1, 1), (1, 0)])
def test_reference_keeps_a_constant(loc, cs):
    for v in (0, 1, 511, 1023, 4095):
        out = chref.upsample(np.full((7, 9), v, np.int16), cs[0], cs[1], loc)
        assert out.shape == (7 << cs[1], 18) and (out == v).all()


@pytest.mark.parametrize("loc", LOCS)
def test_reference_horizontal_ramp(loc):
    """C[j] = 8j: 4x co-sited and 4x - 2 centred away from the clamped ends; the ends as the table says"""
    n = 12
    out = chref.upsample(np.tile(8 * np.arange(n), (4, 1)), 1, 1, loc)
    x = np.arange(2 * n)
    assert (out == out[0]).all()                                          # rows of a horizontal ramp are equal
    row = out[0]
    if loc in H_CENTRED:
        assert np.array_equal(row[1:-1], (4 * x - 2)[1:-1])
        # x = 0: (j - 1: 1, j: 3) with j - 1 clamped to 0 -> C[0]; x = 2n - 1: (j: 3, j + 1: 1) with j + 1 clamped -> C[n - 1]
        assert row[0] == 0 and row[-1] == 8 * (n - 1)
    else:
        assert np.array_equal(row[:-1], (4 * x)[:-1])
        # x = 2n - 1: (j: 2, j + 1: 2) with j + 1 clamped -> C[n - 1]
        assert row[-1] == 8 * (n - 1)


@pytest.mark.parametrize("loc", LOCS)
def test_reference_vertical_ramp(loc):
    """the three vertical phases on C[j] = 8j down the rows: centred 4y - 2, co-sited 4y, bottom 4y - 4, the ends clamped"""
    n = 10
    out = chref.upsample(np.tile(8 * np.arange(n)[:, None], (1, 5)), 1, 1, loc)
    y = np.arange(2 * n)
    assert (out == out[:, :1]).all()
    col = out[:, 0]
    phase = V_PHASE[loc]
    if phase == "centred":
        assert np.array_equal(col[1:-1], (4 * y - 2)[1:-1]) and col[0] == 0 and col[-1] == 8 * (n - 1)
    elif phase == "co-sited":
        assert np.array_equal(col[:-1], (4 * y)[:-1]) and col[-1] == 8 * (n - 1)
    else:
        # even y: (j - 1: 2, j: 2) -> 8j - 4 = 4y - 4; odd y: (j: 4) -> 8j = 4y - 4; y = 0: j - 1 clamped -> C[0]
        assert np.array_equal(col[1:], (4 * y - 4)[1:]) and col[0] == 0


def test_reference_422_and_identity():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 1024, (6, 8)).astype(np.int16)
    outs = [chref.upsample(c, 1, 0, loc) for loc in LOCS]
    assert all(np.array_equal(o, outs[0]) for o in outs)                  # 4:2:2 ignores loc
    assert np.array_equal(outs[0][:, 0::2], c)                            # even columns: the sample itself
    want = (2 * c.astype(np.int64) + 2 * np.concatenate([c[:, 1:], c[:, -1:]], axis=1) + 2) >> 2
    assert np.array_equal(outs[0][:, 1::2], want)                         # odd columns: the mean of two, (2a + 2b) * 4 + 8 >> 4
    assert np.array_equal(chref.upsample(c, 0, 0, 3), c)                  # not subsampled: the identity
    planes = [c, c, c]
    assert all(a is b for a, b in zip(chref.upsample_planes(planes, 3, 2), planes))
    assert all(a is b for a, b in zip(chref.upsample_planes(planes, 0, 2), planes))


def test_reference_rounding_and_all_weights():
    """one isolated sample of 16 in a plane of zeros leaves exactly the product of its weights, every one of the sixteen products
    of (1, 3) x (1, 3) and of (2, 2, 4) occurring; the rounding is + 8 >> 4"""
    c = np.zeros((5, 5), np.int64)
    c[2, 2] = 16
    centred = chref.upsample(c, 1, 1, 1)                                  # both axes centred
    assert np.array_equal(centred[3:7, 3:7], np.outer([1, 3, 3, 1], [1, 3, 3, 1]))
    cosited = chref.upsample(c, 1, 1, 2)                                  # both axes co-sited
    assert np.array_equal(cosited[3:6, 3:6], np.outer([2, 4, 2], [2, 4, 2]))
    c[2, 2] = 1                                                           # 9 / 16 rounds to 1, 3 / 16 to 0, 8 / 16 to 1, 4 / 16 to 0
    assert np.array_equal(chref.upsample(c, 1, 1, 1)[3:7, 3:7], np.outer([0, 1, 1, 0], [0, 1, 1, 0]))
    assert np.array_equal(chref.upsample(c, 1, 1, 2)[3:6, 3:6], [[0, 1, 0], [1, 1, 1], [0, 1, 0]])


# ------------------------------------------------------------------------------------------------ 2. the descriptor
def test_struct_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n",'
                   'sizeof(hmgpu_export_chroma),offsetof(hmgpu_export_chroma,filter),offsetof(hmgpu_export_chroma,loc),'
                   'offsetof(hmgpu_export_chroma,reserved),HMGPU_CHROMA_REPLICATE,HMGPU_CHROMA_LINEAR);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    E = abi.ExportChroma
    assert got == [C.sizeof(E), E.filter.offset, E.loc.offset, E.reserved.offset, abi.CHROMA_REPLICATE, abi.CHROMA_LINEAR] == [32, 0, 4, 8, 0, 1]


def plan_bytes(plan):
    return bytes(C.string_at(C.byref(plan), C.sizeof(plan)))


def status(seq, desc, chroma, scale=None, tensor=None, windows=None, pixel=None, lut=None):
    return libhm_amd.export_chroma_status(seq, desc, scale, tensor, windows, pixel, lut, chroma)


def test_python_keyword_names():
    assert abi.chroma_stage("replicate", None) is None and abi.chroma_stage("replicate", 3) is None
    c = abi.chroma_stage("linear", None, 2)
    assert (c.filter, c.loc) == (abi.CHROMA_LINEAR, 2)
    assert abi.chroma_stage("linear", 5, 2).loc == 5
    with pytest.raises(ValueError):
        abi.chroma_stage("cubic", None)


# ------------------------------------------------------------------------------------------------ 3. refusals, in their order
def test_plan_refusals_in_order():
    seq = abi.make_seq(72, 40, 10, 10)
    good = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2)
    lin = abi.make_export_chroma(abi.CHROMA_LINEAR, 2)
    zero = bytes(C.sizeof(abi.ExportPlan))

    def refused(want, desc, chroma, **kw):
        st, plan = status(seq, desc, chroma, **kw)
        assert st == want and plan_bytes(plan) == zero, (st, want)

    assert status(seq, good, lin)[0] == OK
    # the matching call's own refusals come first, with their statuses: an unknown matrix is EUNSUPPORTED there, and stays so with a
    # chroma descriptor that would be EINVAL
    bad_matrix = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, matrix=7)
    refused(EUNSUPPORTED, bad_matrix, None)
    bad_crop = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, crop=(1, 0, 0, 0))
    refused(EINVAL, bad_crop, abi.make_export_chroma(7, 0))
    refused(EUNSUPPORTED, good, None, scale=abi.make_export_scale(1, 1, abi.SCALE_BILINEAR))      # a 72x reduction
    refused(EINVAL, good, lin, pixel=abi.make_export_pixel(99))
    refused(EINVAL, good, lin, lut=abi.make_colour_lut_desc(8, 17, 0))                            # the colour call's: LUT depth
    # 1. a layout that is not RGB: EINVAL, before the filter is looked at
    for layout in (abi.EXPORT_PLANAR, abi.EXPORT_SEMIPLANAR):
        yuv = abi.make_export_desc(layout, (10, 10), 2)
        refused(EINVAL, yuv, lin)
        refused(EINVAL, yuv, abi.make_export_chroma(7, 0))
        refused(EINVAL, yuv, abi.make_export_chroma(abi.CHROMA_REPLICATE, 0))
    # 2. chroma NULL, a reserved word, loc outside 0 .. 5: EINVAL, before the filter
    refused(EINVAL, good, None)
    for k in range(6):
        c = abi.make_export_chroma(7, 0)
        c.reserved[k] = 1
        refused(EINVAL, good, c)
    for loc in (-1, 6, 1 << 20):
        refused(EINVAL, good, abi.make_export_chroma(7, loc))
        refused(EINVAL, good, abi.make_export_chroma(abi.CHROMA_LINEAR, loc))
        refused(EINVAL, good, abi.make_export_chroma(abi.CHROMA_REPLICATE, loc))
    # 3. an unknown filter: EUNSUPPORTED
    for f in (-1, 2, 7):
        refused(EUNSUPPORTED, good, abi.make_export_chroma(f, 0))
    # every loc with every format; loc is validated where it is ignored too
    for fmt in range(4):
        seq.chroma_format = fmt
        for loc in LOCS:
            assert status(seq, good, abi.make_export_chroma(abi.CHROMA_LINEAR, loc))[0] == OK
        refused(EINVAL, good, abi.make_export_chroma(abi.CHROMA_LINEAR, 6))


# ------------------------------------------------------------------------------------------------ 4. the plans are the existing ones
@pytest.mark.parametrize("filt", [abi.CHROMA_REPLICATE, abi.CHROMA_LINEAR])
def test_plan_is_the_matching_calls_plan(filt):
    seq = abi.make_seq(200, 72, 10, 10)
    chroma = abi.make_export_chroma(filt, 3)
    lut = abi.make_colour_lut_desc(10, 17, 0)
    desc = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, 0, (2, 4, 2, 0))
    tensor = abi.make_export_tensor(abi.SAMPLE_F16)
    scale = abi.make_export_scale(30, 20, abi.SCALE_BICUBIC)
    px = abi.make_export_pixel(abi.PIXEL_BGRA)
    d0 = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2)
    win = [abi.make_export_window((2, 102, 2, 30)), abi.make_export_window((4, 100, 0, 32), True)]

    def same(plan_of, **kw):
        st, plan = status(seq, kw.pop("desc", desc), chroma, **kw)
        assert st == OK
        want = plan_of()
        for name, _ in abi.ExportPlan._fields_:
            a, b = getattr(plan, name), getattr(want, name)
            assert (a == b) if isinstance(a, int) else (list(a) == list(b)), name
        assert plan_bytes(plan) == plan_bytes(want)

    same(lambda: libhm_amd.export_plan(seq, desc))
    same(lambda: libhm_amd.export_scaled_plan(seq, desc, scale), scale=scale)
    same(lambda: libhm_amd.export_tensor_plan(seq, desc, scale, tensor), scale=scale, tensor=tensor)
    same(lambda: libhm_amd.export_pixels_plan(seq, desc, scale, tensor, None, px), scale=scale, tensor=tensor, pixel=px)
    same(lambda: libhm_amd.export_windows_plan(seq, d0, None, None, win), desc=d0, windows=win)
    same(lambda: libhm_amd.export_windows_plan(seq, d0, scale, tensor, win), desc=d0, scale=scale, tensor=tensor, windows=win)
    same(lambda: libhm_amd.export_pixels_plan(seq, d0, scale, tensor, win, px), desc=d0, scale=scale, tensor=tensor, windows=win, pixel=px)
    same(lambda: libhm_amd.export_colour_plan(seq, desc, scale, tensor, None, px, lut), scale=scale, tensor=tensor, pixel=px, lut=lut)
    same(lambda: libhm_amd.export_colour_plan(seq, d0, None, None, win, None, lut), desc=d0, windows=win, lut=lut)


# ------------------------------------------------------------------------------------------------ 5. the parser
def _chroma_locs(name):
    out = []
    with hmdec.Decoder(parse_only=True) as d:
        d.decode_stream(bytes(gu.load(name)["bitstream"]), on_output=lambda p: out.append((p.chroma_loc(), p.colour())))
    return out


def test_parser_keeps_the_chroma_sample_location():
    """the SPS of the rewritten fixture signals chroma_loc_info_present_flag = 1 with type 2 in both fields; everything behind those
    two codes still parses (the pictures come out), and the colour description in front of them is the source's"""
    new = _chroma_locs("export_vui_bt2020_chromaloc2_main10_208x120")
    old = _chroma_locs("export_vui_bt2020_main10_208x120")
    assert len(new) == len(old) == 2
    for (loc, colour), (loc0, colour0) in zip(new, old):
        assert loc == dict(present=1, top_field=2, bottom_field=2)
        assert loc0 == dict(present=0, top_field=0, bottom_field=0)
        assert colour == colour0 and colour["matrix"] == 9


def test_fixture_differs_from_its_source_in_the_sps_alone():
    a = bytes(gu.load("export_vui_bt2020_chromaloc2_main10_208x120")["bitstream"])
    b = bytes(gu.load("export_vui_bt2020_main10_208x120")["bitstream"])
    strip = lambda nal: bytes(nal).rstrip(b"\x00")                        # (the leading zero of a four-byte start code that follows)
    na, nb = [strip(n) for n in hmdec.split_nal_units(a)], [strip(n) for n in hmdec.split_nal_units(b)]
    assert len(na) == len(nb)
    differ = [i for i, (x, y) in enumerate(zip(na, nb)) if x != y]
    assert len(differ) == 1 and (na[differ[0]][0] >> 1) & 0x3f == 33      # one NAL unit, the SPS
