"""The colour stage of the RGB exports without a device: properties of the numpy restatement (tests/export_colour_ref.py), the
refusals of hmgpu_export_colour_plan_for and of hmgpu_colour_lut_check (the rules of hmgpu_colour_lut_create that need no context),
the .cube loader and the host LUT builder against published values."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export
from tests import export_colour_ref as cref

DEPTHS, SIZES = (8, 10, 12, 16), (2, 17, 33, 65)
OK, EINVAL, EUNSUPPORTED = abi.HMGPU_OK, abi.HMGPU_EINVAL, abi.HMGPU_EUNSUPPORTED


def random_rgb(depth, seed, h=40, w=48):
    """random integers with forced extremes and ties in the first pixels"""
    m = (1 << depth) - 1
    rgb = np.random.default_rng(seed).integers(0, m + 1, (3, h, w))
    rgb[:, 0, 0] = 0
    rgb[:, 0, 1] = m
    rgb[:, 0, 2] = m // 3                                             # a three-way tie
    rgb[:, 0, 3] = (m // 5, m // 5, m // 2)                           # a two-way tie
    rgb[:, 0, 4] = (m, 0, m // 2)
    return rgb


def random_lattice(size, depth, seed):
    return np.random.default_rng(seed).integers(0, 1 << depth, (size, size, size, 3)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES)
def test_reference_facts(depth, size):
    """what the arithmetic promises, recomputed: all six orderings and both ties occur, no sum overflows (asserted inside
    lut_apply), a constant lattice returns the constant, and the identity lattice returns the input exactly where the positions
    are exact multiples (depth < 16) and within 1 at depth 16, where full scale stops one short"""
    rgb = random_rgb(depth, 100 * depth + size)
    assert cref.covered(cref.coverage(rgb, depth, size, None))
    m = (1 << depth) - 1
    const = np.empty((size, size, size, 3), np.uint16)
    const[...] = (m, 0, m // 7)
    out = cref.lut_apply(rgb, depth, const, None)
    assert all((out[c] == v).all() for c, v in enumerate((m, 0, m // 7)))
    out = cref.lut_apply(rgb, depth, cref.identity_lattice(size, depth), None)
    err = int(np.abs(out - rgb).max())
    # position u = v * 65535 / M exactly (bit replication) for depth < 16, so node spacing and input spacing agree; at depth 16 the
    # fraction is taken of 65536, not 65535, which moves a value by less than one code value
    assert err == 0 if depth < 16 else err <= 1
    if depth == 16:
        assert cref.lut_apply(np.full((3, 1), m), depth, cref.identity_lattice(size, depth), None).tolist() == [[m - 1]] * 3


@pytest.mark.parametrize("depth,size", [(8, 2), (10, 17), (12, 33), (16, 65)])
def test_reference_symmetries(depth, size):
    rgb = random_rgb(depth, 7 * depth + size)
    lat = random_lattice(size, depth, size)
    out = cref.lut_apply(rgb, depth, lat, None)
    # the lattice with its R and B outputs exchanged exchanges the outputs
    assert np.array_equal(cref.lut_apply(rgb, depth, lat[..., ::-1], None), out[::-1])
    # ... and with its R and B axes exchanged as well, it is the same function of the exchanged input
    assert np.array_equal(cref.lut_apply(rgb[::-1], depth, lat.transpose(2, 1, 0, 3)[..., ::-1], None), out[::-1])
    # a separable lattice (channel c a function of axis c alone) is 1D linear interpolation per channel
    curves = np.random.default_rng(depth).integers(0, 1 << depth, (3, size))
    sep = np.zeros((size, size, size, 3), np.uint16)
    sep[..., 0] = curves[0][None, None, :]
    sep[..., 1] = curves[1][None, :, None]
    sep[..., 2] = curves[2][:, None, None]
    shaper = np.random.default_rng(size).integers(0, 65536, (3, 1 << depth)).astype(np.uint16)
    for sh in (None, shaper):
        i, f = cref.cells(cref.positions(rgb, depth, sh), size)
        want = np.stack([((65536 - f[c]) * curves[c][i[c]] + f[c] * curves[c][i[c] + 1] + 32768) >> 16 for c in range(3)])
        assert np.array_equal(cref.lut_apply(rgb, depth, sep, sh), want)
    # a shaper-only LUT is the table
    codes = np.random.default_rng(1).integers(0, 1 << depth, (3, 1 << depth)).astype(np.uint16)
    assert np.array_equal(cref.lut_apply(rgb, depth, None, codes), np.stack([codes[c][rgb[c]] for c in range(3)]))


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_struct_matches_the_header():
    assert C.sizeof(abi.ColourLutDesc) == 32 and abi.ColourLutDesc.reserved.offset == 12
    assert abi.COLOUR_MAX_LUTS == 8


def plan_status(seq, desc, lut, scale=None, tensor=None, windows=None, pixel=None):
    plan = abi.ExportPlan()
    st = libhm_amd.lib().hmgpu_export_colour_plan_for(C.byref(seq), C.byref(desc), abi.ref(scale), abi.ref(tensor),
                                                      len(windows) if windows else 1, abi.window_array(windows), abi.ref(pixel), abi.ref(lut),
                                                      C.byref(plan))
    return st, plan


def plan_bytes(plan):
    return bytes(C.string_at(C.byref(plan), C.sizeof(plan)))


def test_plan_is_the_matching_calls_plan():
    seq = abi.make_seq(200, 72, 10, 10)
    lut = abi.make_colour_lut_desc(10, 17, 0)
    desc = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, 0, (2, 4, 2, 0))
    tensor = abi.make_export_tensor(abi.SAMPLE_F16)
    scale = abi.make_export_scale(30, 20, abi.SCALE_BICUBIC)
    px = abi.make_export_pixel(abi.PIXEL_BGRA)
    st, plan = plan_status(seq, desc, lut, scale, tensor)
    assert st == OK and plan_bytes(plan) == plan_bytes(libhm_amd.export_tensor_plan(seq, desc, scale, tensor))
    st, plan = plan_status(seq, desc, lut, scale, tensor, pixel=px)
    assert st == OK and plan_bytes(plan) == plan_bytes(libhm_amd.export_pixels_plan(seq, desc, scale, tensor, None, px))
    d0 = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2)
    win = [abi.make_export_window((2, 102, 2, 30)), abi.make_export_window((4, 100, 0, 32), True)]
    st, plan = plan_status(seq, d0, lut, None, None, win)
    assert st == OK and plan_bytes(plan) == plan_bytes(libhm_amd.export_windows_plan(seq, d0, None, None, win))
    # depth 0 in the descriptor: the coding depth
    assert plan_status(seq, abi.make_export_desc(abi.EXPORT_RGB, (0, 0), 2), lut)[0] == OK
    # a shaper-only description
    assert plan_status(seq, d0, abi.make_colour_lut_desc(10, 0, 1))[0] == OK


def test_plan_refusals_in_order():
    seq = abi.make_seq(200, 72, 10, 10)
    good = abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2)
    lut = abi.make_colour_lut_desc(10, 17, 0)
    wrong_depth = abi.make_colour_lut_desc(8, 17, 0)
    zero = bytes(C.sizeof(abi.ExportPlan))

    def refused(want, desc, lut_, **kw):
        st, plan = plan_status(seq, desc, lut_, **kw)
        assert st == want and plan_bytes(plan) == zero, (st, want)

    # the matching call's own refusals come first, with their statuses: each is given a LUT of the wrong depth as well
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 1), wrong_depth)                    # the container
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, crop=(-2, 0, 0, 0)), wrong_depth)
    refused(EUNSUPPORTED, abi.make_export_desc(abi.EXPORT_RGB, (10, 10), 2, matrix=4), wrong_depth)
    refused(EUNSUPPORTED, good, wrong_depth, scale=abi.make_export_scale(2, 2, abi.SCALE_BILINEAR))   # 100x down
    refused(EINVAL, good, wrong_depth, tensor=abi.make_export_tensor(7))
    refused(EINVAL, good, wrong_depth, windows=[abi.make_export_window((0, 0, 0, 0), 2)])
    refused(EINVAL, good, wrong_depth, pixel=abi.make_export_pixel(9))
    refused(EUNSUPPORTED, abi.make_export_desc(abi.EXPORT_SEMIPLANAR, (10, 10), 2), lut, tensor=abi.make_export_tensor(abi.SAMPLE_F16))
    # then the layout ...
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_PLANAR, (10, 10), 2), lut)
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_SEMIPLANAR, (10, 10), 2), lut)
    # ... the description of the LUT ...
    refused(EINVAL, good, None)
    for depth, size, shaper in ((7, 17, 0), (17, 17, 0), (10, 1, 0), (10, 66, 0), (10, -1, 1), (10, 0, 0), (10, 17, 2)):
        d = abi.make_colour_lut_desc(depth, size, 0)
        d.has_shaper = shaper
        refused(EINVAL, good, d)
    for k in range(5):
        d = abi.make_colour_lut_desc(10, 17, 0)
        d.reserved[k] = 1
        refused(EINVAL, good, d)
    # ... and its depth against the call's
    refused(EINVAL, good, wrong_depth)
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_RGB, (0, 0), 2), abi.make_colour_lut_desc(12, 17, 0))
    refused(EINVAL, abi.make_export_desc(abi.EXPORT_RGB, (8, 8), 1), lut)
    for args in ((None, good, lut), (seq, None, lut)):
        st = libhm_amd.lib().hmgpu_export_colour_plan_for(abi.ref(args[0]), abi.ref(args[1]), None, None, 1, None, None, abi.ref(args[2]),
                                                          C.byref(abi.ExportPlan()))
        assert st == EINVAL
    assert libhm_amd.lib().hmgpu_export_colour_plan_for(C.byref(seq), C.byref(good), None, None, 1, None, None, C.byref(lut), None) == EINVAL


def test_lut_refusals_that_need_no_device():
    check = libhm_amd.lib().hmgpu_colour_lut_check
    lat = random_lattice(3, 10, 1)
    shaper = np.random.default_rng(2).integers(0, 65536, (3, 1024)).astype(np.uint16)
    codes = (shaper >> 6).astype(np.uint16)
    assert libhm_amd.colour_lut_status(lat, None, 10) == OK
    assert libhm_amd.colour_lut_status(lat, shaper, 10) == OK                     # positions may use all 16 bits
    assert libhm_amd.colour_lut_status(None, codes, 10) == OK
    for depth, size, has in ((7, 3, 1), (17, 3, 1), (10, 1, 1), (10, 66, 1), (10, 0, 0), (10, 3, 2), (10, 3, -1)):
        d = abi.make_colour_lut_desc(depth, size, 1)
        d.has_shaper = has
        assert libhm_amd.colour_lut_status(lat, shaper, 10, desc=d) == EINVAL, (depth, size, has)
    for k in range(5):
        d = abi.make_colour_lut_desc(10, 3, 1)
        d.reserved[k] = -1
        assert libhm_amd.colour_lut_status(lat, shaper, 10, desc=d) == EINVAL
    # pointers that are needed
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert check(None, p(shaper), p(lat)) == EINVAL
    assert check(C.byref(abi.make_colour_lut_desc(10, 3, 1)), None, p(lat)) == EINVAL
    assert check(C.byref(abi.make_colour_lut_desc(10, 3, 1)), p(shaper), None) == EINVAL
    assert check(C.byref(abi.make_colour_lut_desc(10, 3, 0)), None, p(lat)) == OK  # (no shaper: none needed)
    assert check(C.byref(abi.make_colour_lut_desc(10, 0, 1)), p(codes), None) == OK
    # a node above M, in the last node's last channel and in the first
    for at in ((2, 2, 2, 2), (0, 0, 0, 0)):
        bad = lat.copy()
        bad[at] = 1024
        assert libhm_amd.colour_lut_status(bad, None, 10) == EINVAL
        assert libhm_amd.colour_lut_status(bad, shaper, 10) == EINVAL
    # an entry of a shaper-only LUT above M
    bad = codes.copy()
    bad[2, 1023] = 1024
    assert libhm_amd.colour_lut_status(None, bad, 10) == EINVAL
    # a context is looked at last, and a null one is refused
    assert libhm_amd.lib().hmgpu_colour_lut_create(None, C.byref(abi.make_colour_lut_desc(10, 3, 0)), None, p(lat), C.byref(C.c_int64())) == EINVAL
    assert libhm_amd.lib().hmgpu_colour_lut_destroy(None, 1) == EINVAL
    with pytest.raises(ValueError):
        libhm_amd.colour_lut_arrays(np.zeros((3, 3, 2, 3)), None, 8)
    with pytest.raises(ValueError):
        libhm_amd.colour_lut_arrays(None, np.zeros((3, 255)), 8)
    with pytest.raises(ValueError):
        libhm_amd.colour_lut_arrays(np.full((2, 2, 2, 3), 70000), None, 8)


# ------------------------------------------------------------------------------------------------ 3. .cube files
def write_cube(path, size3, rows3, size1=0, rows1=(), head=()):
    lines = ["TITLE \"t\"", "# a comment"] + list(head)
    if size1:
        lines.append("LUT_1D_SIZE %d" % size1)
    if size3:
        lines.append("LUT_3D_SIZE %d" % size3)
    lines += ["%.6f %.6f %.6f" % tuple(r) for r in list(rows1) + list(rows3)]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_load_cube(tmp_path):
    # 2^3: the corners of the cube, R fastest; 0.5 rounds away from zero at depth 8 (127.5 -> 128)
    rows = [(r, g, b) for b in (0, 1) for g in (0, 1) for r in (0, 1)]
    rows[3] = (0.5, 0.25, 1.0)
    lat, sh = export.load_cube(write_cube(tmp_path / "a.cube", 2, rows, head=["DOMAIN_MIN 0 0 0", "DOMAIN_MAX 1.0 1.0 1.0"]), depth=8)
    assert sh is None and lat.shape == (2, 2, 2, 3) and lat.dtype == np.uint16
    assert lat[0, 0, 1].tolist() == [255, 0, 0] and lat[1, 0, 0].tolist() == [0, 0, 255] and lat[0, 1, 1].tolist() == [128, 64, 255]
    # 3^3 at depth 10: the identity, with values outside 0 .. 1 clipped
    rows = [(r / 2, g / 2, b / 2) for b in range(3) for g in range(3) for r in range(3)]
    rows[0], rows[26] = (-0.25, 0, 0), (1.5, 1, 1)
    lat, sh = export.load_cube(write_cube(tmp_path / "b.cube", 3, rows), depth=10)
    assert sh is None and np.array_equal(lat, cref.identity_lattice(3, 10))
    assert libhm_amd.colour_lut_status(lat, None, 10) == OK
    # a 1D table in front: resampled to 2^D positions by linear interpolation
    rows1 = [(0, 0, 0), (0.5, 0.25, 1.0), (1, 1, 1)]
    lat, sh = export.load_cube(write_cube(tmp_path / "c.cube", 3, rows, 3, rows1), depth=8)
    assert sh.shape == (3, 256) and sh[:, 0].tolist() == [0, 0, 0] and sh[:, 255].tolist() == [65535] * 3
    x = np.arange(256) / 255.0
    assert np.array_equal(sh[1], np.floor(np.interp(x, [0, 0.5, 1], [0, 0.25, 1]) * 65535 + 0.5).astype(np.uint16))
    assert libhm_amd.colour_lut_status(lat, sh, 8) == OK
    # a 1D table alone: a shaper-only LUT of code values
    lat, sh = export.load_cube(write_cube(tmp_path / "d.cube", 0, [], 3, rows1), depth=8)
    assert lat is None and sh[:, 255].tolist() == [255] * 3 and libhm_amd.colour_lut_status(None, sh, 8) == OK
    for name, kw in (("e", dict(head=["DOMAIN_MAX 2 2 2"])), ("f", dict(head=["DOMAIN_MIN 0 0.1 0"])), ("g", dict(head=["LUT_2D_SIZE 4"]))):
        with pytest.raises(ValueError):
            export.load_cube(write_cube(tmp_path / (name + ".cube"), 3, rows, **kw))
    with pytest.raises(ValueError):
        export.load_cube(write_cube(tmp_path / "h.cube", 3, rows[:-1]))


# ------------------------------------------------------------------------------------------------ 4. the LUT builder
def test_published_pins():
    # ST 2084 (BT.2100 table 4 levels): the pins have six decimals and d ln L / dE is about 13 at 0.5 and 9 at 0.75, so 1e-5 relative
    assert np.allclose(export.pq_eotf([0.508078, 0.751827, 1.0]), [100.0, 1000.0, 10000.0], rtol=1e-5, atol=0)
    assert np.allclose(export.pq_inverse_eotf([100.0, 1000.0, 10000.0]), [0.508078, 0.751827, 1.0], rtol=0, atol=1e-6)
    assert abs(float(export.hlg_inverse_oetf(0.5)) - 1.0 / 12.0) < 1e-15 and abs(float(export.hlg_oetf(1.0 / 12.0)) - 0.5) < 1e-15
    assert abs(float(export.hlg_inverse_oetf(1.0)) - 1.0) < 1e-6 and abs(float(export.hlg_oetf(1.0)) - 1.0) < 1e-6
    # BT.2087: BT.2020 to BT.709, four decimals
    want = [[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]]
    assert np.array_equal(np.round(export.primaries_matrix(9, 1), 4), np.array(want))
    assert np.allclose(export.primaries_matrix(9, 1) @ export.primaries_matrix(1, 9), np.eye(3), atol=1e-12)
    assert np.allclose(export.rgb_to_xyz(1)[1], [0.2126, 0.7152, 0.0722], atol=5e-5)
    assert np.allclose(export.rgb_to_xyz(9)[1], [0.2627, 0.6780, 0.0593], atol=5e-5)
    # HLG at its nominal peak: 1000 cd/m2
    assert np.allclose(export.to_display_light(np.ones(3), 9, 18, 203.0), 1000.0, rtol=1e-6)


@pytest.mark.parametrize("src,dst,tone", [((9, 16), (1, 1), "bt2390"), ((9, 18), (1, 13), "bt2390"), ((9, 16), (1, 1), "clip"),
                                          ((12, 13), (1, 1), "clip"), ((1, 1), (9, 16), "clip"), ((9, 18), (9, 16), "clip")])
def test_builder_keeps_grey_grey_and_monotone(src, dst, tone):
    for depth, size in ((8, 17), (10, 33)):
        lat, shaper = export.colour_lut(src, dst, depth, size, tone=tone)
        assert shaper is None and lat.shape == (size, size, size, 3) and libhm_amd.colour_lut_status(lat, None, depth) == OK
        d = np.arange(size)
        grey = lat[d, d, d].astype(np.int64)
        assert (grey[:, 0] == grey[:, 1]).all() and (grey[:, 1] == grey[:, 2]).all()
        assert (np.diff(grey[:, 0]) >= 0).all() and grey[0, 0] == 0 and grey[-1, 0] > grey[0, 0]
    # the tone curve keeps what clipping loses: 1000 cd/m2 and 4000 cd/m2 stay apart
    if tone == "bt2390" and src[1] == 16:
        lat, _ = export.colour_lut(src, dst, 10, 33, tone=tone)
        clip, _ = export.colour_lut(src, dst, 10, 33, tone="clip")
        assert lat[24, 24, 24, 0] < lat[29, 29, 29, 0] and clip[24, 24, 24, 0] == clip[29, 29, 29, 0] == 1023


def test_builder_identity_and_errors():
    for code in ((1, 1), (9, 16), (9, 18), (12, 13), (1, 8)):
        for depth, size in ((8, 2), (8, 3), (10, 17), (12, 33), (16, 65)):
            lat, _ = export.colour_lut(code, code, depth, size)
            assert np.array_equal(lat, cref.identity_lattice(size, depth))
    # SDR white: 203 cd/m2 in PQ is code value 0.58 (BT.2408)
    lat, _ = export.colour_lut((1, 1), (1, 16), 10, 3, white=203.0)
    assert abs(int(lat[2, 2, 2, 0]) - round(0.5807 * 1023)) <= 1
    for bad in (dict(src=(2, 1)), dict(src=(1, 2)), dict(dst=(1, 4)), dict(tone="hable"), dict(size=66), dict(depth=7)):
        kw = dict(src=(9, 16), dst=(1, 1), depth=10, size=17)
        kw.update(bad)
        with pytest.raises(ValueError):
            export.colour_lut(**kw)
    assert export.vui_source(9, 16) == (9, 16)
    with pytest.raises(ValueError):
        export.vui_source(2, 2)


# ------------------------------------------------------------------------------------------------ 5. the decoder's host side
def test_decoder_keeps_luts_on_the_host():
    """hmdec_colour_lut_create validates and stores without a device; handles are the decoder's own; lut="sdr" builds its LUT once
    per decoder, source and depth"""
    from libhm_amd import hmdec
    lat = random_lattice(3, 10, 1)
    with hmdec.Decoder(parse_only=True) as d:
        a, b = d.colour_lut(lat, None, 10), d.colour_lut(None, np.zeros((3, 256), np.uint16), 8)
        assert a.handle and b.handle and a.handle != b.handle and (a.depth, a.size, a.has_shaper) == (10, 3, False)
        bad = lat.copy()
        bad[1, 1, 1, 1] = 1024
        with pytest.raises(libhm_amd.HmgpuError) as e:
            d.colour_lut(bad, None, 10)
        assert e.value.status == EINVAL
        assert hmdec.lib().hmdec_colour_lut_destroy(d.ctx, a.handle + 100) == EINVAL
        a.close()
        assert a.handle == 0 and hmdec.lib().hmdec_colour_lut_destroy(d.ctx, 1) == EINVAL      # (already gone)
        sdr = hmdec._sdr_lut(d.ctx, (9, 16), 10)
        assert hmdec._sdr_lut(d.ctx, (9, 16), 10) is sdr and hmdec._sdr_lut(d.ctx, (9, 18), 10) is not sdr
        assert (sdr.depth, sdr.size) == (10, 33) and any(k[0] == d.ctx for k in hmdec._sdr_luts)
        ctx = d.ctx
    assert not any(k[0] == ctx for k in hmdec._sdr_luts)
