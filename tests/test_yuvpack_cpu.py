"""Packed YUV without a device (include/hmgpu.h "packed YUV"): the numpy model of tests/yuvpack_ref.py against hand-written bytes,
the structs against the header, and the plans and refusals of hmgpu_export_yuvpack_plan_for and hmgpu_import_yuvpack_plan_for with
the order the header states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import yuvpack_ref as yref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, 1, 3
CODES = {"uyvy": 0, "yuy2": 1, "y210": 2, "y216": 3, "v210": 4, "ayuv": 5, "y410": 6, "y416": 7}


def planes(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    m = 1 << yref.DEPTH[fmt]
    cw = w // 2 if yref.CHROMA[fmt] == 2 else w
    return rng.integers(0, m, (h, w)), rng.integers(0, m, (h, cw)), rng.integers(0, m, (h, cw))


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_unpack_inverts_pack(fmt):
    for w, h in ((72, 5), (70, 3), (2, 2), (46, 2), (50, 1)):
        y, cb, cr = planes(fmt, w, h, w + h)
        buf = yref.pack(fmt, y, cb, cr, yref.ALPHA_MAX[fmt], yref.row_bytes(fmt, w) + 24, canary=0xA5)
        got = yref.unpack(fmt, buf, w, h)
        assert all(np.array_equal(a, b) for a, b in zip(got, (y, cb, cr))), (fmt, w, h)
        assert np.all(buf[:, yref.row_bytes(fmt, w):] == 0xA5)


def test_one_unit_of_each_format_byte_by_byte():
    y2, cb1, cr1 = [[0x11, 0x22]], [[0x33]], [[0x44]]
    assert bytes(yref.pack("uyvy", y2, cb1, cr1)[0]) == bytes([0x33, 0x11, 0x44, 0x22])
    assert bytes(yref.pack("yuy2", y2, cb1, cr1)[0]) == bytes([0x11, 0x33, 0x22, 0x44])
    # y210: 0x3ff << 6 = 0xffc0, 0x001 << 6 = 0x0040, 0x2aa << 6 = 0xaa80, 0x155 << 6 = 0x5540; little endian, Y0 Cb Y1 Cr
    assert bytes(yref.pack("y210", [[0x3ff, 0x001]], [[0x2aa]], [[0x155]])[0]) == bytes([0xc0, 0xff, 0x80, 0xaa, 0x40, 0x00, 0x40, 0x55])
    assert bytes(yref.pack("y216", [[0xfedc, 0x0123]], [[0xba98]], [[0x4567]])[0]) == bytes([0xdc, 0xfe, 0x98, 0xba, 0x23, 0x01, 0x67, 0x45])
    assert bytes(yref.pack("ayuv", [[0x11]], [[0x33]], [[0x44]], alpha=0x80)[0]) == bytes([0x44, 0x33, 0x11, 0x80])
    # y410: Cb 0x155 | Y 0x3ff << 10 | Cr 0x001 << 20 | A 2 << 30 = 0x801ffd55
    assert bytes(yref.pack("y410", [[0x3ff]], [[0x155]], [[0x001]], alpha=2)[0]) == bytes([0x55, 0xfd, 0x1f, 0x80])
    assert bytes(yref.pack("y416", [[0x1122]], [[0x3344]], [[0x5566]], alpha=0x7788)[0]) == bytes([0x44, 0x33, 0x22, 0x11, 0x66, 0x55, 0x88, 0x77])


def test_a_v210_group_bit_by_bit():
    y = [[0x001, 0x002, 0x004, 0x008, 0x010, 0x3ff]]
    cb, cr = [[0x020, 0x040, 0x080]], [[0x100, 0x200, 0x155]]
    w = [0x020 | 0x001 << 10 | 0x100 << 20,        # Cb0 Y0 Cr0
         0x002 | 0x040 << 10 | 0x004 << 20,        # Y1 Cb1 Y2
         0x200 | 0x008 << 10 | 0x080 << 20,        # Cr1 Y3 Cb2
         0x010 | 0x155 << 10 | 0x3ff << 20]        # Y4 Cr2 Y5
    want = b"".join(int(v).to_bytes(4, "little") for v in w)
    got = yref.pack("v210", y, cb, cr)
    assert bytes(got[0]) == want
    bits = "".join(format(b, "08b")[::-1] for b in got[0])          # the row as a string of bits, bit 0 of byte 0 first
    fields = [0x020, 0x001, 0x100, 0x002, 0x040, 0x004, 0x200, 0x008, 0x080, 0x010, 0x155, 0x3ff]
    for k, v in enumerate(fields):
        at = 32 * (k // 3) + 10 * (k % 3)
        assert bits[at:at + 10] == format(v, "010b")[::-1], k
    for k in range(4):
        assert bits[32 * k + 30:32 * k + 32] == "00"


@pytest.mark.parametrize("w", [6, 8, 10, 46, 50, 2])
def test_v210_tails(w):
    """W mod 6 in {0, 2, 4}: absent fields are 0, bytes beyond the last group keep the canary"""
    h = 3
    m = np.full((h, w), 0x3ff), np.full((h, w // 2), 0x3ff), np.full((h, w // 2), 0x3ff)
    groups = (w + 5) // 6
    assert yref.row_bytes("v210", w) == 16 * groups
    buf = yref.pack("v210", *m, pitch=16 * groups + 16, canary=0xA5)
    assert np.all(buf[:, 16 * groups:] == 0xA5)
    words = buf[:, :16 * groups].copy().view("<u4").reshape(h, groups, 4)
    assert np.all(words[:, :-1] == 0x3fffffff)
    full = [0x3fffffff] * 4
    want = {0: full, 2: [0x3fffffff, 0x000003ff, 0, 0], 4: [0x3fffffff, 0x3fffffff, 0x000ffc00 | 0x3ff, 0]}[w % 6]
    # w mod 6 = 2: Y0 Y1, Cb0 Cr0;  4: Y0 .. Y3, Cb0 Cb1 Cr0 Cr1 -- w2 = Cr1 | Y3 << 10 (Cb2 absent), w3 = 0
    assert [int(v) for v in words[0, -1]] == want
    y, cb, cr = yref.unpack("v210", buf, w, h)
    assert y.shape == (h, w) and cb.shape == cr.shape == (h, w // 2) and all(np.all(p == 0x3ff) for p in (y, cb, cr))


def test_unpack_reads_over_what_is_not_a_value():
    y, cb, cr = planes("v210", 10, 2, 3)
    buf = yref.pack("v210", y, cb, cr)
    buf[:, 3::4] |= 0xC0                                                   # bits 30-31 of every word
    assert all(np.array_equal(a, b) for a, b in zip(yref.unpack("v210", buf, 10, 2), (y, cb, cr)))
    y, cb, cr = planes("y210", 8, 2, 4)
    buf = yref.pack("y210", y, cb, cr)
    buf[:, 0::2] |= 0x3F                                                   # the low six bits of every element
    assert all(np.array_equal(a, b) for a, b in zip(yref.unpack("y210", buf, 8, 2), (y, cb, cr)))
    for fmt in ("ayuv", "y410", "y416"):
        y, cb, cr = planes(fmt, 5, 2, 5)
        a, b = yref.pack(fmt, y, cb, cr, 0), yref.pack(fmt, y, cb, cr, yref.ALPHA_MAX[fmt])
        assert not np.array_equal(a, b)
        assert all(np.array_equal(p, q) for p, q in zip(yref.unpack(fmt, a, 5, 2), yref.unpack(fmt, b, 5, 2)))


# ------------------------------------------------------------------------------------------------ the structs
def test_structs_match_the_header(tmp_path):
    src = tmp_path / "yp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n",'
                   'sizeof(hmgpu_export_yuvpack),offsetof(hmgpu_export_yuvpack,format),offsetof(hmgpu_export_yuvpack,alpha),'
                   'offsetof(hmgpu_export_yuvpack,reserved),HMGPU_YUVPACK_UYVY,HMGPU_YUVPACK_YUY2,HMGPU_YUVPACK_Y210,HMGPU_YUVPACK_Y216,'
                   'HMGPU_YUVPACK_V210,HMGPU_YUVPACK_AYUV,HMGPU_YUVPACK_Y410,HMGPU_YUVPACK_Y416);return 0;}\n')
    exe = tmp_path / "yp"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P = abi.ExportYuvPack
    assert got == [C.sizeof(P), P.format.offset, P.alpha.offset, P.reserved.offset] + [abi.YUVPACKS[f] for f in yref.FORMATS]
    assert C.sizeof(P) == 32 and [abi.YUVPACKS[f] for f in yref.FORMATS] == list(range(8)) == [CODES[f] for f in yref.FORMATS]
    p = abi.make_export_yuvpack("y410", 3)
    assert (p.format, p.alpha, list(p.reserved)) == (6, 3, [0] * 6)
    for f in yref.FORMATS:
        c = abi.YUVPACKS[f]
        assert (abi.YUVPACK_CHROMA[c], abi.YUVPACK_DEPTH[c], abi.YUVPACK_ELEMENT[c]) == (yref.CHROMA[f], yref.DEPTH[f], yref.ELEMENT[f])


# ------------------------------------------------------------------------------------------------ plans and refusals
def _seq(fmt=1, w=72, h=40, bd=8):
    s = abi.make_seq(w, h, bd)
    s.chroma_format = fmt
    return s


def _desc(fmt, layout=abi.EXPORT_PLANAR, bd=None, nbytes=None, msb=0, crop=(0, 0, 0, 0)):
    d = yref.DEPTH[fmt]
    return abi.make_export_desc(layout, (d, d) if bd is None else bd, (1 if d <= 8 else 2) if nbytes is None else nbytes, msb, crop)


def _status(seq, desc, fmt, pack, tensor=None, windows=None, want=OK):
    plan = abi.ExportPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    wins = None if windows is None else (abi.ExportWindow * len(windows))(*windows)
    st = libhm_amd.lib().hmgpu_export_yuvpack_plan_for(C.byref(seq), None if desc is None else C.byref(desc), None if tensor is None else C.byref(tensor),
                                                       1 if windows is None else len(windows), wins, None if fmt is None else C.byref(fmt),
                                                       None if pack is None else C.byref(pack), C.byref(plan))
    assert st == want, "status %d, expected %d" % (st, want)
    if want != OK:
        assert bytes(plan) == bytes(C.sizeof(plan)), "a refused plan must be all zero"
    return plan


def _cf(fmt, **kw):
    return abi.make_export_format(yref.CHROMA[fmt], **kw)


def _win(seq, x, y, w, h, flip=False):
    return abi.make_export_window((x, seq.width - x - w, y, seq.height - y - h), flip)


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_plans(fmt):
    for src in (0, 1, 2, 3):
        seq = _seq(src)
        for w in (2, 46, 48, 50, 70, 72):
            plan = _status(seq, _desc(fmt, crop=(0, seq.width - w, 0, 2)), _cf(fmt), abi.make_export_yuvpack(fmt))
            assert (plan.planes, plan.width[0], plan.height[0], plan.row_bytes[0]) == (1, w, 38, yref.row_bytes(fmt, w)), (src, w)
            assert list(plan.width[1:]) == list(plan.height[1:]) == list(plan.row_bytes[1:]) == [0, 0] and list(plan.coef) == [0] * 16
            plan = _status(seq, _desc(fmt), _cf(fmt), abi.make_export_yuvpack(fmt), windows=[_win(seq, min(2, 72 - w), 6, w, 26), _win(seq, min(6, 72 - w), 2, w, 26, True)])
            assert (plan.planes, plan.width[0], plan.height[0], plan.row_bytes[0]) == (1, w, 26, yref.row_bytes(fmt, w))
    # the descriptor's zeros: the depth and the container of the format
    _status(_seq(), _desc(fmt, bd=(0, 0), nbytes=0), _cf(fmt), abi.make_export_yuvpack(fmt))


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_each_refusal(fmt):
    seq, d, f, p = _seq(), _desc(fmt), _cf(fmt), abi.make_export_yuvpack(fmt)
    D = yref.DEPTH[fmt]
    _status(seq, d, f, p)
    # 1. pack
    _status(seq, d, f, None, want=EINVAL)
    bad = abi.make_export_yuvpack(fmt)
    bad.reserved[5] = 1
    _status(seq, d, f, bad, want=EINVAL)
    for code in (-1, 8, 100):
        _status(seq, d, f, abi.make_export_yuvpack(code), want=EUNSUPPORTED)
    # 2. the descriptor
    _status(seq, None, f, p, want=EINVAL)
    _status(seq, _desc(fmt, layout=abi.EXPORT_SEMIPLANAR), f, p, want=EINVAL)
    _status(seq, _desc(fmt, layout=abi.EXPORT_RGB), f, p, want=EINVAL)
    other = 10 if D != 10 else 8
    for bd in ((other, D), (D, other), (D + 1 if D < 16 else 12, D), (9, 9)):
        _status(seq, _desc(fmt, bd=bd), f, p, want=EINVAL)
    _status(seq, _desc(fmt, nbytes=2 if D <= 8 else 1), f, p, want=EINVAL)
    if D > 8:
        _status(seq, _desc(fmt, msb=1), f, p, want=EINVAL)
    # 3. format
    _status(seq, d, None, p, want=EINVAL)
    for cf in range(4):
        if cf != yref.CHROMA[fmt]:
            _status(seq, d, abi.make_export_format(cf), p, want=EINVAL)
    # 4. alpha
    amax = yref.ALPHA_MAX[fmt]
    for alpha, ok in ((-1, False), (amax + 1, False), (amax, True), (1, amax >= 1)):
        _status(seq, d, f, abi.make_export_yuvpack(fmt, alpha), want=OK if ok else EINVAL)
    # 5. float elements (no plan function takes a scale: the context's calls refuse it, tests/test_gpu_export_yuvpack.py)
    for st in (abi.SAMPLE_F16, abi.SAMPLE_BF16, abi.SAMPLE_F32):
        _status(seq, d, f, p, tensor=abi.make_export_tensor(st), want=EUNSUPPORTED)
    _status(seq, d, f, p, tensor=abi.make_export_tensor(abi.SAMPLE_UINT))
    _status(seq, d, f, p, tensor=abi.make_export_tensor(7), want=EINVAL)                    # (6: the format export's own rule)
    # 6. the format export's rules: reserved words, loc, filters, whole chroma samples, windows of one size
    r = _cf(fmt)
    r.reserved[0] = 1
    _status(seq, d, r, p, want=EINVAL)
    _status(seq, d, _cf(fmt, loc=6), p, want=EINVAL)
    _status(seq, d, _cf(fmt, up=2), p, want=EUNSUPPORTED)
    _status(seq, d, _cf(fmt, down=2), p, want=EUNSUPPORTED)
    _status(seq, _desc(fmt, crop=(0, 0, 1, 1)), f, p, want=EINVAL)                          # the 4:2:0 source's rows
    odd = _seq(3)                                                                           # a 4:4:4 source allows odd edges ...
    for crop in ((1, 1, 0, 0), (0, 1, 0, 0), (1, 0, 0, 0)):
        _status(odd, _desc(fmt, crop=crop), f, p, want=OK if yref.CHROMA[fmt] == 3 else EINVAL)     # ... the 4:2:2 words do not
    _status(odd, d, f, p, windows=[_win(odd, 1, 0, 46, 26)], want=OK if yref.CHROMA[fmt] == 3 else EINVAL)
    _status(odd, d, f, p, windows=[_win(odd, 2, 0, 45, 26)], want=OK if yref.CHROMA[fmt] == 3 else EINVAL)
    _status(seq, d, f, p, windows=[_win(seq, 2, 2, 46, 26), _win(seq, 2, 2, 48, 26)], want=EINVAL)
    _status(seq, _desc(fmt, crop=(2, 0, 0, 0)), f, p, windows=[_win(seq, 2, 2, 46, 26)], want=EINVAL)
    w = _win(seq, 2, 2, 46, 26)
    w.flip = 2
    _status(seq, d, f, p, windows=[w], want=EINVAL)


def test_the_stated_order():
    """one fault of each status in one call: refused for the rule the header puts first"""
    seq = _seq()
    d, f = _desc("uyvy"), _cf("uyvy")
    rgb = _desc("uyvy", layout=abi.EXPORT_RGB)
    # 1 before 2: an unknown format (EUNSUPPORTED) with the RGB layout (EINVAL)
    _status(seq, rgb, f, abi.make_export_yuvpack(9), want=EUNSUPPORTED)
    # ... but a reserved word of `pack` (EINVAL) stands in front of its format
    bad = abi.make_export_yuvpack(9)
    bad.reserved[0] = 1
    _status(seq, d, f, bad, want=EINVAL)
    # 2, 3, 4 before 5: a float tensor (EUNSUPPORTED) with the RGB layout, the wrong chroma format or an alpha (EINVAL)
    fl = abi.make_export_tensor(abi.SAMPLE_F32)
    _status(seq, rgb, f, abi.make_export_yuvpack("uyvy"), tensor=fl, want=EINVAL)
    _status(seq, d, abi.make_export_format(3), abi.make_export_yuvpack("uyvy"), tensor=fl, want=EINVAL)
    _status(seq, d, f, abi.make_export_yuvpack("uyvy", 1), tensor=fl, want=EINVAL)
    # 5 before 6: a float tensor (EUNSUPPORTED) with an odd crop (EINVAL)
    _status(seq, _desc("uyvy", crop=(1, 1, 0, 0)), f, abi.make_export_yuvpack("uyvy"), tensor=fl, want=EUNSUPPORTED)
    # inside 6 the format export's order: loc (EINVAL, its rule 3) before an unknown filter (EUNSUPPORTED, its rule 4)
    _status(seq, d, _cf("uyvy", up=2, loc=6), abi.make_export_yuvpack("uyvy"), want=EINVAL)
    _status(seq, _desc("uyvy", crop=(2, 0, 1, 1)), _cf("uyvy", up=2), abi.make_export_yuvpack("uyvy"), want=EINVAL)   # (its rule 1: the source's rows)


def test_python_keywords():
    from libhm_amd import export as hexport
    with pytest.raises(ValueError):
        abi.yuvpack_code("nv12")
    code, st = hexport.yuvpack_stages("V210", None, None, "linear", "linear", 2)
    assert code == abi.YUVPACK_V210 and st.yuvpack.alpha == 0 and (st.format.chroma_format, st.format.up, st.format.down, st.format.loc) == (2, 1, 1, 2)
    assert st.scale is None and st.tensor is None and st.pixel is None


# ------------------------------------------------------------------------------------------------ the import's struct, plans and refusals
def test_import_struct_matches_the_header(tmp_path):
    src = tmp_path / "ip.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu\\n",'
                   'sizeof(hmgpu_import_yuvpack),offsetof(hmgpu_import_yuvpack,format),offsetof(hmgpu_import_yuvpack,reserved));return 0;}\n')
    exe = tmp_path / "ip"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P = abi.ImportYuvPack
    assert got == [C.sizeof(P), P.format.offset, P.reserved.offset] and C.sizeof(P) == 32
    p = abi.make_import_yuvpack("v210")
    assert (p.format, list(p.reserved)) == (4, [0] * 7)


def _idesc(fmt, w=0, h=0, **kw):
    d = yref.DEPTH[fmt]
    desc = abi.make_import_desc(abi.EXPORT_PLANAR, -1, (w, h), (d, d), 1 if d <= 8 else 2, 0, abi.SAMPLE_UINT, chroma_format=yref.CHROMA[fmt])
    for k, v in kw.items():
        if k == "bit_depth":
            desc.bit_depth[0], desc.bit_depth[1] = v
        elif k == "reserved":
            desc.reserved[v] = 1
        else:
            setattr(desc, k, v)
    return desc


def _istatus(seq, desc, pack, want=OK):
    plan = abi.ImportPlan()
    C.memset(C.byref(plan), 0xFF, C.sizeof(plan))
    st = libhm_amd.lib().hmgpu_import_yuvpack_plan_for(C.byref(seq), None if desc is None else C.byref(desc), None if pack is None else C.byref(pack),
                                                       C.byref(plan))
    assert st == want, "status %d, expected %d" % (st, want)
    if want != OK:
        assert bytes(plan) == bytes(C.sizeof(plan)), "a refused plan must be all zero"
    return plan


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_import_plans(fmt):
    for pic in (0, 1, 2, 3):
        seq = _seq(pic)
        for w in (2, 46, 48, 50, 70, 72):
            plan = _istatus(seq, _idesc(fmt, w, 38), abi.make_import_yuvpack(fmt))
            assert (plan.planes, plan.width[0], plan.height[0], plan.row_bytes[0]) == (1, w, 38, yref.row_bytes(fmt, w)), (pic, w)
            assert list(plan.width[1:]) == list(plan.height[1:]) == list(plan.row_bytes[1:]) == [0, 0] and list(plan.coef) == [0] * 16
        plan = _istatus(seq, _idesc(fmt, bit_depth=(0, 0), bytes_per_sample=0), abi.make_import_yuvpack(fmt))       # the zeros: the coded size, D
        assert (plan.width[0], plan.height[0], plan.row_bytes[0]) == (72, 40, yref.row_bytes(fmt, 72))


@pytest.mark.parametrize("fmt", yref.FORMATS)
def test_each_import_refusal(fmt):
    seq, p = _seq(2, bd=10), abi.make_import_yuvpack(fmt)
    D, cf = yref.DEPTH[fmt], yref.CHROMA[fmt]
    _istatus(seq, _idesc(fmt), p)
    # 1. pack
    _istatus(seq, _idesc(fmt), None, want=EINVAL)
    bad = abi.make_import_yuvpack(fmt)
    bad.reserved[0] = 1
    _istatus(seq, _idesc(fmt), bad, want=EINVAL)
    for code in (-1, 8):
        _istatus(seq, _idesc(fmt), abi.make_import_yuvpack(code), want=EUNSUPPORTED)
    # 2. the descriptor
    _istatus(seq, None, p, want=EINVAL)
    for kw in (dict(layout=abi.EXPORT_SEMIPLANAR), dict(layout=abi.EXPORT_RGB), dict(order=0), dict(chroma_format=5 - cf), dict(chroma_format=1),
               dict(bit_depth=(D, 12)), dict(bit_depth=(9, D)), dict(bytes_per_sample=2 if D <= 8 else 1), dict(sample_type=abi.SAMPLE_F32),
               dict(sample_type=7), dict(msb_aligned=1)):
        _istatus(seq, _idesc(fmt, **kw), p, want=EINVAL)
    # 3. the planar import's own steps
    for kw in (dict(reserved=7), dict(loc=6), dict(loc=-1), dict(width=74), dict(height=42), dict(width=-2), dict(width=35)):
        _istatus(seq, _idesc(fmt, **kw), p, want=EINVAL)
    _istatus(seq, _idesc(fmt, down=2), p, want=EUNSUPPORTED)
    _istatus(_seq(1), _idesc(fmt, height=37), p, want=EINVAL)                               # whole chroma rows of a 4:2:0 picture
    # the stated order: the format (EUNSUPPORTED) before the descriptor (EINVAL); the descriptor before an unknown `down`
    _istatus(seq, _idesc(fmt, layout=abi.EXPORT_RGB), abi.make_import_yuvpack(9), want=EUNSUPPORTED)
    bad = abi.make_import_yuvpack(9)
    bad.reserved[3] = 1
    _istatus(seq, _idesc(fmt), bad, want=EINVAL)
    _istatus(seq, _idesc(fmt, down=2, order=1), p, want=EINVAL)
    _istatus(seq, _idesc(fmt, down=2, loc=6), p, want=EINVAL)                               # (the planar import's own order: 1 before 2)
