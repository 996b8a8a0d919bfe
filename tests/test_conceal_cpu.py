"""Error concealment without a GPU: the arithmetic of tests/conceal_ref.py (the model the GPU tests compare with), the ctypes mirror
of hmgpu_conceal_job against the header, and the decoder's concealment logic in parse-only mode (which keeps the books of the device
path without its calls).  hmgpu_create needs a GPU, so the refusals of hmgpu_conceal_check are in tests/test_gpu_conceal.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from libhm_amd import abi
from tests import conceal_ref as cr
from tests import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scaling_rule_against_brute_force():
    """H.265 8.5.3.2.7 as the header states it, against the formulas written out from td and tb: every POC distance pair around
    the clipping points and vectors at the ends of the range"""
    for td in range(-130, 131):
        for tb in range(-130, 131):
            ctd, ctb = max(-128, min(127, td)), max(-128, min(127, tb))
            for mv in (-32768, -515, -1, 0, 1, 2, 513, 32767):
                # src_poc - ref_poc = td, dst_poc - src_poc = tb
                assert cr.scale_mv(mv, td, 0, td + tb) == cr.scale_mv_spec(mv, ctd, ctb), (td, tb, mv)
    assert cr.scale_mv(513, 4, 0, 8) == 513 and cr.scale_mv(513, 4, 0, 12) == 1026 and cr.scale_mv(513, 4, 0, 0) == -513
    assert cr.scale_mv(100, 7, 7, 9) == 0                                   # td == 0
    assert cr.scale_mv(32767, 1, 0, 128) == 32767 and cr.scale_mv(-32768, 1, 0, 128) == -32768


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_model_never_reads_outside_a_plane(fmt):
    """vectors of +-32767 quarter samples in every block, in all four directions: every coordinate the model reads lies in the plane,
    and the block at each corner reads the corner sample"""
    w, h, lc = 40, 24, 4
    rng = np.random.RandomState(fmt)
    src = [rng.randint(0, 256, size=s).astype(np.int16) for s in ((h, w),) + ((h >> cr.chroma_shifts(fmt)[1], w >> cr.chroma_shifts(fmt)[0]),) * 2]
    dst = [np.zeros_like(p) for p in src]
    for vx, vy in ((32767, 32767), (-32767, 32767), (32767, -32767), (-32767, -32767), (32767, 0), (0, -32767)):
        grid = dict(used=np.zeros((2, h // 4, w // 4), bool), mv=np.zeros((2, 2, h // 4, w // 4), np.int64), ref_poc=np.zeros((2, h // 4, w // 4), np.int64))
        grid["used"][1] = True                                              # list 1 where list 0 is not used
        grid["mv"][1, 0], grid["mv"][1, 1] = vx, vy
        reads = []
        out = cr.conceal(dst, src, None, cr.MOTION, lc, fmt, (8, 8), dst_poc=2, src_poc=1, grid=grid, reads=reads)
        assert reads
        for c, y, x in reads:
            assert 0 <= y < src[c].shape[0] and 0 <= x < src[c].shape[1]
        for c in ([0] if fmt == 0 else [0, 1, 2]):
            hc, wc = src[c].shape
            want = src[c][(hc - 1 if vy > 0 else 0) if vy else slice(None), (wc - 1 if vx > 0 else 0) if vx else slice(None)]
            if vx and vy:
                assert (out[c] == want).all()
            elif vx:
                assert (out[c] == np.asarray(want)[:, None]).all()
            else:
                assert (out[c] == np.asarray(want)[None, :]).all()
        if fmt == 0:
            assert not out[1].any() and not out[2].any()                    # 4:0:0: the chroma planes are not written


def test_model_masks_fill_and_partial_ctus():
    w, h, lc = 72, 40, 6                                                    # 2 x 1 CTUs, both partial
    src = [np.full((h, w), 7, np.int16), np.full((h // 2, w // 2), 8, np.int16), np.full((h // 2, w // 2), 9, np.int16)]
    dst = [np.zeros_like(p) for p in src]
    out = cr.conceal(dst, src, [False, True], cr.COPY, lc, 1, (8, 8))
    assert (out[0][:, :64] == 0).all() and (out[0][:, 64:] == 7).all() and (out[1][:, :32] == 0).all() and (out[2][:, 32:] == 9).all()
    out = cr.conceal(dst, None, np.array([1], np.uint8), cr.COPY, lc, 1, (10, 8), fill=(-1, 3, -1))
    assert (out[0][:, :64] == 512).all() and (out[0][:, 64:] == 0).all() and (out[1][:, :32] == 3).all() and (out[2][:, :32] == 128).all()


def test_conceal_job_mirror_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %d %d\\n",'
                   'sizeof(hmgpu_conceal_job),offsetof(hmgpu_conceal_job,fill),offsetof(hmgpu_conceal_job,ctu_mask),'
                   'offsetof(hmgpu_conceal_job,reserved),HMGPU_CONCEAL_COPY,HMGPU_CONCEAL_MOTION);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    J = abi.ConcealJob
    assert got == [C.sizeof(J), J.fill.offset, J.ctu_mask.offset, J.reserved.offset, abi.CONCEAL_COPY, abi.CONCEAL_MOTION]
    arr, keep = abi.conceal_job_array([dict(dst=3, mode="motion", dst_poc=5, src_poc=-7, fill=(1, 2, 3), mask=[True, False, True]),
                                       dict(dst=1, src=2)], 3)
    assert (arr[0].dst, arr[0].src, arr[0].mode, arr[0].dst_poc, arr[0].src_poc, list(arr[0].fill)) == (3, abi.NO_PIC, 1, 5, -7, [1, 2, 3])
    assert keep[0].tolist() == [5] and arr[0].ctu_mask == keep[0].ctypes.data
    assert (arr[1].src, arr[1].mode, list(arr[1].fill), arr[1].ctu_mask) == (2, 0, [-1, -1, -1], None)


# ------------------------------------------------------------------------------------------------ the decoder, parse only
def _nal_type(nal):
    return (nal[0] >> 1) & 0x3f


def _is_slice(nal):
    return _nal_type(nal) <= 21


def _run(nals, concealment):
    """(poc, concealed) of every picture delivered, the errors raised on the way, and the decoder's totals"""
    from libhm_amd import hmdec
    out, errors = [], []
    with hmdec.Decoder(parse_only=True, concealment=concealment) as d:
        for i, nal in enumerate(nals):
            while True:
                try:
                    new_pic, check = d.push(nal, i == len(nals) - 1)
                except RuntimeError as e:
                    errors.append(str(e))
                    break
                if check:
                    while True:
                        p = d.get_picture()
                        if p is None:
                            break
                        out.append((p.poc, p.concealed))
                if not new_pic:
                    break
        return out, errors, d.concealed_pictures(), d.concealed_ctus(), d.hash_mismatches


def _arrays(nals, concealment, poc, names):
    """the named parser arrays of picture `poc` (parse only)"""
    from libhm_amd import hmdec
    got = {}
    with hmdec.Decoder(parse_only=True, concealment=concealment) as d:
        def on_output(p):
            if p.poc == poc:
                got.update({n: p.array(n) for n in names})
        d.decode_stream(b"".join(b"\x00\x00\x01" + bytes(n) for n in nals), on_output=on_output)
    return got


def lost_slice_stream():
    """lite_ldp_slices_main8_208x120 without the second slice segment of its last picture; (NAL units, all NAL units, the POC of the
    damaged picture, the CTUs of the lost slice)"""
    from libhm_amd import hmdec
    z = gu.load("lite_ldp_slices_main8_208x120")
    nals = hmdec.split_nal_units(z["bitstream"])
    firsts = [k for k, n in enumerate(nals) if _is_slice(n) and n[2] & 0x80]
    segs = [k for k in range(firsts[-1], len(nals)) if _is_slice(nals[k])]
    assert len(segs) == 3
    return [n for k, n in enumerate(nals) if k != segs[1]], nals, len(firsts) - 1, 3


def lost_picture_stream(k=1):
    """stream_ldp_main8_416x240 without any NAL unit of its picture k (decoding order; a TRAIL_R picture the next one predicts from)"""
    from libhm_amd import hmdec
    z = gu.load("stream_ldp_main8_416x240")
    nals = hmdec.split_nal_units(z["bitstream"])
    firsts = [i for i, n in enumerate(nals) if _is_slice(n) and n[2] & 0x80]
    assert _nal_type(nals[firsts[k]]) == 1                                  # TRAIL_R: referenced, not an IRAP picture
    return [n for i, n in enumerate(nals) if not firsts[k] <= i < firsts[k + 1]], nals


def burst_stream():
    """lite_ldp_slices_main8_208x120 whole, then once more without its second picture and without the second slice segment of its
    third: the stand-in of the second pass lands in a buffer an earlier picture has used, and is the closest picture to the lost slice"""
    from libhm_amd import hmdec
    nals = hmdec.split_nal_units(gu.load("lite_ldp_slices_main8_208x120")["bitstream"])
    firsts = [k for k, n in enumerate(nals) if _is_slice(n) and n[2] & 0x80]
    assert len(firsts) == 3
    segs = [k for k in range(firsts[2], len(nals)) if _is_slice(nals[k])]
    return nals + [n for k, n in enumerate(nals) if not firsts[1] <= k < firsts[2] and k != segs[1]]


def test_parse_only_burst_loss_in_reused_buffers():
    out, errors, pictures, total, _ = _run(burst_stream(), "motion")
    assert not errors and out == [(0, 0), (1, 0), (2, 0), (0, 0), (1, 8), (2, 3)] and (pictures, total) == (2, 11)


def test_parse_only_lost_slice():
    damaged, nals, poc, ctus = lost_slice_stream()
    whole = _run(nals, "copy")
    assert whole[1:] == ([], 0, 0, 0) and all(c == 0 for _, c in whole[0])   # nothing is lost: nothing is concealed
    out, errors, pictures, total, mismatches = _run(damaged, "copy")
    assert not errors
    assert [p for p, _ in out] == [p for p, _ in whole[0]]                  # as many pictures as the undamaged stream
    assert [c for _, c in out] == [ctus if p == poc else 0 for p, _ in out]
    assert (pictures, total, mismatches) == (1, ctus, 0)                    # (the concealed picture is not hash-checked)
    # off: today's books -- the picture comes out, nothing is counted, the slice segment behind the gap is refused
    off = _run(damaged, None)
    assert [p for p, _ in off[0]] == [p for p, _ in whole[0]] and all(c == 0 for _, c in off[0]) and off[2:4] == (0, 0)
    assert len(off[1]) == 1 and "does not continue" in off[1][0]
    assert _run(damaged, "motion")[:4] == (out, errors, pictures, total)
    # the slice behind the gap, parsed only with concealment on: its CTUs hold what they hold in the undamaged stream
    names = ("depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf0", "cbf1", "cbf2", "mv0", "mv1", "ref_idx0", "ref_idx1", "intra_dir0",
             "intra_dir1", "skip", "merge", "coeff0", "coeff1", "coeff2", "sao")
    a, b = _arrays(damaged, "copy", poc, names + ("slice_idx",)), _arrays(nals, "copy", poc, names + ("slice_idx",))
    behind = np.flatnonzero(b["slice_idx"] == 2)
    assert behind.size == 2
    for name in names:
        x, y = a[name].reshape(8, -1), b[name].reshape(8, -1)
        assert np.array_equal(x[behind], y[behind]), name
    assert (a["part_size"].reshape(8, -1)[b["slice_idx"] == 1] == abi.SIZE_NONE).all()


def test_parse_only_lost_picture():
    damaged, nals = lost_picture_stream()
    whole = _run(nals, "copy")
    out, errors, pictures, total, _ = _run(damaged, "copy")
    assert not errors and [p for p, _ in out] == [p for p, _ in whole[0]] == [0, 1, 2]
    ctbs = 7 * 4                                                            # 416x240 in 64-sample CTUs
    assert [c for _, c in out] == [0, ctbs, 0] and (pictures, total) == (1, ctbs)   # exactly one stand-in
    off = _run(damaged, None)
    assert len(off[0]) < len(out) and off[1] and "missing" in off[1][0] and off[2:4] == (0, 0)
    assert len(off[0]) != len(out)                                          # the feature makes the difference
