"""The census of tests/geometry_cases.py, without a GPU: every case of tests/test_gpu_geometry.py holds what its name says -- CTU counts,
partial CTUs, intra and inter CUs, a reader for every margin region, the reference handles and SAO mask words of the 64-picture contexts,
and the slab arithmetic that puts a context on the plain-address path of the motion-compensation kernels."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import geometry_cases as gc
from tests.test_gpu_filter_margins import REGIONS, margin_readers


def _parts(p):
    return int(p.intra.sum()), int((p.inside & ~p.intra).sum())


def test_case_table_covers_the_axes():
    assert len(gc.SMALL_CASES) == len(set(gc.SMALL_CASES)) == 11 * 3 * 4
    for depth in gc.DEPTHS:
        mine = [c for c in gc.SMALL_CASES if c[4:] == depth]
        assert {c[3] for c in mine} == {0, 1, 2, 3} and {c[2] for c in mine} == {4, 5, 6}, depth
    ctus = {gc.geometry(c)[0] * gc.geometry(c)[1] for c in gc.SMALL_CASES}
    assert {1, 2, 3, 5} <= ctus and max(ctus) == 20, sorted(ctus)      # 72x64 in CTUs of 16
    one = [c for c in gc.SMALL_CASES if gc.geometry(c)[:2] == (1, 1)]
    assert {c[2] for c in one} == {4, 5, 6} and any(c[:2] == (56, 56) for c in one)
    # partial CTUs with 8 valid columns / rows, alone (the picture is narrower than a CTU) and behind whole CTUs; one CTU column, one CTU row
    assert any(gc.geometry(c)[0] > 1 and gc.geometry(c)[2] == 8 for c in gc.SMALL_CASES)
    assert any(gc.geometry(c)[1] > 1 and gc.geometry(c)[3] == 8 for c in gc.SMALL_CASES)
    assert any(gc.geometry(c)[0] == 1 and gc.geometry(c)[1] > 1 for c in gc.SMALL_CASES)
    assert any(gc.geometry(c)[1] == 1 and gc.geometry(c)[0] > 1 for c in gc.SMALL_CASES)


@pytest.mark.parametrize("case", gc.SMALL_CASES, ids=gc.case_id)
def test_small_pictures_hold_intra_and_inter(case):
    w, h, log2_ctu, fmt, bd, bdc = case
    cw, ch, _, _ = gc.geometry(case)
    pics = gc.small_pictures(case)
    assert len(pics) == (4 if (w, h) == (8, 8) else 2)
    intra = inter = 0
    for label, p in pics:
        assert (p.num_ctus, p.ctus_w) == (cw * ch, cw) and int(p.inside.sum()) == w * h // 16
        assert (p.seq.chroma_format, p.seq.log2_ctu_size, p.seq.bit_depth_luma, p.seq.bit_depth_chroma) == (fmt, log2_ctu, bd, bdc)
        assert (p.slice.slice_type == abi.B_SLICE) == label.startswith("B")
        a, b = _parts(p)
        if (w, h) == (8, 8):
            assert (a, b) == ((4, 0) if "intra" in label else (0, 4)), label
        else:
            assert a > 0 and b > 0, (label, a, b)
        if label.startswith("B") and b:
            m = p.meta_np
            assert {int(v) for v in p.slice.ref_pic[0][:1]} | {int(v) for v in p.slice.ref_pic[1][:1]} == {0, 1}
            assert (w, h) == (8, 8) or (m["ref_idx1"] >= 0).any()
        intra, inter = intra + a, inter + b
    assert intra > 0 and inter > 0


@pytest.mark.parametrize("case", gc.SMALL_CASES, ids=gc.case_id)
def test_every_margin_region_has_a_reader(case):
    a, bs = gc.margin_pictures(case)
    assert set(a) == set(gc.MARGIN_VARIANTS)
    comps = 1 if case[3] == 0 else 3
    assert (a["sao"].sao_raw[:, :comps, 0] == abi.SAO_NEW).all() and (a["bypass"].sao_raw[:, :comps, 0] == abi.SAO_NEW).all()
    assert (a["no sao"].sao_raw[:, :, 0] == abi.SAO_OFF).all() and not a["no sao"].pp.sao_enabled
    byp = a["bypass"].meta_np["bypass"]
    assert byp[a["bypass"].inside].all() and "bypass" not in a["sao"].meta_np
    assert len(bs) <= 8 and (len(bs) == 8) == (case[:2] == (8, 8))
    got = gc.readers_union(bs)
    for plane in ("luma", "chroma"):
        for r in REGIONS:
            assert got[plane][r] >= 1, "%s: no PU reads the %s margin %s (%s)" % (gc.case_id(case), plane, r, got[plane])
    if case[3] in (0, 1):                                  # the two counts agree where both are defined
        for b in bs:
            assert gc.margin_readers(b) == margin_readers(b)
    assert gc.REGIONS == REGIONS


def test_random_vectors_would_not_reach_every_margin():
    """why the vectors are set: a picture of tests/test_gpu_filter_margins.py's kind at 8x8 reads one region"""
    from tests import synth
    p = synth.make_picture(8, 8, 10, seed=951, ref_handles=([0], [0]), mv_range=160, mode_probs=(0, 0, 0.25, 0.75, 0))
    got = margin_readers(p)
    assert sum(v == 0 for plane in got.values() for v in plane.values()) >= 10


@pytest.mark.parametrize("w,h,log2_ctu", gc.BATCH_SIZES)
def test_batch_pictures_differ(w, h, log2_ctu):
    ctu = 1 << log2_ctu
    ctus = ((w + ctu - 1) // ctu) * ((h + ctu - 1) // ctu)
    assert ctus == {(8, 8): 1, (72, 8): 2, (24, 40): 6}[(w, h)]
    assert {n for n in gc.BATCH_NS if 8 % n == 0} == {1, 2, 8} and {n for n in gc.BATCH_NS if 8 % n or n > 8} == {3, 5, 16}
    # the motion-compensation launch gives each of 8 / n ranges ceil(CTUs * n / 8) CTUs: more and fewer than the picture has, and none
    per = {n: (ctus + 8 // n - 1) // (8 // n) for n in (1, 2, 8)}
    assert per[8] == ctus and per[1] == (1 if ctus <= 8 else 2)
    for bi in (False, True):
        pics = gc.batch_pictures(w, h, log2_ctu, 16, bi)
        assert len({b"".join(np.asarray(v).tobytes() for v in p.meta_np.values()) + b"".join(a.tobytes() for a in p.coeffs.arrays) for p in pics}) == 16
        assert all((p.sao_raw[:, :, 0] == abi.SAO_NEW).all() for p in pics)
        if (w, h) != (8, 8):
            assert sum(p.intra.any() for p in pics) >= 6 and sum(not p.intra.any() for p in pics) >= 4


@pytest.mark.parametrize("s", gc.STRIPS, ids=gc.strip_id)
def test_strips_reach_past_the_coordinates_they_are_for(s):
    w, h, log2_ctu, fmt, bd, bdc, bi = s
    p, far = gc.strip_pictures(s)
    assert w * h <= 600000 and max(w, h) > 4096 and p.intra.any() and (p.inside & ~p.intra).any()
    assert (p.slice.slice_type == abi.B_SLICE) == bi and far.slice.slice_type == abi.B_SLICE
    assert max(p.px.max(), p.py.max()) // 4 >= (2048 if max(w, h) > 8192 else 1024)
    assert (p.ctus_w, p.num_ctus) == {8200: (129 if log2_ctu == 6 else 257, 129 if log2_ctu == 6 else 257 * 3), 64: (1, 69), 16392: (1025, 1025), 8: (1, 513)}[w]
    got = margin_readers(far) if fmt == 1 else gc.margin_readers(far)
    sides = ("above", "below") if w > h else ("left", "right")
    for plane in ("luma", "chroma"):
        for r in sides:
            assert got[plane][r] >= 8, (plane, r, got[plane])


@pytest.mark.parametrize("w,h,log2_ctu,bd", gc.DPB_CONTEXTS)
def test_dpb_pictures_name_handles_on_both_sides_of_32(w, h, log2_ctu, bd):
    dec, pics = gc.dpb_pictures(w, h, log2_ctu, bd)
    lo, hi = gc.dpb_sao_masks()
    assert (lo, hi) == (1 << 31, (1 << 1) | (1 << 31))
    every = set(gc.DPB_UPLOADED) | set(dec)
    assert every == {0, 31, 32, 33, 62, 63}
    for word, base in ((lo, 0), (hi, 32)):                  # each word carries set and clear bits among the handles in use
        mine = [hnd - base for hnd in every if base <= hnd < base + 32]
        assert any(word >> b & 1 for b in mine) and any(not (word >> b & 1) for b in mine)
    # bit b of the other word differs for at least one handle: taking the wrong word shows
    assert any((lo >> (hnd & 31) & 1) != (hi >> (hnd & 31) & 1) for hnd in every)
    used = set()
    for label, p in pics:
        m, sl = p.meta_np, p.slice
        for l in range(2):
            for r in np.unique(m["ref_idx%d" % l][m["ref_idx%d" % l] >= 0]):
                used.add(int(sl.ref_pic[l][int(r)]))
        if "cells" in label:
            from tests import cu_shapes as cs
            assert cs.wants_cells(p), label
            small = p.small_pu
            assert small.any()
        if "weighted" in label:
            assert sl.weighted_pred == 1
            refs = {int(sl.ref_pic[l][r]) for l in range(2) for r in range(2)}
            assert any(hnd >= 32 for hnd in refs) and any(hnd < 32 for hnd in refs)
    assert used == every, used
    assert {p.slice.slice_type for _, p in pics} == {abi.P_SLICE, abi.B_SLICE}


def test_plain_address_geometry_is_the_smallest_past_the_limit():
    w, h, log2_ctu, bd = gc.PLAIN
    seq = abi.make_seq(w, h, bd, log2_ctu=log2_ctu, max_pictures=gc.PLAIN_PICTURES)
    assert gc.plane_set_bytes(seq) == 4416 * 2536 * 2 + 4480 * 1272 * 2 == 33795072          # pitch x rows x 2 bytes, luma and chroma
    assert gc.slab_bytes(seq) == 4325769216 >= gc.WIN_LIMIT
    # what the device test asserts from hmgpu_picture_device_region: first and last picture lie this far apart
    stride = 2 * gc.plane_set_bytes(seq)
    assert (gc.PLAIN_PICTURES - 1) * stride >= gc.WIN_LIMIT - stride
    # one CTU row or one 64-sample column less, or one picture less, stays under the limit
    for dw, dh, dn in ((-64, 0, 0), (0, -64, 0), (0, 0, -1)):
        less = abi.make_seq(w + dw, h + dh, bd, log2_ctu=log2_ctu, max_pictures=gc.PLAIN_PICTURES + dn)
        assert gc.slab_bytes(less) < gc.WIN_LIMIT, (dw, dh, dn)
    # what the comment in k_mc.hip says: 64 pictures of 3840x2160 stay on the buffer path, at 58.9 MB each
    uhd = abi.make_seq(3840, 2160, 10, log2_ctu=6, max_pictures=64)
    assert 2 * gc.plane_set_bytes(uhd) == 58873856 and gc.slab_bytes(uhd) == 3767926784 < gc.WIN_LIMIT
    # 8K: 20 pictures
    assert gc.slab_bytes(abi.make_seq(7680, 4320, 10, log2_ctu=6, max_pictures=20)) >= gc.WIN_LIMIT
    assert gc.slab_bytes(abi.make_seq(7680, 4320, 10, log2_ctu=6, max_pictures=19)) < gc.WIN_LIMIT
    # the last handle straddles 4 GiB: its reconstruction set ends below, the luma plane of its SAO set (the final planes of a picture
    # that went through SAO) holds the byte at that offset; the handle before lies wholly below
    last = gc.PLAIN_PICTURES - 1
    assert gc.straddling_handle(seq) == last
    sao_luma = last * stride + gc.plane_set_bytes(seq)
    assert sao_luma < (1 << 32) < sao_luma + gc.plane_bytes(seq)[0] and sao_luma < gc.WIN_LIMIT
    sao = gc.plain_sao_picture(size=(256, 192))          # (the pictures' options at a size the census can afford)
    assert sao.pp.sao_enabled and (sao.sao_raw[:, :, 0] != abi.SAO_OFF).any()
    pics = dict(gc.plain_pictures(size=(256, 192)))
    assert set(pics) == {"P", "B", "P weighted", "P margins"}
    used = set()
    for label, p in pics.items():
        assert (p.slice.slice_type == abi.B_SLICE) == (label == "B") and bool(p.slice.weighted_pred) == (label == "P weighted") and not p.intra.any()
        for l in range(2):
            m = p.meta_np["ref_idx%d" % l]
            used |= {int(p.slice.ref_pic[l][int(r)]) for r in np.unique(m[m >= 0])}
    assert used == {0, last - 1, last}
    got = margin_readers(pics["P margins"])
    assert all(got[plane][r] >= 1 for plane in got for r in REGIONS), got


@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_export_pictures_are_sub_ctu_and_mixed(w, h, log2_ctu):
    from tests import metrics_ref, synth
    assert w < (1 << log2_ctu) or h < (1 << log2_ctu) or (w, h, log2_ctu) == (24, 40, 4)
    for fmt in (0, 1, 3):
        pics = gc.export_pictures(w, h, log2_ctu, fmt)
        assert not pics[0].intra.any() and pics[1].intra[pics[1].inside].all()
        for p in pics:
            assert len(synth.coded_blocks(p.meta_np, fmt, log2_ctu)) > 0
        assert (pics[0].meta_np["ref_idx1"] >= 0).any() or (w, h) == (8, 8)
    # what include/hmgpu.h says of planes under 8x8: no SSIM window -- the chroma planes of an 8x8 4:2:0 picture
    if (w, h) == (8, 8):
        planes = synth.noise_planes(8, 8, 10, 1)
        rec = metrics_ref.picture(planes, planes, 1, (10, 10))
        assert rec[0]["ssim_windows"] == 1 and rec[1]["ssim_windows"] == 0 and rec[2]["ssim_windows"] == 0 and rec[1]["samples"] == 16
