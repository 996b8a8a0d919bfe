"""GPU: the decoder's error concealment (hmdec_set_concealment) on HM-encoded streams with NAL units taken out: a lost slice and a
lost reference picture, copy and motion copy, one parser thread and three, one device context and two.  Undamaged pictures are HM's
own planes; concealed samples are what tests/conceal_ref.py makes of the source picture; the picture that predicts from a stand-in is
the oracle's reconstruction of the arrays the decoder parsed for it, with that reference replaced."""
import numpy as np
import pytest

from tests import conceal_ref as cr
from tests import golden_util as gu
from tests.test_conceal_cpu import burst_stream, lost_picture_stream, lost_slice_stream
from tests.test_gpu_formats_fullsize import _same

pytestmark = pytest.mark.gpu

SLICES = "lite_ldp_slices_main8_208x120"


def _decode(nals, concealment, threads=1, devices=None, keep=None):
    """{poc: planes} of every picture delivered, {poc: concealed}, errors raised on the way, (hash mismatches, concealed pictures,
    concealed CTUs); keep(picture): more to remember of a picture while it is valid ({poc: ...}, the fifth item)"""
    from libhm_amd import hmdec
    planes, concealed, errors, kept = {}, {}, [], {}
    with hmdec.Decoder(threads=threads, devices=devices, concealment=concealment) as d:
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
                        planes[p.poc] = [p.plane(c) for c in range(3)]
                        concealed[p.poc] = p.concealed
                        if keep:
                            kept[p.poc] = keep(p)
                if not new_pic:
                    break
        return planes, concealed, errors, (d.hash_mismatches, d.concealed_pictures(), d.concealed_ctus()), kept


def _hm_lite(name, poc):
    z = gu.load(name)
    return [z["poc%02d_%d" % (poc, c)] for c in range(3)]


def _slice_masks(nals, poc):
    """per slice of picture `poc` of the undamaged stream: the truth values of its CTUs (parse only)"""
    from libhm_amd import hmdec
    got = {}
    with hmdec.Decoder(parse_only=True) as d:
        d.decode_stream(b"".join(b"\x00\x00\x01" + bytes(n) for n in nals), on_output=lambda p: got.__setitem__(p.poc, p.array("slice_idx").copy()))
    idx = got[poc]
    return [idx == k for k in range(int(idx.max()) + 1)]


def _slice_behind_the_gap_is_hms(got, mask, what):
    """the third slice is decoded behind the lost one: away from the borders it shares with lost CTUs -- the loop filters reach four
    samples in, and read one more --, its samples are HM's"""
    hm = _hm_lite(SLICES, 2)
    rows, cols = np.divmod(np.flatnonzero(mask), 4)                         # 4 x 2 CTUs of 64 samples
    assert list(rows) == [1, 1] and list(cols) == [2, 3]
    for c in range(3):
        sh = 1 if c else 0
        y0, x0 = (64 + 8) >> sh, (128 + 8) >> sh
        assert np.array_equal(got[c][y0:, x0:], hm[c][y0:, x0:]), "%s: the slice behind the gap, component %d" % (what, c)
        assert got[c][y0:, x0:].size >= 48 * 72 >> (2 * sh)


@pytest.mark.parametrize("threads", [1, 3])
def test_lost_slice_is_filled_from_the_previous_picture(threads):
    damaged, nals, poc, ctus = lost_slice_stream()
    masks = _slice_masks(nals, poc)
    assert int(masks[1].sum()) == ctus
    off = _decode(damaged, None, threads)
    on = _decode(damaged, "copy", threads)
    assert not on[2] and sorted(on[0]) == [0, 1, 2] and on[1] == {0: 0, 1: 0, poc: ctus}
    assert on[3] == (0, 1, ctus)                                            # no hash mismatch: the concealed picture is not checked
    # off: nothing is counted; the damaged picture, where it comes out at all, is checked against its hash SEI as ever and fails
    assert off[3][1:] == (0, 0) and off[3][0] == int(poc in off[0]) and all(v == 0 for v in off[1].values())
    for run in (off, on):
        for q in run[0]:
            if q != poc:
                _same(run[0][q], _hm_lite(SLICES, q), "threads %d, POC %d" % (threads, q))
    got = on[0][poc]
    # the lost CTUs: the co-located samples of the previous picture; every other sample as it was delivered
    _same(cr.conceal(got, on[0][poc - 1], masks[1], cr.COPY, 6, 1, (8, 8)), got, "threads %d: the lost CTUs" % threads)
    assert not np.array_equal(cr.conceal(got, _hm_lite(SLICES, poc), masks[1], cr.COPY, 6, 1, (8, 8))[0], got[0])
    _slice_behind_the_gap_is_hms(got, masks[2], "threads %d" % threads)
    if poc in off[0]:
        # (without concealment the slice behind the gap is refused: the first slice is what both runs delivered)
        a = cr.conceal(got, off[0][poc], masks[0], cr.COPY, 6, 1, (8, 8))
        _same(a, got, "threads %d: the delivered CTUs with and without concealment" % threads)


def test_lost_slice_is_the_same_with_one_parser_thread_and_three():
    damaged = lost_slice_stream()[0]
    a, b = _decode(damaged, "copy", 1), _decode(damaged, "copy", 3)
    assert sorted(a[0]) == sorted(b[0]) and a[1] == b[1] and a[3] == b[3]
    for q in a[0]:
        _same(a[0][q], b[0][q], "POC %d, one parser thread and three" % q)


def test_lost_slice_motion_copy():
    """the lost CTUs are the motion model's, fed from the arrays of the previous picture as the decoder's parser left them"""
    from tests import motion_ref
    damaged, nals, poc, ctus = lost_slice_stream()
    masks = _slice_masks(nals, poc)

    def keep(p):
        m = {n: p.array(n) for n in ("depth", "part_size", "pred_mode", "qp", "mv0", "mv1", "ref_idx0", "ref_idx1", "slice_idx")}
        return m, [p.slice_params(i)[0] for i in range(p.num_slices())]
    planes, concealed, errors, totals, kept = _decode(damaged, "motion", keep=keep)
    assert not errors and concealed == {0: 0, 1: 0, poc: ctus} and totals == (0, 1, ctus)
    meta, slices = kept[poc - 1]
    n = masks[1].size
    meta = {k: (v.reshape(n, -1) if k != "slice_idx" else v) for k, v in meta.items()}
    grid = motion_ref.grid(meta, slices, 208, 120, 6)
    assert grid["used"][0].any()
    dx, dy = cr.displacements(grid, 208, 120, poc - 1, poc)
    assert dx.any() or dy.any()                                             # (the model moves something: this is not the COPY test again)
    got = planes[poc]
    want = cr.conceal(got, planes[poc - 1], masks[1], cr.MOTION, 6, 1, (8, 8), dst_poc=poc, src_poc=poc - 1, grid=grid)
    _same(got, want, "motion copy of the lost CTUs")


def _keep_parsed(p):
    """what the oracle needs of a picture, as the decoder's parser left it (tests/test_oracle_lite_streams.py).  Of a parse-only
    decoder: the levels of a picture on its way to the device may be in the compact layout, which the oracle does not read"""
    from tests.test_oracle_lite_streams import FROM_PARSER
    g = p.geometry()
    return dict(geom=g, arrays={k: p.array(v) for k, v in FROM_PARSER.items()}, coeff=[p.array("coeff%d" % c) for c in range(3)],
                sao=p.array("sao").reshape(g["num_ctbs"], 3, 35), slices=[p.slice_params(i) for i in range(p.num_slices())])


def _oracle_of_parsed(oracle, k, refs_by_poc):
    """the oracle's finished planes of a picture kept by _keep_parsed, its references by POC"""
    import ctypes as C
    from libhm_amd import abi
    g = k["geom"]
    seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], max_pictures=8,
                       strong_intra_smoothing=g["strong_intra"], range_ext_flags=g["range_ext"])
    seq.chroma_format = g["chroma_format"]
    parts = len(k["arrays"]["depth"]) // g["num_ctbs"]
    m = {kk: (v.reshape(g["num_ctbs"], parts, 2) if kk.startswith("mv") else v.reshape(g["num_ctbs"], -1) if v.size != g["num_ctbs"] else v)
         for kk, v in k["arrays"].items()}
    meta, coeffs = abi.MetaHolder(m), abi.CoeffHolder(*k["coeff"])
    pocs = sorted(refs_by_poc)
    slices, keep = [], []
    for sp, lists in k["slices"]:
        for l in range(2):
            for i in range(sp.num_ref_idx[l]):
                sp.ref_pic[l][i] = pocs.index(sp.ref_poc[l][i])             # the oracle indexes its reference list by handle
        if sp.scaling_lists:
            keep.append(lists)
            sp.scaling_lists = C.pointer(lists)
        slices.append(sp)
    pp = abi.make_pic_params(sao_enabled=g["sao"], lf_across_tiles=g["lf_across_tiles"], sao_offset_shift=g["sao_shift"])
    cur = [np.full((g["height"] >> (g["csy"] if c else 0), g["width"] >> (g["csx"] if c else 0)), -1, dtype=np.int16) for c in range(3)]
    oracle.decompress_ctus(seq, slices, meta, coeffs, cur, [refs_by_poc[q] for q in pocs])
    oracle.loop_filter_pic(seq, slices, meta, pp, cur, 3)
    if g["sao"]:
        cur = oracle.sao_process(seq, slices, pp, meta, oracle.sao_reconstruct_params(seq, pp, meta, k["sao"]), cur)
    return m, cur


def _parsed(nals):
    """{poc: _keep_parsed} of a parse-only decoder with concealment on: the same parser, HM's dense level layout"""
    from libhm_amd import hmdec
    kept = {}
    with hmdec.Decoder(parse_only=True, concealment="copy") as d:
        d.decode_stream(b"".join(b"\x00\x00\x01" + bytes(n) for n in nals), on_output=lambda p: kept.__setitem__(p.poc, _keep_parsed(p)))
    return kept


def _keep_vectors(p):
    return {n: p.array(n) for n in ("mv0", "mv1", "ref_idx0", "ref_idx1", "part_size", "pred_mode")}


def _lost_picture_checks(oracle, run, what, parsed, whole):
    """POC 2 is the oracle's reconstruction of POC 2 with POC 1 replaced by the stand-in -- of the arrays this decoder's parser made of
    POC 2, not of the fixture's HM arrays: temporal motion vector prediction finds nothing in a stand-in (as in HM behind
    xCreateLostPicture), so the vectors of the pictures that take candidates from it are other vectors than those of the undamaged
    stream.  The test asserts that they differ, and holds the device path to the oracle on the arrays that were decoded."""
    from libhm_amd import abi
    planes, concealed, errors, totals, kept = run
    pics = gu.stream_pictures("ldp_main8_416x240")
    assert not errors and sorted(planes) == [0, 1, 2], (what, errors)
    assert concealed == {0: 0, 1: pics[1].num_ctus, 2: 0} and totals[1:] == (1, pics[1].num_ctus)
    _same(planes[0], pics[0].fin, what + ": POC 0 is HM's")
    _same(planes[1], planes[0], what + ": the stand-in is the picture before it")
    for name, a in kept[2].items():                                         # the device run parsed what the parse-only run parsed
        assert np.array_equal(a, parsed[2]["arrays"][name]), (what, name)
    m, want = _oracle_of_parsed(oracle, parsed[2], {0: planes[0], 1: planes[1]})
    _same(planes[2], want, what + ": POC 2 predicts from the stand-in")
    # everything of POC 2 that cannot depend on temporal candidates is what HM's parser left for the undamaged stream
    for name in ("depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf_y", "cbf_u", "cbf_v", "ts_y", "ts_u", "ts_v", "ref_idx0", "ref_idx1",
                 "intra_dir_l", "intra_dir_c", "bypass", "ipcm", "slice_idx"):
        a, b = m[name].astype(np.int64), np.asarray(pics[2].meta_np[name]).astype(np.int64).reshape(m[name].shape)
        if name in ("depth", "qp"):                                          # (partitions outside the picture: HM's dump and the parser differ)
            a, b = a[m["part_size"] != abi.SIZE_NONE], b[m["part_size"] != abi.SIZE_NONE]
        assert np.array_equal(a, b), name
    for c in range(3):
        assert np.array_equal(parsed[2]["coeff"][c], np.asarray(pics[2].coeffs.arrays[c]).reshape(-1)), "levels of component %d" % c
    # (SAO: the unused offsets differ between HM's dump and the parser; the parser's own of the undamaged stream is held to HM elsewhere)
    assert np.array_equal(parsed[2]["sao"], whole[2]["sao"]) and np.array_equal(parsed[2]["sao"][..., 0], pics[2].sao_raw[..., 0])
    assert not np.array_equal(m["mv0"], np.asarray(pics[2].meta_np["mv0"]).reshape(m["mv0"].shape))
    assert not np.array_equal(planes[2][0], pics[2].fin[0])
    # POC 2 is not concealed and predicts from a concealed picture: the one picture whose hash SEI disagrees
    assert totals[0] == 1, (what, totals)


@pytest.mark.parametrize("threads", [1, 3])
def test_lost_picture_gets_a_stand_in(oracle, threads):
    damaged, nals = lost_picture_stream()
    a = _decode(damaged, "copy", threads, keep=_keep_vectors)
    _lost_picture_checks(oracle, a, "threads %d" % threads, _parsed(damaged), _parsed(nals))
    b = _decode(damaged, "copy", threads)
    for q in a[0]:
        _same(a[0][q], b[0][q], "threads %d, POC %d: two runs" % (threads, q))
    off = _decode(damaged, None, threads)
    assert sorted(off[0]) == [0] and off[2] and off[3] == (0, 0, 0)


def test_lost_picture_with_two_device_contexts(oracle, monkeypatch):
    """two contexts on one GPU: the stand-in is made in the context that holds its source, and the picture that predicts from it
    finds it there or has it copied"""
    # (every picture moves on to the next context, as in tests/test_gpu_decoder.py: the decoder reads the switch once per process)
    monkeypatch.setenv("HMDEC_PLACE_ROUND_ROBIN", "1")
    damaged, nals = lost_picture_stream()
    _lost_picture_checks(oracle, _decode(damaged, "copy", 1, devices=[0, 0], keep=_keep_vectors), "two contexts", _parsed(damaged), _parsed(nals))
    whole = _decode(nals, "copy", 1, devices=[0, 0])
    assert whole[3] == (0, 0, 0) and not whole[2]
    for p in gu.stream_pictures("ldp_main8_416x240"):
        _same(whole[0][p.poc], p.fin, "undamaged stream, two contexts, POC %d" % p.poc)


def test_stand_in_in_a_reused_buffer_is_copied_not_moved():
    """burst loss with motion copy: the stream once whole, then again with its second picture lost and a slice of its third.  The
    stand-in of the second pass sits in a buffer -- a device handle -- in which the first pass decoded a P picture, whose motion arrays
    are still resident there; it is the closest picture to the lost slice and has no motion of its own, so the lost CTUs are its
    co-located samples, whatever the handle held before"""
    nals = lost_slice_stream()[1]
    masks = _slice_masks(nals, 2)
    planes, concealed, errors, totals, _ = _decode(burst_stream(), "motion")
    assert not errors and concealed == {0: 0, 1: 8, 2: 3} and totals[1:] == (2, 11)         # (the second pass; the first concealed nothing)
    _same(planes[0], _hm_lite(SLICES, 0), "POC 0 of the second pass")
    _same(planes[1], planes[0], "the stand-in is the picture before it")
    got = planes[2]
    _same(cr.conceal(got, planes[1], masks[1], cr.COPY, 6, 1, (8, 8)), got, "the lost CTUs are the stand-in's co-located samples")
    a, b = _decode(burst_stream(), "copy"), _decode(burst_stream(), "motion", threads=3)
    for q in planes:
        _same(a[0][q], planes[q], "POC %d: copy and motion copy" % q)
        _same(b[0][q], planes[q], "POC %d: one parser thread and three" % q)


def test_lost_slice_with_two_device_contexts(monkeypatch):
    """the incomplete picture is filled in the context it was decoded in, from the closest picture whose samples that context holds:
    with every picture moving on to the next context, the previous picture is there as a transferred reference -- samples without
    motion arrays, so motion copy copies"""
    monkeypatch.setenv("HMDEC_PLACE_ROUND_ROBIN", "1")
    damaged, nals, poc, ctus = lost_slice_stream()
    masks = _slice_masks(nals, poc)
    one = _decode(damaged, "copy", 1)
    for mode in ("copy", "motion"):
        planes, concealed, errors, totals, _ = _decode(damaged, mode, 1, devices=[0, 0])
        assert not errors and concealed == {0: 0, 1: 0, poc: ctus} and totals == (0, 1, ctus)
        for q in planes:
            _same(planes[q], one[0][q], "%s, two contexts, POC %d: as with one context" % (mode, q))
        got = planes[poc]
        _same(cr.conceal(got, planes[poc - 1], masks[1], cr.COPY, 6, 1, (8, 8)), got, "%s, two contexts: the lost CTUs" % mode)
