"""The picture generator (tests/synth.py) in the shapes beyond 4:2:0 / 64-sample CTUs, pinned without a GPU.

The oracle is pinned to HM for 4:2:2, 4:4:4, 4:0:0 and small CTUs on HM-made metadata only.  A generator that laid, say, the 4:2:2 flags
out differently from HM would make pictures on which oracle and device agree or disagree for reasons that are nobody's bug.  So:
  1. synth.coded_blocks() -- which level blocks a picture's per-partition arrays declare coded, and where they lie -- is held against HM's
     own fixtures: every non-zero level HM wrote lies inside a listed block, every listed block holds a non-zero level (HM sets a flag only
     for a block with one), and for 4:2:0 the listed blocks are exactly what hmgpu_pack_levels (host code) packs.  The stream_* fixtures
     (HM's own dump) are all 64-sample CTUs; for 16 / 32 the arrays come from the lite_* streams (HM-encoded) through libhmdec's parser,
     which tests/test_parser_streams.py pins to HM's dump array by array and whose pictures for these streams are HM's.
  2. make_picture, which lays its levels out in code of its own, agrees with that function for every format and CTU size.
  3. oracle-only properties of generated pictures at 416x240 (partial CTUs on the lower border with 64 / 32-sample CTUs)."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import golden_util as gu
from tests import synth

FORMATS_CTUS = [(f, l) for f in (0, 1, 2, 3) for l in (4, 5, 6)]
PARSED = ["ldp_ctu32_main8_208x120", "ldp_ctu16_main10_208x120", "ldp_ctu32_mincu16_main8_224x128", "ldb_444_ctu16_main8_208x120",
          "ldb_422_ctu32_main8_208x120", "ldb_422_lossless_main8_208x120", "ldb_444_main10_208x120", "ldb_mono_rext_main8_208x120"]


def _check_layout(meta, levels, chroma_format, log2_ctu, what):
    """levels: three [num_ctus, elems] arrays.  Returns (blocks, non-zero chroma levels)"""
    n = levels[0].shape[0]
    blocks = synth.coded_blocks(meta, chroma_format, log2_ctu)
    masks = synth.block_mask(blocks, n, [a.shape[1] for a in levels])
    for c in range(3):
        outside = (levels[c] != 0) & ~masks[c]
        assert not outside.any(), "%s: %d non-zero levels of component %d outside every listed block" % (what, int(outside.sum()), c)
    for sz in np.unique(blocks[:, 3]):
        b = blocks[blocks[:, 3] == sz]
        idx = b[:, 2][:, None] + np.arange(sz * sz)[None, :]
        for c in range(3):
            s = b[:, 0] == c
            if s.any():
                empty = ~(levels[c][b[s, 1][:, None], idx[s]] != 0).any(axis=1)
                assert not empty.any(), "%s: %d listed %dx%d blocks of component %d hold no level" % (what, int(empty.sum()), sz, sz, c)
    return blocks, sum(int((levels[c] != 0).sum()) for c in (1, 2))


def _check_pack_levels(seq, meta, coeffs, blocks, what):
    import libhm_amd
    packed = libhm_amd.pack_levels(seq, meta, coeffs)
    n = abi.num_ctus(seq)
    for c in range(3):
        b = blocks[blocks[:, 0] == c]
        per_ctu = np.bincount(b[:, 1], weights=b[:, 3] * b[:, 3], minlength=n).astype(np.int64)
        assert np.array_equal(np.diff(packed.starts[c].astype(np.int64)), per_ctu), "%s: elements packed per CTU, component %d" % (what, c)


_chroma_levels = {}


@pytest.mark.parametrize("name", gu.STREAMS + gu.STREAMS_EXT)
def test_coded_block_rules_hold_on_hm_dumps(name):
    for p in gu.stream_pictures(name):
        what = "%s picture %d" % (name, p.index)
        levels = [a.reshape(p.num_ctus, -1) for a in p.coeffs.arrays]
        log2_ctu = int(np.log2(p.ctu_size))
        blocks, nz = _check_layout(p.meta_np, levels, p.chroma_format, log2_ctu, what)
        _chroma_levels[(p.chroma_format, log2_ctu)] = _chroma_levels.get((p.chroma_format, log2_ctu), 0) + nz
        if p.chroma_format == 1:
            _check_pack_levels(p.seq, p.meta, p.coeffs, blocks, what)


@pytest.mark.parametrize("name", PARSED)
def test_coded_block_rules_hold_on_hm_streams_through_the_parser(name):
    from libhm_amd import hmdec
    z = gu.load("lite_" + name)
    seen = []
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(pic):
            g = pic.geometry()
            n, parts = g["num_ctbs"], 1 << (2 * g["log2_ctb"] - 4)
            meta = {k: pic.array(a).reshape(n, parts) for k, a in (("depth", "depth"), ("part_size", "part_size"), ("tr_idx", "tr_idx"),
                                                                   ("cbf_y", "cbf0"), ("cbf_u", "cbf1"), ("cbf_v", "cbf2"))}
            levels = [pic.array("coeff%d" % c).reshape(n, -1) for c in range(3)]
            fmt = g["chroma_format"]
            assert levels[1].shape[1] == (1 << (2 * g["log2_ctb"])) >> (g["csx"] + g["csy"])
            what = "%s POC %d" % (name, pic.poc)
            blocks, nz = _check_layout(meta, levels, fmt, g["log2_ctb"], what)
            _chroma_levels[(fmt, g["log2_ctb"])] = _chroma_levels.get((fmt, g["log2_ctb"]), 0) + nz
            if fmt == 1:
                seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"])
                _check_pack_levels(seq, abi.MetaHolder(meta), abi.CoeffHolder(*levels), blocks, what)
            seen.append(pic.poc)
        d.decode_stream(z["bitstream"], on_output=on_output)
    assert seen


def test_every_format_and_ctu_size_had_chroma_levels_to_show():
    """(runs after the two tests above in file order; on its own it fills the table itself)"""
    if not _chroma_levels:
        for name in gu.STREAMS_EXT[:4] + gu.STREAMS[:1]:
            test_coded_block_rules_hold_on_hm_dumps(name)
        for name in PARSED:
            test_coded_block_rules_hold_on_hm_streams_through_the_parser(name)
    for fmt in (1, 2, 3):
        assert _chroma_levels.get((fmt, 6), 0) > 0, "no HM fixture with non-zero chroma levels for chroma format %d" % fmt
    for key in ((1, 5), (1, 4), (2, 5), (3, 4)):
        assert _chroma_levels.get(key, 0) > 0, "no HM stream with non-zero chroma levels for format %d, log2 CTU %d" % key
    assert _chroma_levels.get((0, 6), 1) == 0 or (0, 6) not in _chroma_levels          # monochrome: nothing coded in chroma


def test_444_scaling_list_stream_holds_coded_32x32_chroma_blocks():
    """lite_ldb_444_sl_main8_208x120 is there for the 32x32 chroma scaling lists, which HM copies from the 16x16 chroma lists (the list
    file has no entries for them): the stream must hold coded 32x32 Cb and Cr blocks, and its lists must tell the components apart --
    else parser, oracle and device agreeing with HM's reconstruction on it (tests/test_oracle_lite_streams.py, tests/test_gpu_decoder.py)
    would prove nothing about those lists.  (All of the stream's 32x32 chroma blocks are inter blocks: lists 4 and 5.)"""
    from libhm_amd import hmdec
    z = gu.load("lite_ldb_444_sl_main8_208x120")
    count = {1: 0, 2: 0}
    lists = []
    with hmdec.Decoder(parse_only=True) as d:
        def on_output(pic):
            g = pic.geometry()
            assert g["chroma_format"] == 3 and g["log2_ctb"] == 6
            n = g["num_ctbs"]
            meta = {k: pic.array(a).reshape(n, 256) for k, a in (("depth", "depth"), ("part_size", "part_size"), ("tr_idx", "tr_idx"),
                                                                 ("cbf_y", "cbf0"), ("cbf_u", "cbf1"), ("cbf_v", "cbf2"))}
            b = synth.coded_blocks(meta, 3, 6)
            for c in (1, 2):
                count[c] += int(((b[:, 0] == c) & (b[:, 3] == 32)).sum())
            lists.append(pic.slice_params(0)[1])
        d.decode_stream(z["bitstream"], on_output=on_output)
    assert count[1] >= 10 and count[2] >= 10, count
    for sl in lists:
        m = lambda sz, l: (tuple(sl.coef[sz][l][:]), sl.dc[sz][l])
        for l in (1, 2, 4, 5):
            assert m(3, l) == m(2, l)                                 # derived from the 16x16 list of the same id
        assert len({m(3, l) for l in range(6)}) == 6                   # and no two of the six 32x32 lists alike
        assert all(len(set(m(3, l)[0])) > 8 for l in (1, 2, 4, 5))     # none of them flat


# ------------------------------------------------------------------------------------------------ the generator against the rules
@pytest.mark.parametrize("dist", ["stress", "typical"])
@pytest.mark.parametrize("fmt,log2_ctu", FORMATS_CTUS)
def test_generated_levels_lie_where_the_rules_say(fmt, log2_ctu, dist):
    p = synth.make_picture(416, 240, 10, seed=40 + fmt + 4 * log2_ctu, bi=True, intra_frac=0.2, cbf_prob=0.6, coef_dist=dist,
                           mode_probs=(0.15, 0.25, 0.25, 0.2, 0.15), chroma_format=fmt, log2_ctu=log2_ctu, bit_depth_chroma=8, ref_handles=([0], [1]))
    ctu = 1 << log2_ctu
    assert p.num_ctus == ((416 + ctu - 1) // ctu) * ((240 + ctu - 1) // ctu) and p.meta_np["depth"].shape == (p.num_ctus, ctu * ctu // 16)
    levels = p.coeffs.arrays
    sh = 2 if fmt in (0, 1) else (1 if fmt == 2 else 0)
    assert [a.shape for a in levels] == [(p.num_ctus, ctu * ctu), (p.num_ctus, ctu * ctu >> sh), (p.num_ctus, ctu * ctu >> sh)]
    assert (p.seq.chroma_format, p.seq.log2_ctu_size, p.seq.bit_depth_luma, p.seq.bit_depth_chroma) == (fmt, log2_ctu, 10, 8)
    if dist == "stress":
        blocks, nz = _check_layout(p.meta_np, levels, fmt, log2_ctu, "format %d CTU %d" % (fmt, ctu))      # both directions: every block filled
    else:
        blocks = synth.coded_blocks(p.meta_np, fmt, log2_ctu)
        masks = synth.block_mask(blocks, p.num_ctus, [a.shape[1] for a in levels])
        nz = sum(int((levels[c] != 0).sum()) for c in (1, 2))
        for c in range(3):
            assert not ((levels[c] != 0) & ~masks[c]).any()
    assert (nz > 0) == (fmt != 0)
    if fmt == 0:
        assert not p.meta_np["cbf_u"].any() and not p.meta_np["cbf_v"].any()
    if fmt in (0, 1):
        _check_pack_levels(p.seq, p.meta, p.coeffs, blocks, "format %d CTU %d" % (fmt, ctu))
    sizes = {c: set(int(v) for v in np.unique(blocks[blocks[:, 0] == c, 3])) for c in range(3)}
    assert sizes[0] == {4, 8, 16, 32} & set(range(4, ctu + 1))
    if fmt == 3:
        assert sizes[1] == sizes[0] and sizes[2] == sizes[0]                      # twins of every luma size: 4x4 chroma, 32x32 chroma
    elif fmt:
        assert sizes[1] == {4, 8, 16} & set(range(4, ctu // 2 + 1))
    # undecoded partitions keep HM's initCU defaults and nothing is coded there
    out = ~p.inside
    assert (p.meta_np["part_size"][out] == abi.SIZE_NONE).all() and not p.meta_np["cbf_y"][out].any() and not p.meta_np["cbf_u"][out].any()
    assert out.any() == (240 % ctu != 0)


@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
def test_422_flags_follow_hm_parse_rules(log2_ctu):
    """TDecSbac::parseQtCbf: the two squares' flags at the unit's depth + 1 over the upper / lower half of the block's partitions, the
    unit's own bit their OR on all of them; a 4x8 block of an 8x8 CU split into 4x4 luma TUs: flags at depth 2 over the CU's halves, bits 0
    and 1 on the whole CU"""
    p = synth.make_picture(416, 240, 8, seed=7 + log2_ctu, intra_frac=0.3, cbf_prob=0.6, chroma_format=2, log2_ctu=log2_ctu, ref_handles=([0], [0]))
    m = p.meta_np
    parts = m["depth"].shape[1]
    z = np.arange(parts)[None, :]
    log2tu = log2_ctu - m["depth"] - m["tr_idx"]
    blk_parts = np.where(log2tu == 2, 4, 1 << (2 * np.maximum(log2tu - 2, 0)))
    first = z & ~(blk_parts - 1)
    upper_only = lower_only = both = 0
    for key in ("cbf_u", "cbf_v"):
        cbf = m[key]
        own = (cbf >> m["tr_idx"]) & 1
        sub = (cbf >> (m["tr_idx"] + 1)) & 1
        up = np.take_along_axis(sub, first, axis=1)
        lo = np.take_along_axis(sub, np.minimum(first + blk_parts // 2, parts - 1), axis=1)
        dec = p.inside
        assert np.array_equal(own[dec], (up | lo)[dec])
        lower_half = (z - first) >= blk_parts // 2
        assert np.array_equal(sub[dec], np.where(lower_half, lo, up)[dec])          # constant over each half
        assert not (cbf[dec] >> (m["tr_idx"][dec] + 2)).any()
        shared = dec & (log2tu == 2)
        assert np.array_equal((cbf[shared] & 1), (cbf[shared] >> 1) & 1)
        org = dec & (z == first)
        upper_only += int((org & (up == 1) & (lo == 0)).sum())
        lower_only += int((org & (up == 0) & (lo == 1)).sum())
        both += int((org & (up == 1) & (lo == 1)).sum())
    assert upper_only > 50 and lower_only > 50 and both > 50


def test_ctu16_amp_gives_4_and_12_wide_prediction_units():
    p = synth.make_picture(416, 240, 8, seed=3, mode_probs=(0, 0, 0.3, 0.2, 0.5), log2_ctu=4, ref_handles=([0], [0]))
    m = p.meta_np
    amp = (m["part_size"] >= abi.SIZE_2NxnU) & (m["part_size"] <= abi.SIZE_nRx2N)
    assert amp.any() and (m["depth"][amp] == 0).all() and (m["tr_idx"][amp] == 1).all()
    for ps, col in ((abi.SIZE_nLx2N, 0), (abi.SIZE_nRx2N, 3)):
        a = np.nonzero((m["part_size"][:, 0] == ps))[0]
        assert a.size
        # the narrow PU is one partition (4 samples) wide: its column has a motion vector of its own, the other three columns share one
        zx = np.array([sum(((z >> (2 * b)) & 1) << b for b in range(2)) for z in range(16)])
        for ctu in a[:20]:
            narrow = m["mv0"][ctu][zx == col]
            wide = m["mv0"][ctu][zx != col]
            assert (narrow == narrow[0]).all() and (wide == wide[0]).all()
        assert any((m["mv0"][c][zx == col][0] != m["mv0"][c][zx != col][0]).any() for c in a)
    assert not (amp & (m["pred_mode"] == abi.MODE_INTRA)).any()


def test_ccp_weights_sit_on_coded_luma_units():
    p = synth.make_picture(416, 240, 8, seed=5, intra_frac=0.3, chroma_format=3, ccp_prob=0.8, ref_handles=([0], [0]))
    m = p.meta_np
    chain = (1 << (m["tr_idx"] + 1)) - 1
    luma_coded = p.inside & ((m["cbf_y"] & chain) == chain)
    z = np.arange(256)[None, :]
    tu_first = z & ~(np.maximum(1 << (2 * (6 - m["depth"] - m["tr_idx"] - 2)), 1) - 1)
    for key in ("ccp_u", "ccp_v"):
        w = m[key]
        assert set(int(v) for v in np.unique(w)) == {-8, -4, -2, -1, 0, 1, 2, 4, 8}
        assert not w[~luma_coded].any()
        assert np.array_equal(w[p.inside], np.take_along_axis(w, tu_first, axis=1)[p.inside])           # one weight per transform unit
        intra = m["pred_mode"] == abi.MODE_INTRA
        assert not w[intra & (m["intra_dir_c"] != 36)].any() and w[intra].any()
        assert (w[luma_coded] != 0).mean() > 0.5
    assert "ccp_u" not in synth.make_picture(416, 240, 8, seed=5, chroma_format=3, ref_handles=([0], [0])).meta_np
    assert p.meta.struct.ccp_alpha[0] and p.meta.struct.ccp_alpha[1]


# ------------------------------------------------------------------------------------------------ oracle-only properties
def _planes_equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("fmt,log2_ctu", FORMATS_CTUS)
def test_oracle_properties_of_generated_pictures(oracle, fmt, log2_ctu):
    w, h, bd, bdc = 416, 240, 10, 8
    kw = dict(chroma_format=fmt, log2_ctu=log2_ctu, bit_depth_chroma=bdc, ref_handles=([0], [0]))
    ref = synth.noise_planes(w, h, bd, 31, fmt, bdc)
    start = synth.blocky_planes(w, h, bd, 32, fmt, bdc)
    assert ref[1].shape == (h >> (1 if fmt in (0, 1) else 0), w >> (0 if fmt == 3 else 1)) and ref[1].max() < 256 <= ref[0].max()
    # (1) zero motion and no coded block reproduce the reference planes (4:0:0: luma; the chroma planes stay what they were)
    p = synth.make_picture(w, h, bd, seed=21, cbf_prob=0.0, mv_range=0, **kw)
    m = dict(p.meta_np)
    m["mv0"] = np.zeros_like(m["mv0"])
    p.meta = abi.MetaHolder(m)
    rec = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, rec, [ref])
    assert np.array_equal(rec[0], ref[0])
    for c in (1, 2):
        assert np.array_equal(rec[c], start[c] if fmt == 0 else ref[c]), "component %d" % c
    # (2) deblocking disabled and SAO off leave a reconstruction unchanged
    q = synth.make_picture(w, h, bd, seed=22, bi=False, intra_frac=0.2, sao=False, num_slices=3, **kw)
    rec = [a.copy() for a in start]
    oracle.decompress_ctus(q.seq, q.slices, q.meta, q.coeffs, rec, [ref])
    assert not np.array_equal(rec[0], start[0])
    for sl in q.slices:
        sl.deblocking_disable = 1
    fin = [a.copy() for a in rec]
    oracle.loop_filter_pic(q.seq, q.slices, q.meta, q.pp, fin, 3)
    assert _planes_equal(fin, rec)
    # ... and enabled, the filter changes luma, and chroma unless the picture is monochrome
    for sl in q.slices:
        sl.deblocking_disable = 0
    oracle.loop_filter_pic(q.seq, q.slices, q.meta, q.pp, fin, 3)
    assert not np.array_equal(fin[0], rec[0])
    for c in (1, 2):
        assert np.array_equal(fin[c], rec[c]) == (fmt == 0)
    # (3) 4:0:0: reconstruction, deblocking and SAO leave the chroma planes as they were
    if fmt == 0:
        r = synth.make_picture(w, h, bd, seed=23, intra_frac=0.3, **kw)
        rec = [a.copy() for a in start]
        oracle.decompress_ctus(r.seq, r.slices, r.meta, r.coeffs, rec, [ref])
        oracle.loop_filter_pic(r.seq, r.slices, r.meta, r.pp, rec, 3)
        prm = oracle.sao_reconstruct_params(r.seq, r.pp, r.meta, r.sao_raw)
        fin = oracle.sao_process(r.seq, r.slices, r.pp, r.meta, prm, rec)
        assert not np.array_equal(fin[0], start[0])
        assert np.array_equal(fin[1], start[1]) and np.array_equal(fin[2], start[2])


@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
@pytest.mark.parametrize("bd,bdc", [(8, 8), (10, 8), (8, 10)])
def test_ccp_weights_change_the_oracle_picture(oracle, log2_ctu, bd, bdc):
    w, h = 416, 240
    p = synth.make_picture(w, h, bd, seed=9, intra_frac=0.2, cbf_prob=0.7, chroma_format=3, log2_ctu=log2_ctu, bit_depth_chroma=bdc, ccp_prob=0.8,
                           ref_handles=([0], [0]))
    ref = synth.noise_planes(w, h, bd, 31, 3, bdc)
    start = synth.blocky_planes(w, h, bd, 32, 3, bdc)
    with_w = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, with_w, [ref])
    m = dict(p.meta_np)
    m["ccp_u"], m["ccp_v"] = np.zeros_like(m["ccp_u"]), np.zeros_like(m["ccp_v"])
    without = [a.copy() for a in start]
    oracle.decompress_ctus(p.seq, p.slices, abi.MetaHolder(m), p.coeffs, without, [ref])
    assert np.array_equal(with_w[0], without[0])
    assert not np.array_equal(with_w[1], without[1]) and not np.array_equal(with_w[2], without[2])
