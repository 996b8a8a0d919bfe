"""What the intra fixtures (gu.STREAMS_INTRA: HM's encoder on the directional content of oracle/make_golden.py intra_clip) hold, counted
from HM's own parsed data: every luma mode at 16x16 and 32x32 per chroma format, every chroma mode, blocks where strong intra smoothing
decides samples at every bit depth, intra blocks with inter neighbours under constrained intra prediction.  The fixtures were made for
these counts; a regenerated fixture that no longer holds them checks less than it seems to, and fails here.  Run with -s to see the counts."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import golden_util as gu

REXT_INTRA_SMOOTHING_DISABLED = 8                # HMGPU_REXT_INTRA_SMOOTHING_DISABLED (include/hmgpu.h)
NOSMOOTH = [n for n in gu.STREAMS_INTRA if "nosmooth" in n]
CIP = [n for n in gu.STREAMS_INTRA if "cip" in n]


def fmt_of(name):
    return "444" if "_444" in name else "422" if "_422" in name else "420"


def _zscan(parts):
    z = np.arange(parts)
    x = sum(((z >> (2 * b)) & 1) << b for b in range(8))
    y = sum(((z >> (2 * b + 1)) & 1) << b for b in range(8))
    return x, y


def luma_tus(p):
    """(log2 size, mode, x, y) of every luma intra TU of a picture: log2 size = log2_ctu - depth - tr_idx, one entry per TU (its first
    4x4 partition in z-order)"""
    m = p.meta_np
    log2 = int(np.log2(p.ctu_size)) - m["depth"].astype(np.int32) - m["tr_idx"].astype(np.int32)
    zx, zy = _zscan(p.parts)
    ctu = np.arange(p.num_ctus)[:, None]
    x = (ctu % p.ctus_w) * p.ctu_size + 4 * zx[None, :]
    y = (ctu // p.ctus_w) * p.ctu_size + 4 * zy[None, :]
    first = (np.arange(p.parts)[None, :] % (1 << (2 * np.maximum(log2 - 2, 0)))) == 0
    sel = (m["pred_mode"] == abi.MODE_INTRA) & (m["part_size"] != abi.SIZE_NONE) & (m["ipcm"] == 0) & first & (x < p.width) & (y < p.height)
    return np.stack([log2[sel], m["intra_dir_l"][sel].astype(np.int32), x[sel], y[sel]], axis=1)


def modes_by_size(names):
    """{log2 size: 35 TU counts by luma mode} over all pictures of the named streams"""
    out = {s: np.zeros(35, dtype=np.int64) for s in (2, 3, 4, 5)}
    for name in names:
        for p in gu.stream_pictures(name):
            for log2, mode, _, _ in luma_tus(p):
                out[int(log2)][int(mode)] += 1
    return out


def _copy(struct, **fields):
    s = type(struct).from_buffer_copy(struct)
    for k, v in fields.items():
        setattr(s, k, v)
    return s


def _oracle_pre(oracle, pics, seq_fields=None, slice_fields=None):
    """the oracle's reconstruction of every picture (references: HM's final pictures), with fields of the sequence / slice parameters replaced"""
    finals, out = [], []
    for p in pics:
        seq = _copy(p.seq, **(seq_fields or {}))
        slices = [_copy(sl, **(slice_fields or {})) for sl in p.slices]
        cur = [np.full_like(a, -1) for a in p.pre]
        oracle.decompress_ctus(seq, slices, p.meta, p.coeffs, cur, finals)
        out.append(cur)
        finals.append(p.fin)
    return out


def _areas32(a, b):
    """number of 32x32 areas in which two planes differ"""
    d = a != b
    h, w = d.shape
    return sum(bool(d[y:y + 32, x:x + 32].any()) for y in range(0, h, 32) for x in range(0, w, 32))


def strong_smoothing_areas(oracle, name):
    """32x32 luma areas that come out differently with strong_intra_smoothing forced to 0 (an upper bound on the blocks where the tool is
    decisive: a difference spreads to the blocks predicted from it).  With the flag as the stream has it the oracle must equal HM."""
    pics = gu.stream_pictures(name)
    given = _oracle_pre(oracle, pics)
    for p, g in zip(pics, given):
        for c in range(3):
            assert np.array_equal(g[c], p.pre[c]), "%s pic %d comp %d" % (name, p.index, c)
    off = _oracle_pre(oracle, pics, seq_fields={"strong_intra_smoothing": 0})
    return sum(_areas32(g[0], o[0]) for g, o in zip(given, off))


# ---------------------------------------------------------------------------------------------------------------- luma modes
# modes that HM's RD search did not pick at a size in any fixture of a format (at most two per format and size): none
MISSING = {}


@pytest.mark.parametrize("fmt, sizes", [("420", (2, 3, 4, 5)), ("422", (4, 5)), ("444", (4, 5))])
def test_every_luma_mode_at_every_large_size(fmt, sizes):
    names = [n for n in gu.STREAMS_INTRA if fmt_of(n) == fmt]
    assert names
    counts = modes_by_size(names)
    for s in sizes:
        allowed = MISSING.get((fmt, s), [])
        assert len(allowed) <= 2
        absent = [m for m in range(35) if counts[s][m] == 0]
        print("%s %2dx%-2d: TUs per mode, least %d (mode %d), planar %d DC %d, absent %s" % (
            fmt, 1 << s, 1 << s, counts[s].min(), int(counts[s].argmin()), counts[s][0], counts[s][1], absent))
        assert absent == sorted(allowed), "%s at %dx%d: modes without a TU %s" % (fmt, 1 << s, 1 << s, absent)


@pytest.mark.parametrize("fmt", ["422", "444"])
def test_every_chroma_mode(fmt):
    """intra_dir_c as HM holds it: planar, DC, horizontal, vertical, 34 (the substitute where the luma mode is one of those four) and 36 (DM)"""
    seen = {}
    for name in gu.STREAMS_INTRA:
        if fmt_of(name) != fmt:
            continue
        for p in gu.stream_pictures(name):
            m = p.meta_np
            sel = (m["pred_mode"] == abi.MODE_INTRA) & (m["part_size"] != abi.SIZE_NONE)
            for v, n in zip(*np.unique(m["intra_dir_c"][sel], return_counts=True)):
                seen[int(v)] = seen.get(int(v), 0) + int(n)
    print("%s chroma modes (4x4 partitions): %s" % (fmt, seen))
    assert sorted(seen) == [0, 1, 10, 26, 34, 36]


# ---------------------------------------------------------------------------------------------------------------- strong smoothing
def _depth_group(name):
    p = gu.stream_pictures(name)[0]
    return "444" if fmt_of(name) == "444" else "bd%d" % p.bd_y


@pytest.mark.parametrize("group", ["bd8", "bd10", "bd12", "444"])
def test_strong_intra_smoothing_is_decisive(oracle, group):
    """per luma bit depth (threshold 1 << (bd - 5)) and for 4:4:4: at least 8 areas of 32x32 luma samples change when the flag is cleared"""
    total = 0
    for name in gu.STREAMS_INTRA:
        if name in NOSMOOTH or _depth_group(name) != group:
            continue
        n = strong_smoothing_areas(oracle, name)
        print("%s: %s, %d areas of 32x32 differ without strong intra smoothing" % (group, name, n))
        total += n
    assert total >= 8


@pytest.mark.parametrize("name", NOSMOOTH)
def test_no_smoothing_fixture(oracle, name):
    pics = gu.stream_pictures(name)
    assert all(p.seq.range_ext_flags & REXT_INTRA_SMOOTHING_DISABLED for p in pics)
    assert all(p.seq.strong_intra_smoothing == 0 for p in pics)
    assert strong_smoothing_areas(oracle, name) == 0
    assert modes_by_size([name])[5].sum() > 0                               # 32x32 blocks, where the smoothing would have been


# ---------------------------------------------------------------------------------------------------------------- constrained intra
def _intra_tus_beside_inter(p, min_log2=4):
    """luma intra TUs of 16x16 or larger with an inter-coded CU directly left of them or above them"""
    m = p.meta_np
    zx, zy = _zscan(p.parts)
    grid = np.full((p.height // 4 + 16, p.width // 4 + 16), -1, dtype=np.int32)      # pred_mode per 4x4 partition, -1 outside
    for a in range(p.num_ctus):
        gx, gy = (a % p.ctus_w) * (p.ctu_size // 4) + zx, (a // p.ctus_w) * (p.ctu_size // 4) + zy
        grid[gy, gx] = np.where(m["part_size"][a] != abi.SIZE_NONE, m["pred_mode"][a].astype(np.int32), -1)
    found = []
    for log2, mode, x, y in luma_tus(p):
        if log2 < min_log2:
            continue
        n, gx, gy = (1 << log2) // 4, x // 4, y // 4
        left = gx > 0 and (grid[gy:gy + n, gx - 1] == abi.MODE_INTER).any()
        above = gy > 0 and (grid[gy - 1, gx:gx + n] == abi.MODE_INTER).any()
        if left or above:
            found.append((int(log2), int(mode), int(x), int(y)))
    return found


@pytest.mark.parametrize("name", CIP)
def test_constrained_intra_fixture(oracle, name):
    pics = gu.stream_pictures(name)
    assert [p.slice_type for p in pics] == [abi.I_SLICE] + [abi.P_SLICE] * 4
    assert all(sl.constrained_intra_pred == 1 for p in pics for sl in p.slices)
    given = _oracle_pre(oracle, pics)
    cleared = _oracle_pre(oracle, pics, slice_fields={"constrained_intra_pred": 0})
    for p, g, o in zip(pics, given, cleared):
        for c in range(3):
            assert np.array_equal(g[c], p.pre[c])
        if p.slice_type == abi.I_SLICE:
            continue
        tus = _intra_tus_beside_inter(p)
        diff = _areas32(g[0], o[0])
        print("%s pic %d: %d intra TUs of 16x16 or more beside inter CUs (modes %s), %d areas of 32x32 differ with the flag cleared" % (
            name, p.index, len(tus), sorted({t[1] for t in tus}), diff))
        assert len(tus) >= 1
        assert diff >= 1


# ---------------------------------------------------------------------------------------------------------------- the floor before
def test_existing_fixtures_keep_their_modes():
    """the fixtures from synth_clip content (gu.STREAMS + gu.STREAMS_EXT), on record: how few large angular blocks they hold -- 13 of the 33
    angular modes at 16x16 and 6 at 32x32, in 35 and 14 TUs.  (PCM CUs are not counted: they carry DC in intra_dir_l without being
    predicted; with them DC reads 24 and 206.)  All sizes 4x4 and 8x8 hold every angular mode."""
    counts = modes_by_size(gu.STREAMS + gu.STREAMS_EXT)
    got = {s: (int(counts[s][0]), int(counts[s][1]), int(counts[s][2:].sum()), int((counts[s][2:] > 0).sum())) for s in (4, 5)}
    print("existing fixtures, (planar, DC, angular TUs, distinct angular modes): 16x16 %s, 32x32 %s" % (got[4], got[5]))
    assert all((counts[s][2:] > 0).all() for s in (2, 3))
    for s, floor in ((4, (36, 18, 35, 13)), (5, (36, 204, 14, 6))):
        assert all(g >= f for g, f in zip(got[s], floor)), (s, got[s])
