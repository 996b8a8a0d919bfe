"""The packed picture input on the host (hmgpu_pack_input / hmgpu_unpack_input / hmgpu_packed_max_bytes): exact round trips on HM's
own metadata and on synthetic 2160p pictures, determinism, the byte budget, the validator on malformed blobs, the format envelope and the
ABI of the new struct.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import golden_util as gu
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_WORDS = 8                      # magic, version, num_ctus, parts, groups, bytes, 2 reserved; then {offset, size} per section
S_CTU, S_LSTART, S_LTAB, S_LDATA = 0, 16, 17, 18
BENCH_SEED = 0x484D3136
# the fixtures with HM's metadata in 4:0:0 / 4:2:0
FIXTURES_420 = gu.STREAMS + gu.STREAMS_BD12 + gu.STREAMS_INTRA_420
COMPARED = ["depth", "part_size", "pred_mode", "qp", "tr_idx", "cbf_y", "cbf_u", "cbf_v", "ts_y", "ts_u", "ts_v", "mv0", "mv1",
            "ref_idx0", "ref_idx1", "intra_dir_l", "intra_dir_c", "bypass", "ipcm", "slice_idx", "tile_idx"]


def _check_round_trip(seq, meta_np, meta, coeffs, what):
    blob = libhm_amd.pack_input(seq, meta, coeffs)
    assert blob.nbytes <= libhm_amd.packed_max_bytes(seq)
    arrays, levels, starts = libhm_amd.unpack_input(seq, blob)
    for name in COMPARED:
        want = meta_np.get(name)
        if want is None:
            continue
        got = arrays[name].reshape(-1)
        assert np.array_equal(got, np.asarray(want).reshape(-1).astype(got.dtype)), "%s: %s" % (what, name)
    ref = libhm_amd.pack_levels(seq, meta, coeffs)
    n = abi.num_ctus(seq)
    for k in range(3):
        assert np.array_equal(starts[k], ref.starts[k]), "%s: CTU starts of component %d" % (what, k)
        assert np.array_equal(levels[k], ref.arrays[k][:int(ref.starts[k][n])]), "%s: levels of component %d" % (what, k)
    return blob


@pytest.mark.parametrize("name", FIXTURES_420)
def test_round_trip_golden_fixtures(name):
    pics = gu.stream_pictures(name)
    assert pics[0].chroma_format in (0, 1)
    for p in pics:
        _check_round_trip(p.seq, p.meta_np, p.meta, p.coeffs, "%s pic %d" % (name, p.index))


SYNTH = {"P": dict(), "B": dict(bi=True), "intra25": dict(intra_frac=0.25), "stress": dict(coef_dist="stress"),
         "dense": dict(coef_dist="dense")}


@pytest.mark.parametrize("kind", sorted(SYNTH))
def test_round_trip_synthetic_2160p(kind):
    p = synth.make_picture(3840, 2160, 10, seed=11, ref_handles=([0], [1]), **SYNTH[kind])
    _check_round_trip(p.seq, p.meta_np, p.meta, p.coeffs, kind)


def test_dense_and_compact_levels_give_the_same_blob():
    for kw in ({}, dict(bi=True, intra_frac=0.25)):
        p = synth.make_picture(1920, 1080, 10, seed=5, ref_handles=([0], [1]), **kw)
        a = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
        b = libhm_amd.pack_input(p.seq, p.meta, libhm_amd.pack_levels(p.seq, p.meta, p.coeffs))
        assert a.tobytes() == b.tobytes()
        assert libhm_amd.pack_input(p.seq, p.meta, p.coeffs).tobytes() == a.tobytes()


@pytest.mark.parametrize("bi,limit", [(False, 6e6), (True, 7e6)])
def test_bench_pictures_fit_the_byte_budget(bi, limit):
    p = synth.make_picture(3840, 2160, 10, seed=BENCH_SEED, bi=bi, ref_handles=([0], [1]))
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
    assert blob.nbytes <= limit, blob.nbytes
    # and about 3x fewer bytes than the arrays + compact levels the staging blocks move
    ref = libhm_amd.pack_levels(p.seq, p.meta, p.coeffs)
    n = abi.num_ctus(p.seq)
    assert blob.nbytes * 2.5 < 2 * sum(int(ref.starts[k][n]) for k in range(3)) + 13 * n * 256


def _adversarial(seq):
    """a different tuple in every partition of every group, every level of every full-length piece non-zero"""
    n, parts, ctu = abi.num_ctus(seq), abi.parts_per_ctu(seq), 1 << seq.log2_ctu_size
    z = np.arange(n * parts)
    m = {"depth": z % 2, "part_size": z % 3, "pred_mode": z % 2, "qp": z % 50, "tr_idx": z % 2, "cbf_y": z % 2, "cbf_u": z % 2,
         "cbf_v": z % 2, "ts_y": z % 2, "ts_u": z % 2, "ts_v": z % 2, "mv0": np.arange(2 * n * parts) % 1000,
         "mv1": np.arange(2 * n * parts) % 999, "ref_idx0": z % 2, "ref_idx1": z % 2, "intra_dir_l": z % 35, "intra_dir_c": z % 5,
         "bypass": z % 2, "ipcm": z % 2, "slice_idx": np.zeros(n), "tile_idx": np.arange(n) % 3}
    meta = abi.MetaHolder(m)
    per = [ctu * ctu >> (2 if k else 0) for k in range(3)]
    lv = [(np.arange(n * per[k]) % 2000 + 1).astype(np.int16) for k in range(3)]
    co = abi.CoeffHolder(*lv)
    co.starts = [(np.arange(n + 1) * per[k]).astype(np.uint32) for k in range(3)]
    for k in range(3):
        co.struct.ctu_level_start[k] = co.starts[k].ctypes.data
    return m, meta, co


@pytest.mark.parametrize("log2_ctu", [4, 5, 6])
def test_adversarial_input_stays_within_max_bytes(log2_ctu):
    seq = abi.make_seq(416, 240, 10, log2_ctu=log2_ctu)
    m, meta, co = _adversarial(seq)
    blob = libhm_amd.pack_input(seq, meta, co)
    assert blob.nbytes <= libhm_amd.packed_max_bytes(seq)
    arrays, levels, starts = libhm_amd.unpack_input(seq, blob)
    for name in COMPARED:
        assert np.array_equal(arrays[name].reshape(-1), np.asarray(m[name]).reshape(-1).astype(arrays[name].dtype)), name
    for k in range(3):
        assert np.array_equal(levels[k], co.arrays[k]) and np.array_equal(starts[k], co.starts[k])
    # a capacity one byte short is refused
    out = np.zeros(blob.nbytes + 16, dtype=np.uint8)
    out = out[(-out.ctypes.data) % 16:][:blob.nbytes - 1]
    with pytest.raises(libhm_amd.HmgpuError):
        libhm_amd.pack_input(seq, meta, co, out=out)


@pytest.fixture(scope="module")
def small():
    p = synth.make_picture(416, 240, 10, seed=3, bi=True, intra_frac=0.25, ref_handles=([0], [1]))
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
    return p, blob.copy()


def _words(blob):
    return blob.view(np.uint32)


def _sec(blob, s):
    w = _words(blob)
    return int(w[HEADER_WORDS + 2 * s]), int(w[HEADER_WORDS + 2 * s + 1])


def _status(seq, blob):
    return libhm_amd.unpack_input_status(seq, blob)


def test_valid_blob_passes(small):
    p, blob = small
    assert _status(p.seq, blob) == abi.HMGPU_OK


def test_truncated_blobs(small):
    p, blob = small
    for n in sorted(set([0, 4, 100, 191, 192, blob.nbytes // 2, blob.nbytes - 4, blob.nbytes - 1])):
        assert _status(p.seq, blob[:n].copy()) == abi.HMGPU_EINVAL, n
    longer = np.concatenate([blob, np.zeros(16, dtype=np.uint8)])
    assert _status(p.seq, longer) == abi.HMGPU_EINVAL


def _mutated(blob, fn):
    b = blob.copy()
    fn(b)
    return b


def test_hand_made_malformed_blobs(small):
    p, blob = small
    seq = p.seq
    n, parts = abi.num_ctus(seq), abi.parts_per_ctu(seq)
    cases = {}
    cases["magic"] = _mutated(blob, lambda b: _words(b).__setitem__(0, 0x12345678))
    cases["version"] = _mutated(blob, lambda b: _words(b).__setitem__(1, 2))
    cases["num_ctus"] = _mutated(blob, lambda b: _words(b).__setitem__(2, n + 1))
    cases["parts"] = _mutated(blob, lambda b: _words(b).__setitem__(3, parts // 4))
    cases["groups without CU"] = _mutated(blob, lambda b: _words(b).__setitem__(4, int(_words(b)[4]) & ~1))
    cases["unknown group"] = _mutated(blob, lambda b: _words(b).__setitem__(4, int(_words(b)[4]) | 64))
    cases["bytes"] = _mutated(blob, lambda b: _words(b).__setitem__(5, blob.nbytes + 16))
    for s in (S_CTU, 2, S_LTAB, S_LDATA):
        cases["section %d past the end" % s] = _mutated(blob, lambda b, s=s: _words(b).__setitem__(HEADER_WORDS + 2 * s, blob.nbytes))
        cases["section %d misaligned" % s] = _mutated(blob, lambda b, s=s: _words(b).__setitem__(HEADER_WORDS + 2 * s,
                                                                                                 _sec(blob, s)[0] + 4))
    cases["section inside the header"] = _mutated(blob, lambda b: _words(b).__setitem__(HEADER_WORDS + 2 * S_CTU, 16))
    # run ends of the CU group (section 2): the first CTU's runs
    off_st, _ = _sec(blob, 1)
    off_en, _ = _sec(blob, 2)
    st = blob[off_st:off_st + 8].view(np.uint32)
    nr = int(st[1] - st[0])
    assert nr >= 2
    ends = lambda b: b[off_en:off_en + 2 * nr].view(np.uint16)
    cases["non-ascending ends"] = _mutated(blob, lambda b: ends(b).__setitem__(1, ends(b)[0]))
    cases["last end not parts"] = _mutated(blob, lambda b: ends(b).__setitem__(nr - 1, parts - 1))
    cases["last end beyond parts"] = _mutated(blob, lambda b: ends(b).__setitem__(nr - 1, parts + 1))
    cases["zero end"] = _mutated(blob, lambda b: ends(b).__setitem__(0, 0))
    cases["run start"] = _mutated(blob, lambda b: b[off_st:off_st + 4].view(np.uint32).__setitem__(0, 1))
    # levels: a sparse piece -- positions outside the piece, duplicates
    ls_off, _ = _sec(blob, S_LSTART)
    lt_off, _ = _sec(blob, S_LTAB)
    d_off, _ = _sec(blob, S_LDATA)
    lstart = blob[ls_off:ls_off + 12 * (n + 1)].view(np.uint32).reshape(3, n + 1)
    ltab = blob[lt_off:lt_off + 24 * n].view(np.uint32).reshape(n, 3, 2)
    sparse = [(a, k) for a in range(n) for k in range(3) if ltab[a, k, 1] != 0x80000000 and ltab[a, k, 1] >= 2]
    assert sparse
    a, k = sparse[0]
    npairs, length = int(ltab[a, k, 1]), int(lstart[k, a + 1] - lstart[k, a])
    pos = lambda b: b[d_off + 4 * int(ltab[a, k, 0]):][:2 * npairs].view(np.uint16)
    cases["position outside the piece"] = _mutated(blob, lambda b: pos(b).__setitem__(npairs - 1, length))
    cases["duplicate positions"] = _mutated(blob, lambda b: pos(b).__setitem__(1, pos(b)[0]))
    cases["descending positions"] = _mutated(blob, lambda b: (pos(b).__setitem__(0, pos(b)[1]), pos(b).__setitem__(1, pos(b)[0] - 1)))
    cases["more pairs than levels"] = _mutated(blob, lambda b: b[lt_off:].view(np.uint32).__setitem__((a * 3 + k) * 2 + 1, length + 1))
    cases["piece data past the section"] = _mutated(blob, lambda b: b[lt_off:].view(np.uint32).__setitem__((a * 3 + k) * 2, 1 << 28))
    cases["CTU piece longer than a CTU"] = _mutated(blob, lambda b: b[ls_off:].view(np.uint32).__setitem__(n, 1 << 20))
    cases["first CTU start"] = _mutated(blob, lambda b: b[ls_off:].view(np.uint32).__setitem__(0, 1))
    for what, b in cases.items():
        assert _status(seq, b) == abi.HMGPU_EINVAL, what


def test_seeded_mutations_never_crash(small):
    """random bytes of the structure (header, run tables, level tables and positions) changed: the validator says EINVAL or, for a
    change that leaves a well-formed blob, expands it -- inside the caller's buffers"""
    p, blob = small
    rng = np.random.RandomState(1234)
    structural = [(0, 192)]
    for s in (1, 2, 4, 5, 7, 8, S_LSTART, S_LTAB):
        o, sz = _sec(blob, s)
        structural.append((o, o + sz))
    n_inval = 0
    for i in range(300):
        b = blob.copy()
        for _ in range(1 + i % 3):
            lo, hi = structural[rng.randint(len(structural))]
            if hi <= lo:
                continue
            b[rng.randint(lo, hi)] ^= np.uint8(1 << rng.randint(8))
        st = _status(p.seq, b)
        assert st in (abi.HMGPU_OK, abi.HMGPU_EINVAL)
        if st == abi.HMGPU_OK:
            libhm_amd.unpack_input(p.seq, b)
        n_inval += st == abi.HMGPU_EINVAL
    assert n_inval > 150


@pytest.mark.parametrize("fmt", [2, 3])
def test_422_and_444_are_unsupported(fmt):
    p = synth.make_picture(416, 240, 10, seed=4, ref_handles=([0], [1]))
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    seq.chroma_format = fmt
    with pytest.raises(libhm_amd.HmgpuError) as e:
        libhm_amd.pack_input(seq, p.meta, p.coeffs)
    assert e.value.status == abi.HMGPU_EUNSUPPORTED
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
    assert _status(seq, blob) == abi.HMGPU_EUNSUPPORTED


def test_meta_out_struct_matches_the_header(tmp_path):
    src = tmp_path / "mo.c"
    src.write_text('#include <stdio.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu\\n",sizeof(hmgpu_ctu_meta_out),'
                   'sizeof(hmgpu_ctu_meta));return 0;}\n')
    exe = tmp_path / "mo"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(abi.CtuMetaOut), C.sizeof(abi.CtuMeta)]


def test_packed_job_struct_matches_the_header(tmp_path):
    from libhm_amd import build
    build.build()
    src = tmp_path / "pk.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hmgpu.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n",'
                   'sizeof(hmgpu_packed_job),offsetof(hmgpu_packed_job,blob),offsetof(hmgpu_packed_job,bytes),'
                   'offsetof(hmgpu_packed_job,pcm_sample),offsetof(hmgpu_packed_job,slices));return 0;}\n')
    exe = tmp_path / "pk"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    J = abi.PackedJob
    assert got == [C.sizeof(J), J.blob.offset, J.bytes.offset, J.pcm_sample.offset, J.slices.offset]
