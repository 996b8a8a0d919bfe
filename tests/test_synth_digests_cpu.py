"""tests/synth.py with its default keywords is the workload of bench.py and of every 4:2:0 / 64-CTU parity test: the pictures it draws
must not change when the generator learns new shapes (same arrays, same bytes, i.e. the PRNG consumed in the same order).

How the digests below were taken: this very file was run as a script (`python -m tests.test_synth_digests_cpu`) against
tests/synth.py of commit 4fd5969 -- the last commit before make_picture gained chroma_format / log2_ctu / bit_depth_chroma -- and
the printed table pasted into DIGESTS.  It uses no keyword that commit does not know.  One digest covers, in this order: every
array of p.meta.arrays (name, dtype, shape, bytes; absent arrays by name), the three level arrays, sao_raw, the bytes of every
hmgpu_slice_params of the picture and its slice ranges, the sequence parameters and p.inside / p.intra.
"""
import hashlib

import numpy as np

from tests import synth

BENCH_SEED = 0x484D3136          # bench.py: seed = BENCH_SEED + 7 * rank + i, i = 0, 1

# (name, positional (width, height, bit depth), keywords)
CASES = [
    # bench.py --workload full / mc (P) and --bi 1 / mc_bi (B), both pictures of the pair, at its default size
    ("bench_full_p0", (3840, 2160, 10), dict(seed=BENCH_SEED, bi=False, ref_handles=([0], [1]))),
    ("bench_full_p1", (3840, 2160, 10), dict(seed=BENCH_SEED + 1, bi=False, ref_handles=([0], [1]))),
    ("bench_full_b0", (3840, 2160, 10), dict(seed=BENCH_SEED, bi=True, ref_handles=([0], [1]))),
    ("bench_full_b1", (3840, 2160, 10), dict(seed=BENCH_SEED + 1, bi=True, ref_handles=([0], [1]))),
    # the other workloads' keywords (1080p keeps the test short; the code path does not depend on the size)
    ("bench_idct", (1920, 1080, 10), dict(seed=BENCH_SEED, bi=False, ref_handles=([0], [1]), mode_probs=(1.0, 0, 0, 0, 0), cbf_prob=1.0,
                                          coef_dist="stress", sao=False)),
    ("bench_filter", (1920, 1080, 10), dict(seed=BENCH_SEED + 1, bi=False, ref_handles=([0], [1]), intra_frac=0.25, intra_modes=False)),
    ("bench_intra", (1920, 1080, 10), dict(seed=BENCH_SEED, bi=False, ref_handles=([0], [1]), intra_frac=1.0)),
    ("bench_gop", (1920, 1080, 10), dict(seed=BENCH_SEED + 5, bi=True, ref_handles=([0], [0]))),
    ("bench_rank1", (1920, 1080, 10), dict(seed=BENCH_SEED + 7, bi=False, ref_handles=([0], [1]))),
    ("bench_experiment_flags", (1920, 1080, 10), dict(seed=BENCH_SEED, bi=True, ref_handles=([0], [1]), cbf_prob=0.3, intra_frac=0.1, mv_range=8,
                                                      mode_probs=(0.2, 0.2, 0.2, 0.2, 0.2))),
    # tests/test_gpu_fullsize.py and smoke()
    ("smoke", (416, 240, 10), dict(seed=9, bi=True, intra_frac=0.05, ref_handles=([0], [1]))),
    ("fullsize_bi_8bit", (416, 240, 8), dict(seed=416 + 8 + 1, bi=True, intra_frac=0.1, ref_handles=([0], [1]))),
    ("fullsize_12bit", (832, 480, 12), dict(seed=832 + 12, bi=False, intra_frac=0.3, ref_handles=([0], [1]))),
    ("fullsize_five_slices", (832, 480, 10), dict(seed=91, intra_frac=0.3, ref_handles=([0], [0]), num_slices=5, lf_across_slices=0)),
    ("fullsize_stress_ts", (1920, 1080, 10), dict(seed=0x484D3136 + 10 + 1, mode_probs=(0, 0, 0, 1.0, 0), cbf_prob=1.0, coef_dist="stress", sao=False,
                                                  tr_split_prob=1.0, intra_frac=0.0, ref_handles=([0], [1]))),
    ("fullsize_dense", (832, 480, 10), dict(seed=3, mode_probs=(0, 0, 0.5, 0.5, 0), cbf_prob=1.0, coef_dist="dense", sao=False, tr_split_prob=0.5,
                                            intra_frac=0.3, ref_handles=([0], [1]))),
    ("fullsize_partial_ctus", (200, 136, 8), dict(seed=0x1A7 + 3, mode_probs=(0, 0, 0, 1, 0), tr_split_prob=0.7, intra_frac=1.0, cbf_prob=0.7, sao=False,
                                                  ref_handles=([0], [0]))),
    ("fullsize_partial_ctus_16", (416, 240, 10), dict(seed=0xFA17, intra_frac=1.0, cbf_prob=0.5, sao=False, ref_handles=([0], [0]))),
    ("two_refs_three_slices", (832, 480, 8), dict(seed=0x5CA7 + 14, intra_frac=0.25, num_refs=2, ref_handles=([0, 1], [0]), num_slices=3, cbf_prob=0.6)),
]

DIGESTS = {
    "bench_full_p0": "f0b94fe1d739cf7f3c903a1a8e48032a1cb6ffa1b8d3d08cba6bc62d0131bb9e",
    "bench_full_p1": "6cf9e305e2b7e7bc2fd0189af99664097d3511432b1d7d6d4b6cc9a1793a88cd",
    "bench_full_b0": "6335084d29d6b922ad06577bcfb130d103cb619437a4786d61cfc4753b4da91f",
    "bench_full_b1": "70f6b35faaa24eb841930c94cb46e026ee2f650237791d073fb06ad982cdc475",
    "bench_idct": "c644d22b674c2c757f1240ee0c6b647a6e4e7676aee70d7b13a68892cadf629f",
    "bench_filter": "0e5cb7066f17ec036e0611be1bbb2a6ee7bb23594993169a9a9a9d4694e97e11",
    "bench_intra": "b1a61510033c8dcaddc608e2a37454ba48ebabe1472cdd17e2950e679a82d341",
    "bench_gop": "5ae4556cf7349885256481484e0184d93392f9035104d264c4934c3f0a71eff5",
    "bench_rank1": "fe908e2c6be6927fb5940e8fa524c03f2da35ecfd99ba9de16f268421b748a07",
    "bench_experiment_flags": "e482b85793e1c36d4e3ec1e0451712e05b0a479fddc6114017a3b3c3a6f94a5f",
    "smoke": "7cd8023d9843719c132362888e7517681216e7bb304a3e9c17798b4ddf426b56",
    "fullsize_bi_8bit": "7b3e63fe9ac7592daa1c2213f85c64bcae7e0019d8130bbb830db8d2180bb71a",
    "fullsize_12bit": "3d548e0abb05a401ee32bf6715544d18a03476141c033af4bed7fc81392e52dd",
    "fullsize_five_slices": "aa0a92ff331e54de68a658bfab05957381d00ed5b1184e6bb8934fdb239efafb",
    "fullsize_stress_ts": "e1aac014b42eacbf36f82194dcaa7bf5f81366fabdb7a84369961d7fbb725239",
    "fullsize_dense": "192b40661523f601125867822d8d33a1bb303374bb4d7e7bc28fecd8096fd970",
    "fullsize_partial_ctus": "12667a9b0d39c2901a6bca80cbd941ecc559c1176896e8daccc04b17127eb32a",
    "fullsize_partial_ctus_16": "3cd8b9ef37f2dda0489d9581782d695a4fe1def13c9375050b212aaae9355b4a",
    "two_refs_three_slices": "dc049c48f0fd9de42d832eb3c88319807e71e93fccb7aaed9514086335d4ec06",
}

PLANE_CASES = [("noise", (3840, 2160, 10, 100)), ("noise", (416, 240, 8, 11)), ("blocky", (3840, 2160, 10, 200)), ("blocky", (200, 136, 12, 13))]
PLANE_DIGESTS = {
    "noise(3840, 2160, 10, 100)": "5e29afc5a4722a13715a6c093b834196eece01557c8a5b7f2713a08dad5cc77d",
    "noise(416, 240, 8, 11)": "261a9a99d7e7c47cc78a7c69cbf625b17cbfe803438719f5044ebbb7c64f0993",
    "blocky(3840, 2160, 10, 200)": "fd617956401e1a8cc964d4532053af73f67f7f06419b39c0cc8201d4f1c26ad8",
    "blocky(200, 136, 12, 13)": "e15924f590f100bd4b48fb8d5156a2fd056dc9e105a6124755749eb46b13d102",
}


def _feed(h, name, a):
    h.update(name.encode())
    if a is None:
        h.update(b"<none>")
        return
    a = np.ascontiguousarray(a)
    h.update(str(a.dtype).encode() + str(a.shape).encode())
    h.update(a.tobytes())


def picture_digest(p):
    h = hashlib.sha256()
    for name in sorted(p.meta.arrays):
        _feed(h, name, p.meta.arrays[name])
    for name in sorted(p.meta_np):
        _feed(h, "np_" + name, np.asarray(p.meta_np[name]))
    for k in range(3):
        _feed(h, "level%d" % k, p.coeffs.arrays[k])
    _feed(h, "sao_raw", p.sao_raw)
    for sl in p.slices:
        raw = bytearray(bytes(sl))
        h.update(bytes(raw))
    _feed(h, "slice_ranges", np.array(p.slice_ranges, dtype=np.int64))
    h.update(bytes(p.seq))
    h.update(bytes(p.pp))
    _feed(h, "inside", p.inside)
    _feed(h, "intra", p.intra)
    h.update(repr((p.width, p.height, p.bit_depth, p.num_ctus, p.ctus_w)).encode())
    return h.hexdigest()


def plane_digest(kind, args):
    planes = (synth.noise_planes if kind == "noise" else synth.blocky_planes)(*args)
    h = hashlib.sha256()
    for c, a in enumerate(planes):
        _feed(h, "plane%d" % c, a)
    return h.hexdigest()


def test_case_names_are_unique_and_all_pinned():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    assert set(names) == set(DIGESTS)
    assert {"%s%r" % c for c in PLANE_CASES} == set(PLANE_DIGESTS)


def test_default_pictures_are_byte_identical_to_the_pinned_generator():
    for name, pos, kw in CASES:
        assert picture_digest(synth.make_picture(*pos, **kw)) == DIGESTS[name], "make_picture changed its default output: case %s" % name


def test_default_planes_are_byte_identical_to_the_pinned_generator():
    for kind, args in PLANE_CASES:
        assert plane_digest(kind, args) == PLANE_DIGESTS["%s%r" % (kind, args)], "%s_planes%r changed" % (kind, args)


if __name__ == "__main__":
    print("DIGESTS = {")
    for name, pos, kw in CASES:
        print('    "%s": "%s",' % (name, picture_digest(synth.make_picture(*pos, **kw))))
    print("}")
    print("PLANE_DIGESTS = {")
    for kind, args in PLANE_CASES:
        print('    "%s%r": "%s",' % (kind, args, plane_digest(kind, args)))
    print("}")
