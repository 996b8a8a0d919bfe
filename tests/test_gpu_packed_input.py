"""GPU: the packed picture input (hmgpu_decompress_pictures_packed + k_unpack) -- HM's fixtures against HM's planes, synthetic 2160p
pictures against the array path on the same pictures, one expansion launch per call, and picture handles that alternate between the
array path and the packed one."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import golden_util as gu
from tests import synth

pytestmark = pytest.mark.gpu

FIXTURES_420 = gu.STREAMS + gu.STREAMS_BD12 + gu.STREAMS_INTRA_420


@pytest.mark.parametrize("name", FIXTURES_420)
def test_fixture_pictures_through_the_packed_entry_match_hm(name):
    """PCM, lossless, transform skip, weighted prediction, scaling lists, tiles, slices, constrained intra prediction, intra pictures"""
    import libhm_amd
    pics = gu.stream_pictures(name)
    with libhm_amd.Context(pics[0].seq) as ctx:
        for p in pics:
            h = ctx.acquire()
            assert h == p.index
            ctx.upload(h, [np.full_like(a, 77) for a in p.pre])
            blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
            ctx.decompress_pictures_packed([(h, p.slices, blob, p.coeffs.pcm)])
            rec = ctx.download(h)
            for c in range(3):
                assert np.array_equal(rec[c], p.pre[c]), "%s pic %d comp %d: reconstruction" % (name, p.index, c)
            ctx.filter_picture(h, p.pp, p.sao_raw, stages=3)
            dbk = ctx.download(h)
            for c in range(3):
                assert np.array_equal(dbk[c], p.dbk[c]), "%s pic %d comp %d: deblocking" % (name, p.index, c)
            ctx.filter_picture(h, p.pp, p.sao_raw, stages=4)
            fin = ctx.download(h)
            for c in range(3):
                assert np.array_equal(fin[c], p.fin[c]), "%s pic %d comp %d: SAO" % (name, p.index, c)


SYNTH = {"P": dict(), "B": dict(bi=True), "intra5": dict(intra_frac=0.05), "intra25": dict(intra_frac=0.25, bi=True),
         "stress": dict(coef_dist="stress")}


@pytest.mark.parametrize("n", [1, 16])
@pytest.mark.parametrize("kind", sorted(SYNTH))
def test_synthetic_2160p_matches_the_array_path(kind, n):
    import libhm_amd
    w, h, bd = 3840, 2160, 10
    p = synth.make_picture(w, h, bd, seed=0x484D3136, ref_handles=([0], [1]), **SYNTH[kind])
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    seq.max_pictures = 2 + 2 * n
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
    compact = libhm_amd.pack_levels(p.seq, p.meta, p.coeffs)
    with libhm_amd.Context(seq) as ctx:
        r0, r1 = ctx.acquire(), ctx.acquire()
        assert (r0, r1) == (0, 1)
        ctx.upload(r0, synth.noise_planes(w, h, bd, 1))
        ctx.upload(r1, synth.blocky_planes(w, h, bd, 2))
        arr = [ctx.acquire() for _ in range(n)]
        pk = [ctx.acquire() for _ in range(n)]
        start = synth.blocky_planes(w, h, bd, 3)
        for t in arr + pk:
            ctx.upload(t, start)
        ctx.decompress_pictures([(t, [p.slice], p.meta, compact) for t in arr])
        ctx.filter_pictures([(t, p.pp, abi.sao_array_from_raw(p.sao_raw)) for t in arr])
        ctx.set_profiling(True)
        ctx.stats(reset=True)
        ctx.decompress_pictures_packed([(t, [p.slice], blob, None) for t in pk])
        ctx.sync()
        st = ctx.stats(reset=True)
        ctx.set_profiling(False)
        assert st["kernels"]["unpack"][1] == 1, st["kernels"]["unpack"]
        ctx.filter_pictures([(t, p.pp, abi.sao_array_from_raw(p.sao_raw)) for t in pk])
        want = ctx.download(arr[0])
        for t in pk:
            got = ctx.download(t)
            for c in range(3):
                assert np.array_equal(got[c], want[c]), "%s n=%d picture %d comp %d" % (kind, n, t, c)
        if n > 1:
            for t in arr[1:]:
                other = ctx.download(t)
                assert all(np.array_equal(other[c], want[c]) for c in range(3))


def test_picture_handle_alternates_between_arrays_and_packed():
    """a lossless picture through the arrays (transform-skip / lossless flags on the device), a plain picture through the packed form in
    the same handle, then the lossless one through the arrays again: the flags the device holds must follow each time"""
    import libhm_amd
    name = "ldp_lossless_main10_208x120"
    pics = gu.stream_pictures(name)
    p0 = pics[0]
    assert int(np.asarray(p0.meta_np["bypass"]).max()) == 1 or int(np.asarray(p0.meta_np["ts_y"]).max()) >= 1
    seq = abi.SeqParams.from_buffer_copy(p0.seq)
    seq.max_pictures = 6
    w, h, bd = p0.width, p0.height, p0.bd_y
    with libhm_amd.Context(seq) as ctx:
        hc, r0, r1, href = ctx.acquire(), ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(r0, synth.noise_planes(w, h, bd, 1))
        ctx.upload(r1, synth.blocky_planes(w, h, bd, 2))
        plain = synth.make_picture(w, h, bd, seed=21, bi=True, intra_frac=0.1, ref_handles=([r0], [r1]))
        blob = libhm_amd.pack_input(seq, plain.meta, plain.coeffs)

        def lossless():
            ctx.upload(hc, [np.full_like(a, 77) for a in p0.pre])
            ctx.decompress_pictures([(hc, p0.slices, p0.meta, p0.coeffs)])
            ctx.filter_picture(hc, p0.pp, p0.sao_raw)
            fin = ctx.download(hc)
            for c in range(3):
                assert np.array_equal(fin[c], p0.fin[c]), "lossless picture comp %d" % c

        lossless()
        start = synth.blocky_planes(w, h, bd, 3)
        ctx.upload(hc, start)
        ctx.decompress_pictures_packed([(hc, [plain.slice], blob, None)])
        ctx.filter_picture(hc, plain.pp, plain.sao_raw)
        got = ctx.download(hc)
        ctx.upload(href, start)
        ctx.decompress_pictures([(href, [plain.slice], plain.meta, plain.coeffs)])
        ctx.filter_picture(href, plain.pp, plain.sao_raw)
        want = ctx.download(href)
        for c in range(3):
            assert np.array_equal(got[c], want[c]), "plain picture through the packed form, comp %d" % c
        lossless()


def test_bad_blob_is_refused_before_anything_runs():
    import libhm_amd
    p = synth.make_picture(416, 240, 10, seed=8, ref_handles=([0], [1]))
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs).copy()
    blob[:4] = 0
    with libhm_amd.Context(seq) as ctx:
        r0, r1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.decompress_pictures_packed([(hc, [p.slice], blob, None)])
        assert e.value.status == abi.HMGPU_EINVAL
        ctx.sync()


# ---- libhmdec with packed input on: every 4:0:0 / 4:2:0 bitstream of the fixtures, against the same decoder with it off
DEC_420 = [("stream_" + n) for n in gu.STREAMS + gu.STREAMS_BD12] + \
    [("lite_" + n) for n in gu.LITE + gu.LITE_BD12 + gu.SURGERY if "_444" not in n and "_422" not in n]
BINS = ["bench_ldp_main10_1920x1080_17.bin", "bench_ra_main10_1920x1080.bin", "bench_ldp_main10_3840x2160.bin",
        "bench_ldp_wpp_main10_3840x2160.bin"]


def _bitstream(name):
    import os
    if name.endswith(".bin"):
        return open(os.path.join(gu.GOLD, name), "rb").read()
    return gu.load(name)["bitstream"]


def _decode(data, packed, threads, devices=None, chroma=True):
    from libhm_amd import hmdec
    out = {}
    with hmdec.Decoder(threads=threads, devices=devices, packed_input=packed) as d:
        def on_output(p):
            out[p.poc] = [p.cropped_plane(c).copy() for c in range(3 if chroma else 1)]
        d.decode_stream(data, on_output=on_output)
        assert d.hash_mismatches == 0
        return out, d.pictures_decoded, d.packed_pictures


def _check_decoder(name, threads, devices=None):
    data = _bitstream(name)
    chroma = "_mono_" not in name
    off, n_off, p_off = _decode(data, False, threads, devices, chroma)
    on, n_on, p_on = _decode(data, True, threads, devices, chroma)
    assert p_off == 0 and n_on == n_off and p_on == n_on > 0, (p_off, n_off, n_on, p_on)
    assert sorted(on) == sorted(off)
    for poc in off:
        for c in range(len(off[poc])):
            assert np.array_equal(on[poc][c], off[poc][c]), "%s POC %d component %d" % (name, poc, c)


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("name", DEC_420 + BINS)
def test_libhmdec_with_packed_input_matches_packed_input_off(name, threads):
    _check_decoder(name, threads)


@pytest.mark.parametrize("name", ["stream_ra_main10_208x120", "lite_ldp_wpp_main10_416x240", "lite_ldb_mono_rext_main8_208x120",
                                  "bench_ra_main10_1920x1080.bin"])
def test_libhmdec_packed_input_on_two_contexts_of_one_gpu(name, monkeypatch):
    monkeypatch.setenv("HMDEC_PLACE_ROUND_ROBIN", "1")       # (every picture moves on: both contexts copy blobs)
    _check_decoder(name, 3, devices=[0, 0])


def test_duplicate_level_positions_are_refused_by_the_packed_entry():
    """the packed entry validates the whole blob, level positions included, before anything is enqueued"""
    import libhm_amd
    p = synth.make_picture(416, 240, 10, seed=8, ref_handles=([0], [1]))
    seq = abi.SeqParams.from_buffer_copy(p.seq)
    blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs).copy()
    w = blob.view(np.uint32)
    lt_off, d_off = int(w[8 + 2 * 17]), int(w[8 + 2 * 18])
    n = abi.num_ctus(seq)
    ltab = blob[lt_off:lt_off + 24 * n].view(np.uint32).reshape(n, 3, 2)
    a, k = next((a, k) for a in range(n) for k in range(3) if ltab[a, k, 1] != 0x80000000 and ltab[a, k, 1] >= 2)
    pos = blob[d_off + 4 * int(ltab[a, k, 0]):][:4].view(np.uint16)
    pos[1] = pos[0]
    with libhm_amd.Context(seq) as ctx:
        r0, r1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        with pytest.raises(libhm_amd.HmgpuError) as e:
            ctx.decompress_pictures_packed([(hc, [p.slice], blob, None)])
        assert e.value.status == abi.HMGPU_EINVAL
        ctx.sync()
