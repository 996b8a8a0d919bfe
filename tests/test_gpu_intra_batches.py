"""The batch forms of the intra kernel against HM itself.  tests/test_gpu_streams.py decodes one picture per call, so HM's data reaches
k_intra<kIntraWavesOne> only; here the pictures of the intra fixtures (gu.STREAMS_INTRA: every luma mode at 16x16 and 32x32, strong intra
smoothing at work, constrained intra prediction among inter CUs) go through hmgpu_decompress_pictures four at a time (kIntraWavesMany; the
lean instantiation where the call holds no I slice) and two at a time, bit-exact against HM's planes before and after the loop filters."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

CIP = "imodes_cip_ldp_main10_224x128"


def _same(got, want, what):
    for c in range(3):
        assert np.array_equal(got[c], want[c]), "%s, component %d" % (what, c)


def _decode_batch(ctx, jobs, expect):
    """one hmgpu_decompress_pictures call for jobs [(handle, picture)].  expect: "one" (fewer than four pictures), "many" (four or more, an I
    slice among them) or "lean" (four or more, no I slice).  The statistics count launches per kernel family, not per instantiation, so what
    is asserted is the host's rule (launch_intra in k_intra.hip: b.n >= 4 && lean, else b.n >= 4, else the one-picture kernel; lean = no I
    slice in the call, hmgpu_api.hip) from its inputs, and that the whole call was one intra launch"""
    n = len(jobs)
    any_islice = any(int(sl.slice_type) == abi.I_SLICE for _, p in jobs for sl in p.slices)
    rule = "lean" if (n >= 4 and not any_islice) else "many" if n >= 4 else "one"
    assert rule == expect
    assert all(((p.meta_np["pred_mode"] == abi.MODE_INTRA) & (p.meta_np["part_size"] != abi.SIZE_NONE)).any() for _, p in jobs)
    ctx.set_profiling(True)
    ctx.stats(reset=True)
    ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs) for h, p in jobs])
    ctx.sync()
    assert ctx.stats()["kernels"]["intra"][1] == 1
    ctx.set_profiling(False)


def _check(ctx, jobs, what):
    for h, p in jobs:
        _same(ctx.download(h), p.pre, "%s, picture %d in handle %d, reconstruction" % (what, p.index, h))
    ctx.filter_pictures([(h, p.pp, abi.sao_array_from_raw(p.sao_raw)) for h, p in jobs])
    for h, p in jobs:
        fin = ctx.download(h)
        _same(fin, p.fin, "%s, picture %d in handle %d, filtered" % (what, p.index, h))
        assert gu.hm_md5(fin, [p.bd_y, p.bd_c, p.bd_c]) == p.md5


@pytest.mark.parametrize("name", ["imodes_large_main12_416x256", "imodes_large_b_444_ccp_main10_416x256", "imodes_large_a_422_main8_416x256",
                                  "imodes_nosmooth_422_main12_224x128"])
def test_four_i_pictures_in_one_call(name):
    """k_intra<kIntraWavesMany> at the smallest batch it serves: the frames of an all-intra fixture, repeated cyclically into four handles
    (I pictures need no references)"""
    import libhm_amd
    pics = gu.stream_pictures(name)
    with libhm_amd.Context(pics[0].seq) as ctx:
        jobs = []
        for i in range(4):
            p = pics[i % len(pics)]
            h = ctx.acquire()
            ctx.upload(h, [np.full_like(a, 33 + i) for a in p.pre])
            jobs.append((h, p))
        _decode_batch(ctx, jobs, "many")
        _check(ctx, jobs, name)


def test_four_p_pictures_in_one_call():
    """the lean instantiation: the four P pictures of the constrained-intra fixture (intra TUs of 16x16 and 32x32 whose inter neighbours are
    no references) decoded in one call into handles of their own, from HM's final pictures in the handles the slices name"""
    import libhm_amd
    pics = gu.stream_pictures(CIP)
    assert len(pics) == 5 and pics[0].seq.max_pictures >= 9
    with libhm_amd.Context(pics[0].seq) as ctx:
        for p in pics:
            assert ctx.acquire() == p.index
            ctx.upload(p.index, p.fin)
        jobs = []
        for p in pics[1:]:
            h = ctx.acquire()
            ctx.upload(h, [np.full_like(a, 21) for a in p.pre])
            jobs.append((h, p))
        _decode_batch(ctx, jobs, "lean")
        _check(ctx, jobs, CIP)


@pytest.mark.parametrize("name", ["imodes_large_main8_416x256", "imodes_all_main10_416x240"])
def test_two_i_pictures_in_one_call(name):
    """more than one picture, fewer than four: the one-picture kernel over two pictures"""
    import libhm_amd
    pics = gu.stream_pictures(name)
    assert len(pics) == 2
    with libhm_amd.Context(pics[0].seq) as ctx:
        jobs = []
        for p in pics:
            h = ctx.acquire()
            ctx.upload(h, [np.full_like(a, 77) for a in p.pre])
            jobs.append((h, p))
        _decode_batch(ctx, jobs, "one")
        _check(ctx, jobs, name)


def test_i_and_p_pictures_in_one_call():
    """the I picture of the constrained-intra fixture among its P pictures: five pictures with an I slice in the call (kIntraWavesMany on
    pictures that are mostly inter)"""
    import libhm_amd
    pics = gu.stream_pictures(CIP)
    with libhm_amd.Context(pics[0].seq) as ctx:
        for p in pics:
            assert ctx.acquire() == p.index
            ctx.upload(p.index, p.fin)
        jobs = []
        for p in pics:
            h = ctx.acquire()
            ctx.upload(h, [np.full_like(a, 21) for a in p.pre])
            jobs.append((h, p))
        _decode_batch(ctx, jobs, "many")
        _check(ctx, jobs, CIP)


def test_every_input_form_gives_hms_planes():
    """a picture of HM's through ordinary arrays with dense levels, compact levels, a staging block (dense, then compact) and the packed entry"""
    import libhm_amd
    p = gu.stream_pictures("imodes_large_main8_416x256")[1]
    with libhm_amd.Context(p.seq) as ctx:
        hs = [ctx.acquire() for _ in range(5)]
        for hnd in hs:
            ctx.upload(hnd, [np.full_like(a, 9) for a in p.pre])
        compact = ctx.pack_levels(p.meta, p.coeffs)
        stg = ctx.staging_alloc()
        stg.fill(p.meta, p.coeffs)
        stg.set_groups(intra=True, flags=True)
        blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
        ctx.decompress_pictures([(hs[0], p.slices, p.meta, p.coeffs), (hs[1], p.slices, p.meta, compact), (hs[2], p.slices, stg, stg)])
        ctx.decompress_pictures_packed([(hs[3], p.slices, blob, None)])
        ctx.sync()
        stg.fill_compact(libhm_amd.lib(), ctx.seq, p.meta, p.coeffs)
        ctx.decompress_pictures([(hs[4], p.slices, stg, stg)])
        forms = ("dense arrays", "compact levels", "staging block", "packed entry", "staging block with compact levels")
        for hnd, form in zip(hs, forms):
            _same(ctx.download(hnd), p.pre, form + ", reconstruction")
        ctx.filter_pictures([(hnd, p.pp, abi.sao_array_from_raw(p.sao_raw)) for hnd in hs])
        for hnd, form in zip(hs, forms):
            _same(ctx.download(hnd), p.fin, form + ", filtered")
        ctx.staging_free(stg)
