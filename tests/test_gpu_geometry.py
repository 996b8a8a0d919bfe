"""GPU parity at the extremes of picture, batch and slab geometry, where grid mappings and address arithmetic degenerate: pictures of one
to a few CTUs (8x8 to 72x64, every CTU size and chroma format) through every stage, every input form and as references read through their
margins; batches of 1 to 16 such pictures per call; strips past 4096 and 8192 samples; contexts of 64 pictures with references at handles 32
and above; a slab of pictures of more than 4 GiB, where the motion-compensation kernels take plain 64-bit addresses; and the side-information
and analysis exports on pictures smaller than a CTU.  The cases are those of tests/geometry_cases.py, which tests/test_geometry_cases_cpu.py
holds to what their names say; everything is compared bit for bit with the C oracle or the exports' reference modules."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import cu_shapes as cs
from tests import geometry_cases as gc
from tests import synth
from tests.test_gpu_filter_margins import REGIONS
from tests.test_gpu_formats_fullsize import _check_all_stages, _decompress, _oracle_chain, _planes, _same

pytestmark = pytest.mark.gpu


def _seq(p, max_pictures):
    s = abi.SeqParams.from_buffer_copy(p.seq)
    s.max_pictures = max_pictures
    return s


def _launches(ctx):
    ctx.sync()
    return {k: v[1] for k, v in ctx.stats(reset=True)["kernels"].items()}


# ------------------------------------------------------------------------------------------------ 1. pictures of at most a few CTUs
@pytest.mark.parametrize("case", gc.SMALL_CASES, ids=gc.case_id)
def test_small_pictures_match_oracle_at_every_stage_and_input_form(oracle, case):
    """a P and a B picture with intra and inter CUs (8x8: one all inter, one all intra): reconstruction, deblocking, SAO, all stages in one
    call, the partition counts; then the same picture through the batch entry with dense and -- 4:0:0 / 4:2:0 -- compact levels and as
    packed input, reconstructed and filtered"""
    import libhm_amd
    for label, p in gc.small_pictures(case):
        what = "%s, %s: " % (gc.case_id(case), label)
        want = _check_all_stages(oracle, p, what=what)
        ref0, ref1, cur = _planes(p, (11, 12, 13))
        forms = [("dense levels", lambda ctx, h: ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs)]))]
        if case[3] in (0, 1):
            compact = libhm_amd.pack_levels(p.seq, p.meta, p.coeffs)
            blob = libhm_amd.pack_input(p.seq, p.meta, p.coeffs)
            forms.append(("compact levels", lambda ctx, h: ctx.decompress_pictures([(h, p.slices, p.meta, compact)])))
            forms.append(("packed input", lambda ctx, h: ctx.decompress_pictures_packed([(h, p.slices, blob, None)])))
        with libhm_amd.Context(_seq(p, 2 + len(forms))) as ctx:
            h0, h1 = ctx.acquire(), ctx.acquire()
            ctx.upload(h0, ref0)
            ctx.upload(h1, ref1)
            sao = abi.sao_array_from_raw(p.sao_raw)
            for name, run in forms:
                h = ctx.acquire()
                ctx.upload(h, cur)
                run(ctx, h)
                _same(ctx.download(h), want[0], what + name + ", reconstruction")
                ctx.filter_pictures([(h, p.pp, sao)])
                _same(ctx.download(h), want[2], what + name + ", filtered")


@pytest.mark.parametrize("case", gc.SMALL_CASES, ids=gc.case_id)
def test_small_pictures_serve_as_references_through_every_margin(oracle, case):
    """picture A decoded and filtered -- SAO on in every CTU (4:0:0 / 4:2:0: the fused filter's border tiles write the margins), SAO off
    (the extension kernel does), cu_transquant_bypass on the whole picture (the fused filter's variant for exempt CUs) --, then pictures
    B whose PUs lie, after clipMv, in A's margins: every one of the eight regions of luma and chroma has a reader"""
    import libhm_amd
    a_of, bs = gc.margin_pictures(case)
    w, h, _, fmt, bd, bdc = case
    got = gc.readers_union(bs)
    assert all(got[plane][r] >= 1 for plane in got for r in REGIONS), got
    ref0 = synth.noise_planes(w, h, bd, 3, fmt, bdc)
    zero = [np.zeros_like(x) for x in ref0]
    with libhm_amd.Context(_seq(bs[0], 3)) as ctx:
        h0, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire()
        assert h0 == 0
        ctx.upload(h0, ref0)
        ctx.set_profiling(True)
        for variant in gc.MARGIN_VARIANTS:
            a = a_of[variant]
            what = "%s, A with %s" % (gc.case_id(case), variant)
            fin = _oracle_chain(oracle, a, zero, [ref0])[2]
            ctx.upload(ha, zero)
            ctx.decompress_slice(ha, 0, a.slice, a.meta, a.coeffs)
            _launches(ctx)
            ctx.filter_picture(ha, a.pp, a.sao_raw)
            ran = _launches(ctx)
            fused = fmt in (0, 1) and variant != "no sao"
            assert ran["filter_fused"] == int(fused), "%s: %s" % (what, ran)
            extended = ran["extend_border"]
            _same(ctx.download(ha), fin, what + ": picture A")
            for k, b in enumerate(bs):
                sl = abi.clone_slice(b.slice)
                sl.ref_pic[0][0] = ha
                want = [x.copy() for x in zero]
                oracle.decompress_ctus(b.seq, [b.slice], b.meta, b.coeffs, want, [fin])
                ctx.upload(hb, zero)
                ctx.decompress_slice(hb, 0, sl, b.meta, b.coeffs)
                _same(ctx.download(hb), want, "%s: picture B%d, predicted from A's margins" % (what, k))
            extended += _launches(ctx)["extend_border"]                # by the filter call or before A's first use as a reference: once
            assert extended == (0 if fused else 1), "%s: %d border extensions" % (what, extended)


# ------------------------------------------------------------------------------------------------ 2. several tiny pictures per call
@pytest.mark.parametrize("bi", [False, True], ids=["P", "B"])
@pytest.mark.parametrize("n", gc.BATCH_NS)
@pytest.mark.parametrize("w,h,log2_ctu", gc.BATCH_SIZES)
def test_batches_of_tiny_pictures_match_oracle(oracle, w, h, log2_ctu, n, bi):
    """n different pictures of 1, 2 or 6 CTUs through hmgpu_decompress_pictures and hmgpu_filter_pictures: n that divide 8 and n that do
    not, ranges of CTUs per workgroup column longer and shorter than a picture; each picture against its own oracle, one launch per kernel
    class and call"""
    import libhm_amd
    pics = gc.batch_pictures(w, h, log2_ctu, n, bi)
    ref0, ref1, cur = _planes(pics[0], (31, 32, 33))
    wants = [_oracle_chain(oracle, p, cur, [ref0, ref1]) for p in pics]
    with libhm_amd.Context(_seq(pics[0], 2 + n)) as ctx:
        h0, h1 = ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        hs = [ctx.acquire() for _ in range(n)]
        for hnd in hs:
            ctx.upload(hnd, cur)
        ctx.set_profiling(True)
        _launches(ctx)
        ctx.decompress_pictures([(hs[i], pics[i].slices, pics[i].meta, pics[i].coeffs) for i in range(n)])
        ran = _launches(ctx)
        any_intra = any(p.intra.any() for p in pics)
        assert (ran["prep"], ran["itx"], ran["mc_luma"], ran["mc_chroma"]) == (1, 1, 1, 1) and ran["intra"] == int(any_intra), ran
        for i in range(n):
            _same(ctx.download(hs[i]), wants[i][0], "picture %d of %d, reconstruction" % (i, n))
        _launches(ctx)
        ctx.filter_pictures([(hs[i], pics[i].pp, abi.sao_array_from_raw(pics[i].sao_raw)) for i in range(n)])
        ran = _launches(ctx)
        assert (ran["filter_fused"], ran["deblock_ver"], ran["deblock_hor"], ran["sao"], ran["extend_border"]) == (1, 0, 0, 0, 0), ran
        for i in range(n):
            _same(ctx.download(hs[i]), wants[i][2], "picture %d of %d, filtered" % (i, n))


# ------------------------------------------------------------------------------------------------ 3. strips
@pytest.mark.parametrize("s", gc.STRIPS, ids=gc.strip_id)
def test_strips_match_oracle(oracle, s):
    """pitches beyond 8192 elements, block coordinates beyond 2048, one CTU column and 1025 of them: all four stages, then a B picture
    whose vectors reach the margins along the strip's long sides"""
    import libhm_amd
    p, far = gc.strip_pictures(s)
    _check_all_stages(oracle, p, seeds=(61, 62, 63), what=gc.strip_id(s) + ": ")
    ref0, ref1, cur = _planes(far, (61, 62, 63))
    want = [a.copy() for a in cur]
    oracle.decompress_ctus(far.seq, far.slices, far.meta, far.coeffs, want, [ref0, ref1])
    with libhm_amd.Context(far.seq) as ctx:
        h0, h1, hc = ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, ref0)
        ctx.upload(h1, ref1)
        ctx.upload(hc, cur)
        _decompress(ctx, hc, far)
        _same(ctx.download(hc), want, gc.strip_id(s) + ", vectors into the margins: reconstruction")


# ------------------------------------------------------------------------------------------------ 4. sixty-four pictures
@pytest.mark.parametrize("w,h,log2_ctu,bd", gc.DPB_CONTEXTS)
def test_references_at_handles_32_and_above(oracle, w, h, log2_ctu, bd):
    """references at handles 0, 31, 32, 33, 62 and 63 of a context of 64 pictures -- uploaded, decoded and finished with SAO (their SAO
    planes are the picture) and decoded and finished without (their reconstruction planes are) on both sides of 32: both words of the SAO
    mask carry set and clear bits --, read by P and B pictures through the picture kernels, the cells kernels and weighted prediction"""
    import libhm_amd
    dec, pics = gc.dpb_pictures(w, h, log2_ctu, bd)
    planes = [None] * 64
    planes[0], planes[32] = synth.noise_planes(w, h, bd, 1), synth.blocky_planes(w, h, bd, 2)
    cur = synth.blocky_planes(w, h, bd, 3)
    with libhm_amd.Context(_seq(pics[0][1], 64)) as ctx:
        assert [ctx.acquire() for _ in range(64)] == list(range(64))
        for hnd in gc.DPB_UPLOADED:
            ctx.upload(hnd, planes[hnd])
        for hnd, p in sorted(dec.items()):
            ctx.upload(hnd, cur)
            _decompress(ctx, hnd, p)
            ctx.filter_picture(hnd, p.pp, p.sao_raw)
            planes[hnd] = _oracle_chain(oracle, p, cur, [planes[0]])[2]
            _same(ctx.download(hnd), planes[hnd], "reference decoded into handle %d" % hnd)
        ctx.set_profiling(True)
        for k, (label, p) in enumerate(pics):
            hc = (5, 40)[k % 2]
            want = [a.copy() for a in cur]
            oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, want, planes)
            ctx.upload(hc, cur)
            _launches(ctx)
            _decompress(ctx, hc, p)
            ran = _launches(ctx)
            assert ran["mc_cells"] == (2 if "cells" in label else 2 * int(cs.wants_cells(p))), (label, ran)
            _same(ctx.download(hc), want, "%s picture in handle %d: reconstruction" % (label, hc))


# ------------------------------------------------------------------------------------------------ 5. the plain-address windows
def _plain_context(seq):
    import libhm_amd
    try:
        return libhm_amd.Context(seq)
    except libhm_amd.HmgpuError as e:
        if e.status in (abi.HMGPU_EDEVICE, abi.HMGPU_ENOMEM):
            pytest.skip("hmgpu_create answers status %d for a context of %.2f GB of planes" % (e.status, gc.slab_bytes(seq) / 1e9))
        raise


def test_plain_address_windows_match_oracle_and_the_buffer_path(oracle):
    """a context whose slab of pictures has 0xffff0000 bytes or more: k_mc_luma and k_mc_chroma run with plain 64-bit addresses instead of
    buffer loads, in all four variants (P, B, weighted, vectors into the margins), from references at handle 0, at the last handle wholly
    below 4 GiB and at the last one, whose final (SAO) luma plane straddles 4 GiB.  Reconstruction against the oracle; the same pictures
    in a context of four pictures (the buffer path) give the same planes.  The last handle's picture is decoded and filtered on the
    device and read back: what the filters make of it is not the subject here, its planes are the oracle's reference as they are."""
    w, h, log2_ctu, bd = gc.PLAIN
    seq = abi.make_seq(w, h, bd, log2_ctu=log2_ctu, max_pictures=gc.PLAIN_PICTURES)
    last, below = gc.PLAIN_PICTURES - 1, gc.PLAIN_PICTURES - 2
    pics = gc.plain_pictures()
    planes = [None] * gc.PLAIN_PICTURES
    planes[0], planes[below] = synth.noise_planes(w, h, bd, 1), synth.blocky_planes(w, h, bd, 2)
    cur = synth.blocky_planes(w, h, bd, 3)
    a = gc.plain_sao_picture()
    got = {}
    with _plain_context(seq) as ctx:
        assert [ctx.acquire() for _ in range(gc.PLAIN_PICTURES)] == list(range(gc.PLAIN_PICTURES))
        ctx.upload(0, planes[0])
        ctx.upload(below, planes[below])
        ctx.upload(last, cur)
        _decompress(ctx, last, a)
        ctx.filter_picture(last, a.pp, a.sao_raw)
        planes[last] = ctx.download(last)
        assert not np.array_equal(planes[last][0], cur[0])
        # the condition of the plain path, from the ABI: the final planes of the first and of the last picture lie so far apart that
        # the slab, one picture stride longer, has kWinLimit bytes or more; the last one's are its SAO set, across 4 GiB
        first_base, nbytes = ctx.device_region(0)
        last_rec = ctx.device_region(below)[0] + 2 * nbytes
        last_base = ctx.device_region(last)[0]
        assert nbytes == gc.plane_set_bytes(seq) and last_base == last_rec + nbytes
        assert last_rec - first_base >= gc.WIN_LIMIT - 2 * nbytes
        assert last_base - first_base < (1 << 32) < last_base - first_base + gc.plane_bytes(seq)[0]
        for label, p in pics:
            ctx.upload(5, cur)
            _decompress(ctx, 5, p)
            got[label] = ctx.download(5)
    for label, p in pics:
        want = [x.copy() for x in cur]
        oracle.decompress_ctus(p.seq, p.slices, p.meta, p.coeffs, want, planes)
        _same(got[label], want, "slab past 4 GiB, %s picture: reconstruction" % label)
    # the buffer path on the same pictures: a context of four pictures, the references at handles 0 .. 2
    import libhm_amd
    with libhm_amd.Context(_seq(pics[0][1], 4)) as ctx:
        hs = [ctx.acquire() for _ in range(4)]
        assert gc.slab_bytes(ctx.seq) < gc.WIN_LIMIT
        for hnd, src in zip(hs, (0, below, last)):
            ctx.upload(hnd, planes[src])
        for label, p in pics:
            sl = abi.clone_slice(p.slice)
            for l in range(2):
                for r in range(int(sl.num_ref_idx[l])):
                    sl.ref_pic[l][r] = {0: hs[0], below: hs[1], last: hs[2]}[int(sl.ref_pic[l][r])]
            ctx.upload(hs[3], cur)
            ctx.decompress_slice(hs[3], 0, sl, p.meta, p.coeffs)
            _same(ctx.download(hs[3]), got[label], "%s picture: the buffer path against the plain one" % label)


# ------------------------------------------------------------------------------------------------ 6. exports on sub-CTU pictures
CANARY = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


class _Decoded:
    """a context with two uploaded references (handles 0 and 1) and the three pictures of gc.export_pictures decoded and filtered into
    handles 2 .. 4, each equal to the oracle's planes (self.fin)"""

    def __init__(self, oracle, w, h, log2_ctu, fmt):
        import libhm_amd
        self.pics = gc.export_pictures(w, h, log2_ctu, fmt)
        self.seq = _seq(self.pics[0], 6)
        self.depths = (10, 10)
        self.refs = [synth.noise_planes(w, h, 10, 5, fmt), synth.blocky_planes(w, h, 10, 6, fmt)]
        cur = synth.blocky_planes(w, h, 10, 7, fmt)
        self.fin = [_oracle_chain(oracle, p, cur, self.refs)[2] for p in self.pics]
        self.ctx = libhm_amd.Context(self.seq)
        try:
            for planes in self.refs:
                self.ctx.upload(self.ctx.acquire(), planes)
            self.hs = [self.ctx.acquire() for _ in self.pics]
            for hnd in self.hs:
                self.ctx.upload(hnd, cur)
            self.ctx.decompress_pictures([(hnd, p.slices, p.meta, p.coeffs) for hnd, p in zip(self.hs, self.pics)])
            for hnd, p, fin in zip(self.hs, self.pics, self.fin):
                self.ctx.filter_picture(hnd, p.pp, p.sao_raw)
                _same(self.ctx.download(hnd), fin, "%dx%d picture in handle %d" % (w, h, hnd))
        except BaseException:
            self.ctx.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.close()


def _tensors(res):
    return list(res.values()) if isinstance(res, dict) else list(res) if isinstance(res, (tuple, list)) else [res]


def _host(t):
    from tests.test_gpu_motion import bits
    import torch
    return t.cpu().numpy() if t.dtype == torch.uint8 else bits(t)


def _one_and_three(call, hs, wants, what):
    """call(pics, out) -> dict or tuple of tensors with a leading batch dimension; wants[i]: the model's arrays of picture i in the same
    order.  One picture and a batch of three (in another order), each once into tensors of the wrapper's own and once into views of
    larger canary-filled tensors -- one batch entry, two rows and three columns more, the view at row 1, column 2: nothing outside
    the views changes"""
    import torch
    for order in ([0], [1], [2], [2, 0, 1]):
        pics = [hs[i] for i in order]
        plain = call(pics, None)
        names = list(plain) if isinstance(plain, dict) else None
        got = _tensors(plain)
        assert len(got) == len(wants[0]), (what, len(got), len(wants[0]))
        for slot, i in enumerate(order):
            for k, t in enumerate(got):
                g, want = _host(t[slot]), np.asarray(wants[i][k])
                assert g.shape == want.shape, (what, order, slot, k, g.shape, want.shape)
                assert np.array_equal(g.astype(np.int64), want.astype(np.int64)), (what, order, slot, names[k] if names else k, int((g != want).sum()))
        bigs, views = [], []
        for t in got:
            h, w = t.shape[-2:]
            big = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:-2]) + (h + 2, w + 3), CANARY[t.element_size()], dtype=t.dtype, device=t.device)
            bigs.append(big)
            views.append(big[(slice(0, t.shape[0]),) + (slice(None),) * (t.dim() - 3) + (slice(1, 1 + h), slice(2, 2 + w))])
        torch.cuda.synchronize()
        call(pics, dict(zip(names, views)) if names else tuple(views))
        torch.cuda.synchronize()
        for k, (t, big, view) in enumerate(zip(got, bigs, views)):
            assert torch.equal(view, t), (what, order, "view", k)
            rest = big.clone()
            rest[(slice(0, t.shape[0]),) + (slice(None),) * (t.dim() - 3) + (slice(1, 1 + t.shape[-2]), slice(2, 2 + t.shape[-1]))] = CANARY[t.element_size()]
            assert bool((rest == CANARY[t.element_size()]).all()), (what, order, "canaries", k)


@pytest.mark.parametrize("fmt", [0, 1, 3])
@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_yuv_and_motion_exports_of_sub_ctu_pictures(oracle, w, h, log2_ctu, fmt):
    """planar YUV at 8 and 10 bits (tests/export_ref.py) and the motion grid (tests/motion_ref.py)"""
    from tests import export_ref, motion_ref
    with _Decoded(oracle, w, h, log2_ctu, fmt) as d:
        for out_bd in (8, 10):
            wants = [[a.reshape(a.shape[0], -1) for a in export_ref.export_yuv(fin, fmt, d.depths, (out_bd, out_bd), export_ref.PLANAR)] for fin in d.fin]
            _one_and_three(lambda pics, out: d.ctx.export_batch(pics, layout="planar", bit_depth=out_bd, out=out), d.hs, wants, "planar %d" % out_bd)
        wants = []
        for p in d.pics:
            m = motion_ref.blocks(p.meta_np, p.slices, w, h, log2_ctu, 3)
            wants.append([m["mv"], m["ref_poc"], m["block"]])
        _one_and_three(lambda pics, out: d.ctx.export_motion(pics, out=out), d.hs, wants, "motion")


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_residual_export_of_sub_ctu_pictures(oracle, w, h, log2_ctu, fmt):
    from tests import residual_ref
    with _Decoded(oracle, w, h, log2_ctu, fmt) as d:
        ncomp = 1 if fmt == 0 else 3
        wants = [residual_ref.planes(d.seq, p.slices, p.meta_np, p.coeffs.arrays)[:ncomp] for p in d.pics]
        assert all(a.any() for want in wants for a in want)
        _one_and_three(lambda pics, out: d.ctx.export_residual(pics, out=out), d.hs, wants, "residual")


@pytest.mark.parametrize("fmt", [1, 3])
@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_transform_export_of_sub_ctu_pictures(oracle, w, h, log2_ctu, fmt):
    """levels, coefficients and the info grid; a chroma row of an 8-wide 4:2:0 picture is half of the kernel's 16-byte segments"""
    from tests import transform_ref
    with _Decoded(oracle, w, h, log2_ctu, fmt) as d:
        for value in ("levels", "coeffs"):
            wants = []
            for p in d.pics:
                planes = transform_ref.levels_planes(d.seq, p.meta_np, p.coeffs.arrays) if value == "levels" else \
                    transform_ref.coeff_planes(d.seq, p.slices, p.meta_np, p.coeffs.arrays)
                assert all(a.any() for a in planes)
                wants.append(list(planes) + [transform_ref.info_grid(d.seq, p.meta_np)])
            _one_and_three(lambda pics, out: d.ctx.export_transform(pics, value, out=out), d.hs, wants, value)


@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_loopfilter_export_of_sub_ctu_pictures(oracle, w, h, log2_ctu):
    """the edge grid and the SAO grid (one CTB)"""
    from tests import loopfilter_ref
    with _Decoded(oracle, w, h, log2_ctu, 1) as d:
        wants = [list(loopfilter_ref.picture_model(oracle, p)) for p in d.pics]
        assert any((want[0][:2] > 0).any() for want in wants) or (w, h) == (8, 8)
        _one_and_three(lambda pics, out: d.ctx.export_loopfilter(pics, out=out), d.hs, wants, "loop filter")


@pytest.mark.parametrize("w,h,log2_ctu", gc.EXPORT_CASES)
def test_metrics_maps_and_histograms_of_sub_ctu_pictures(oracle, w, h, log2_ctu):
    """every decoded picture against reference 0: the records with SSIM -- the 4x4 chroma planes of an 8x8 picture have no window, as
    include/hmgpu.h says --, the maps at blocks of 8 and of 64, the latter into a padded canary-filled destination too, and the
    histograms of Y, Cb, Cr and maxRGB with their records"""
    import torch
    from libhm_amd import metrics
    from tests import histogram_ref, metrics_map_ref, metrics_ref
    from tests import test_gpu_histogram as th
    from tests import test_gpu_metrics as tm
    from tests import test_gpu_metrics_map as tmm
    with _Decoded(oracle, w, h, log2_ctu, 1) as d:
        for order in ([0], [2, 0, 1]):
            pics, fins, n = [d.hs[i] for i in order], [d.fin[i] for i in order], len(order)
            want = [metrics_ref.picture(fin, d.refs[0], 1, d.depths) for fin in fins]
            rec = tm.check(d.ctx.metrics(pics, ref_pics=[0] * n, ssim=True), want, "metrics %s" % order)
            if (w, h) == (8, 8):
                assert all(want[i][k]["ssim_windows"] == 0 and int(rec[i, k, metrics_ref.FIELDS.index("ssim_windows")]) == 0 and
                           int(rec[i, k, metrics_ref.FIELDS.index("ssim_q32")]) == 0 for i in range(n) for k in (1, 2))
                assert all(want[i][0]["ssim_windows"] == 1 for i in range(n))
            for block in (8, 64):
                wmap = tmm.model(fins, [d.refs[0]] * n, 1, d.depths, block)
                tmm.check(d.ctx.metrics_map(pics, ref_pics=[0] * n, block=block), wmap, "maps %d %s" % (block, order))
                nbx, nby = metrics_map_ref.grid(w, h, block)
                pitch, fstride = nbx + 3, (nbx + 3) * nby + 5
                bstride = fstride * 6 + 7
                per = 11 + n * bstride
                base = [11 + k * per for k in range(3)]
                buf = torch.full((3 * per + 11,), tmm.CAN, dtype=torch.int64, device="cuda")
                tmm.raw_call(d.ctx, pics, [0] * n, block, (0, 1, 2), True, buf, base, pitch, fstride, bstride)
                torch.cuda.synchronize()
                host = buf.cpu().numpy()
                got, written = np.zeros_like(wmap), np.zeros(host.shape, bool)
                for k in range(3):
                    for i in range(n):
                        for f in range(6):
                            for y in range(nby):
                                s = base[k] + i * bstride + f * fstride + y * pitch
                                got[i, k, f, y] = host[s:s + nbx]
                                written[s:s + nbx] = True
                tmm.compare(got, wmap, "padded maps %d %s" % (block, order))
                assert (host[~written] == tmm.CAN).all() and written.sum() == wmap.size
            coef = th.coef_of(d.seq)
            whist = [histogram_ref.picture(fin, 1, d.depths, (0, 1, 2, 3), coef=coef) for fin in fins]
            th.check(d.ctx.histogram(pics, channels=th.ALL), whist, "histogram %s" % order)
