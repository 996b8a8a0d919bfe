"""GPU: hmgpu_pictures_conceal against tests/conceal_ref.py, plane for plane and sample for sample -- COPY, fill and MOTION on noise and
on decoded pictures, every chroma format, partial CTUs, destinations and sources that went through SAO and ones that did not, calls of
16 jobs, the margins behind a concealed picture, and the refusals of include/hmgpu.h "error concealment"."""
import numpy as np
import pytest

from libhm_amd import abi
from tests import conceal_ref as cr
from tests import geometry_cases as gc
from tests import synth
from tests.test_gpu_formats_fullsize import _decompress, _same

pytestmark = pytest.mark.gpu

SIZES = [(8, 8, 4), (72, 40, 6), (208, 120, 4), (208, 120, 5)]                  # (width, height, log2 CTU size)
CASES = [s + (f, bd, bd) for s in SIZES for f in (0, 1, 2, 3) for bd in (8, 10)] + [(208, 120, 4, 1, 12, 10)]


def _id(c):
    return "%dx%d-ctu%d-fmt%d-bd%d-%d" % (c[0], c[1], 1 << c[2], c[3], c[4], c[5])


def _masks(cw, ch):
    """none, all (as a mask), the four corner CTUs, a checkerboard, one interior CTU (the nearest to one there is)"""
    n = cw * ch
    a = np.arange(n)
    x, y = a % cw, a // cw
    corners = ((x == 0) | (x == cw - 1)) & ((y == 0) | (y == ch - 1))
    one = np.zeros(n, bool)
    one[min(ch - 1, 1) * cw + min(cw - 1, 1)] = True
    return [("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("corners", corners), ("checkerboard", (x + y) % 2 == 0), ("one", one)]


def _seq(case, max_pictures):
    w, h, lc, f, bd, bdc = case
    s = abi.make_seq(w, h, bd, bdc, log2_ctu=lc, max_pictures=max_pictures)
    s.chroma_format = f
    return s


def _decoded(ctx, case, seed, bi=False, sao=True, **kw):
    """a picture decoded from reference handle 0 into a new handle and filtered (sao: its final planes are the SAO planes)"""
    w, h, lc, f, bd, bdc = case
    p = synth.make_picture(w, h, bd, seed=seed, bi=bi, ref_handles=([0], [0]), sao=sao, chroma_format=f, log2_ctu=lc, bit_depth_chroma=bdc, **kw)
    hnd = ctx.acquire()
    ctx.upload(hnd, synth.noise_planes(w, h, bd, 1000 + seed, f, bdc))
    _decompress(ctx, hnd, p)
    ctx.filter_picture(hnd, p.pp, p.sao_raw)
    return hnd, p


def _model(case, dst, src, mask, mode=cr.COPY, **kw):
    return cr.conceal(dst, src, mask, mode, case[2], case[3], (case[4], case[5]), **kw)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_copy_and_fill_match_the_model(case):
    """every mask, into a destination that went through SAO and one that did not, from a source of either kind and from no source"""
    import libhm_amd
    w, h, lc, f, bd, bdc = case
    S = 1 << lc
    cw, chh = (w + S - 1) // S, (h + S - 1) // S
    with libhm_amd.Context(_seq(case, 6)) as ctx:
        h0 = ctx.acquire()
        ctx.upload(h0, synth.noise_planes(w, h, bd, 1, f, bdc))
        src_sao, _ = _decoded(ctx, case, 5)
        src_up = ctx.acquire()
        ctx.upload(src_up, synth.noise_planes(w, h, bd, 2, f, bdc))
        dst_sao, _ = _decoded(ctx, case, 6)
        dst_up = ctx.acquire()
        ctx.upload(dst_up, synth.noise_planes(w, h, bd, 3, f, bdc))
        planes = {k: ctx.download(k) for k in (src_sao, src_up, dst_sao, dst_up)}
        assert not np.array_equal(planes[src_sao][0], planes[dst_sao][0])
        top = [(1 << bd) - 1, 0, (1 << bdc) - 1]
        k = 0
        for name, mask in _masks(cw, chh):
            for dst in (dst_sao, dst_up):
                for src, fill in ((src_sao, None), (src_up, None), (None, (-1, -1, -1)), (None, top)):
                    k += 1
                    job = dict(dst=dst, src=src, mode="copy" if k % 2 else "motion", mask=None if name == "all" and k % 3 else mask)
                    if fill is not None:
                        job["fill"] = fill
                    before = ctx.concealed_ctus(dst)
                    ctx.conceal([job])
                    want = _model(case, planes[dst], None if src is None else planes[src], mask, fill=fill or (-1, -1, -1))
                    got = ctx.download(dst)
                    _same(got, want, "%s, mask %s, dst %d, src %s" % (_id(case), name, dst, src))
                    planes[dst] = got
                    assert ctx.concealed_ctus(dst) >= max(before, int(mask.sum()))
        assert ctx.concealed_ctus(dst_up) == cw * chh and ctx.concealed_ctus(src_up) == 0
        for k in (src_sao, src_up):
            _same(ctx.download(k), planes[k], "source %d is left alone" % k)
        ctx.release(dst_up)
        assert ctx.acquire() == dst_up and ctx.concealed_ctus(dst_up) == 0      # acquire resets the count


def test_sixteen_jobs_in_one_call_and_a_shared_source():
    import libhm_amd
    case = (208, 120, 4, 1, 10, 10)
    w, h, lc, f, bd, bdc = case
    n = 13 * 8
    rng = np.random.RandomState(7)
    with libhm_amd.Context(_seq(case, 18)) as ctx:
        srcs = [ctx.acquire(), ctx.acquire()]
        dsts = [ctx.acquire() for _ in range(16)]
        planes = {}
        for k in srcs + dsts:
            planes[k] = synth.noise_planes(w, h, bd, 20 + k, f, bdc)
            ctx.upload(k, planes[k])
        jobs, masks = [], []
        for i, d in enumerate(dsts):
            masks.append(rng.rand(n) < (i + 1) / 17.0)
            jobs.append(dict(dst=d, src=None if i % 5 == 4 else srcs[i % 2], mode="copy", mask=masks[-1], fill=(i, -1, 3 * i)))
        ctx.conceal(jobs)
        for i, d in enumerate(dsts):
            src = jobs[i]["src"]
            want = _model(case, planes[d], None if src is None else planes[src], masks[i], fill=jobs[i]["fill"])
            _same(ctx.download(d), want, "job %d of 16" % i)
            assert ctx.concealed_ctus(d) == int(masks[i].sum())
        # two jobs, one source
        ctx.conceal([dict(dst=dsts[0], src=srcs[0]), dict(dst=dsts[1], src=srcs[0])])
        for d in dsts[:2]:
            _same(ctx.download(d), planes[srcs[0]], "two jobs share a source")


MARGIN_CASES = [c for c in gc.SMALL_CASES if (c[0], c[1]) in ((8, 8), (24, 40), (72, 64)) and (c[2], c[3]) in ((4, 1), (6, 1), (5, 2), (4, 3), (6, 0))]


@pytest.mark.parametrize("case", MARGIN_CASES, ids=gc.case_id)
def test_margins_of_a_concealed_picture(oracle, case):
    """picture A, whose margins are up to date for its old samples -- as a decoded and filtered picture, and as an uploaded one that has
    served as a reference --, has its border CTUs concealed; P pictures whose PUs lie in A's margins on all sides then equal the oracle
    given the model's planes"""
    import libhm_amd
    w, h, lc, f, bd, bdc = case
    S = 1 << lc
    cw, chh = (w + S - 1) // S, (h + S - 1) // S
    a_of, bs = gc.margin_pictures(case)
    a = np.arange(cw * chh)
    border = (a % cw == 0) | (a % cw == cw - 1) | (a // cw == 0) | (a // cw == chh - 1)
    zero = [np.zeros_like(x) for x in synth.noise_planes(w, h, bd, 3, f, bdc)]
    seq = abi.SeqParams.from_buffer_copy(bs[0].seq)
    seq.max_pictures = 4
    with libhm_amd.Context(seq) as ctx:
        h0, hs, ha, hb = ctx.acquire(), ctx.acquire(), ctx.acquire(), ctx.acquire()
        ctx.upload(h0, synth.noise_planes(w, h, bd, 3, f, bdc))
        src = synth.noise_planes(w, h, bd, 4, f, bdc)
        ctx.upload(hs, src)
        for variant in ("decoded", "uploaded"):
            if variant == "decoded":
                p = a_of["sao"]
                ctx.upload(ha, zero)
                ctx.decompress_slice(ha, 0, p.slice, p.meta, p.coeffs)
                ctx.filter_picture(ha, p.pp, p.sao_raw)
            else:
                ctx.upload(ha, synth.noise_planes(w, h, bd, 5, f, bdc))
            sl = abi.clone_slice(bs[0].slice)
            sl.ref_pic[0][0] = ha
            ctx.upload(hb, zero)
            ctx.decompress_slice(hb, 0, sl, bs[0].meta, bs[0].coeffs)       # (A's margins are now those of its old samples)
            fin = _model(case, ctx.download(ha), src, border)
            ctx.conceal([dict(dst=ha, src=hs, mask=border)])
            _same(ctx.download(ha), fin, "%s, %s: concealed picture" % (gc.case_id(case), variant))
            for k, b in enumerate(bs):
                sl = abi.clone_slice(b.slice)
                sl.ref_pic[0][0] = ha
                want = [x.copy() for x in zero]
                oracle.decompress_ctus(b.seq, [b.slice], b.meta, b.coeffs, want, [fin])
                ctx.upload(hb, zero)
                ctx.decompress_slice(hb, 0, sl, b.meta, b.coeffs)
                _same(ctx.download(hb), want, "%s, %s: picture B%d, predicted from the concealed picture's margins" % (gc.case_id(case), variant, k))


MOTION_CASES = [(208, 120, 4, 1, 8, 8), (208, 120, 5, 2, 10, 10), (72, 40, 6, 3, 10, 10), (208, 120, 6, 0, 10, 10), (200, 120, 5, 1, 10, 10)]
# (src_poc, dst_poc) against reference POCs 100 (list 0) and 200 (list 1): tb == td, tb == 2 td, tb == -td, td clipped at both ends, td == 0
POCS = [(104, 108), (104, 112), (104, 100), (-200, -190), (400, 410), (100, 107)]


@pytest.mark.parametrize("case", MOTION_CASES, ids=_id)
def test_motion_copy_matches_the_model(case):
    """a P and a B picture decoded into source handles; a checkerboard of an uploaded destination concealed from each at every POC pair;
    an uploaded source (no side information) gives the COPY result; a handle that held the B picture and now holds a P picture reads no
    list-1 value"""
    import libhm_amd
    from tests import motion_ref
    w, h, lc, f, bd, bdc = case
    S = 1 << lc
    cw, chh = (w + S - 1) // S, (h + S - 1) // S
    a = np.arange(cw * chh)
    checker = (a % cw + a // cw) % 2 == 0
    with libhm_amd.Context(_seq(case, 6)) as ctx:
        h0 = ctx.acquire()
        ctx.upload(h0, synth.noise_planes(w, h, bd, 1, f, bdc))
        hp, pp = _decoded(ctx, case, 11, intra_frac=0.2)
        hb, pb = _decoded(ctx, case, 12, bi=True, sao=False, intra_frac=0.2, num_slices=2 if cw * chh > 2 else 1)
        dst = ctx.acquire()
        start = synth.noise_planes(w, h, bd, 9, f, bdc)
        sides = set()
        for hnd, p in ((hp, pp), (hb, pb)):
            src = ctx.download(hnd)
            grid = motion_ref.grid(p.meta_np, p.slices, w, h, lc)
            assert grid["used"][0].any() and (p is pp or (grid["used"][1] & ~grid["used"][0]).any())
            for src_poc, dst_poc in POCS:
                ctx.upload(dst, start)
                ctx.conceal([dict(dst=dst, src=hnd, mode="motion", mask=checker, src_poc=src_poc, dst_poc=dst_poc)])
                want = _model(case, start, src, checker, cr.MOTION, src_poc=src_poc, dst_poc=dst_poc, grid=grid)
                _same(ctx.download(dst), want, "%s, source %d, POCs %d -> %d" % (_id(case), hnd, src_poc, dst_poc))
                dx, dy = cr.displacements(grid, w, h, src_poc, dst_poc)
                by, bx = np.mgrid[0:dx.shape[0], 0:dx.shape[1]]
                sides |= {s for s, hit in (("left", (8 * bx + dx < 0).any()), ("right", (8 * bx + 7 + dx > w - 1).any()),
                                           ("above", (8 * by + dy < 0).any()), ("below", (8 * by + 7 + dy > h - 1).any())) if hit}
        assert sides == {"left", "right", "above", "below"}, sides          # clamping acted on every border
        # no side information: the COPY result
        up = ctx.acquire()
        src = synth.noise_planes(w, h, bd, 10, f, bdc)
        ctx.upload(up, src)
        ctx.upload(dst, start)
        ctx.conceal([dict(dst=dst, src=up, mode="motion", mask=checker, src_poc=104, dst_poc=112)])
        _same(ctx.download(dst), _model(case, start, src, checker), "motion copy from an uploaded source")
        # the B picture's handle now holds a P picture: its list-1 arrays still hold the B picture's values and are not read
        p2 = synth.make_picture(w, h, bd, seed=13, ref_handles=([0], [0]), chroma_format=f, log2_ctu=lc, bit_depth_chroma=bdc)
        ctx.upload(hb, start)
        _decompress(ctx, hb, p2)
        src = ctx.download(hb)
        grid = motion_ref.grid(p2.meta_np, p2.slices, w, h, lc)
        ctx.upload(dst, start)
        ctx.conceal([dict(dst=dst, src=hb, mode="motion", src_poc=104, dst_poc=112)])
        _same(ctx.download(dst), _model(case, start, src, None, cr.MOTION, src_poc=104, dst_poc=112, grid=grid), "P picture in a B picture's handle")


def test_refusals_leave_the_destination_untouched():
    import libhm_amd
    case = (72, 40, 5, 1, 10, 8)
    w, h, lc, f, bd, bdc = case
    n = 3 * 2
    with libhm_amd.Context(_seq(case, 5)) as ctx:
        a, b, c = ctx.acquire(), ctx.acquire(), ctx.acquire()
        planes = {k: synth.noise_planes(w, h, bd, 40 + k, f, bdc) for k in (a, b, c)}
        for k in planes:
            ctx.upload(k, planes[k])
        ok = dict(dst=a, src=b)
        high = np.zeros(1, np.uint8)
        high[0] = 1 << n                                                        # CTU 6 of 6
        bad = [("n = 0", []), ("n = 17", [ok] * 17), ("dst invalid", [dict(dst=7, src=b)]), ("dst not acquired", [dict(dst=3, src=b)]),
               ("src not acquired", [dict(dst=a, src=3)]), ("src = -2", [dict(dst=a, src=-2)]), ("dst == src", [dict(dst=a, src=a)]),
               ("two writers", [ok, dict(dst=a, src=c)]), ("dst is another job's src", [ok, dict(dst=c, src=a)]),
               ("mode 2", [dict(dst=a, src=b, mode=2)]), ("mode -1", [dict(dst=a, src=b, mode=-1)]), ("mask bit beyond", [dict(dst=a, src=b, mask=high)]),
               ("luma fill", [dict(dst=a, fill=(1024, 0, 0))]), ("chroma fill", [dict(dst=a, fill=(0, 0, 256))]),
               ("reserved", [dict(dst=a, src=b, reserved=(0, 0, 0, 1))])]
        for what, jobs in bad:
            for check_only in (True, False):
                assert ctx.conceal_status(jobs, check_only=check_only) == abi.HMGPU_EINVAL, what
        for k in planes:
            _same(ctx.download(k), planes[k], "after the refusals, picture %d" % k)
            assert ctx.concealed_ctus(k) == 0
        assert ctx.conceal_status([ok, dict(dst=c, src=b, fill=(1023, 255, 255))], check_only=True) == abi.HMGPU_OK
        _same(ctx.download(a), planes[a], "hmgpu_conceal_check enqueues nothing")
        # 4:0:0: the chroma fills are not looked at
    mono = (72, 40, 5, 0, 8, 8)
    with libhm_amd.Context(_seq(mono, 2)) as ctx:
        a = ctx.acquire()
        assert ctx.conceal_status([dict(dst=a, fill=(255, 4096, 4096))], check_only=True) == abi.HMGPU_OK
        assert ctx.conceal_status([dict(dst=a, fill=(256, 0, 0))], check_only=True) == abi.HMGPU_EINVAL
