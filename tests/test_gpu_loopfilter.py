"""Loop-filter export on the GPU (hmgpu_pictures_export_loopfilter, k_lfinfo.hip) behind Context.export_loopfilter, and through libhmdec:
the edge grid, the SAO grid and the dense form, every element equal to the model (tests/loopfilter_ref.py: the oracle's boundary
strengths and SAO parameters, the tc / beta tables of the standard).  No tolerance anywhere: the values are integers."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec, loopfilter
from tests import bs_ref
from tests import golden_util as gu
from tests import loopfilter_ref as lref
from tests import synth
from tests.test_gpu_motion import _hip

pytestmark = pytest.mark.gpu

W, H = 520, 328
CANARY = 0x5A
MERGE_LEFT, MERGE_ABOVE = 0, 1          # HMGPU_SAO_MERGE_LEFT / ABOVE


def _torch():
    import torch
    return torch


def motion_picture(fmt, bi):
    """the pictures of tests/test_gpu_filter_controls.py: P or B, 10 % intra CUs, few coded blocks, motion that spreads over
    neighbouring PUs, two references in swapped lists -- Bs 0, 1 by motion, 1 by references and 2 all occur in hundreds of units"""
    return synth.make_picture(W, H, 10, seed=0xC0 + 2 * fmt + int(bi), bi=bi, intra_frac=0.1, cbf_prob=0.2, mv_coherence=0.7, num_refs=2,
                              l1_refs=2 if bi else 1, ref_handles=([0, 1], [1, 0]), chroma_format=fmt)


def small_picture(seed, fmt=1, log2_ctu=6, bd=10, bdc=None, w=136, h=72, **kw):
    kw.setdefault("intra_frac", 0.3)
    kw.setdefault("cbf_prob", 0.3)
    kw.setdefault("mv_coherence", 0.5)
    return synth.make_picture(w, h, bd, seed=seed, bi=True, num_refs=2, ref_handles=([0, 1], [1]), chroma_format=fmt, log2_ctu=log2_ctu,
                              bit_depth_chroma=bdc, **kw)


class Ctx:
    """a context with two uploaded reference pictures (handles 0 and 1)"""

    def __init__(self, seq):
        self.seq = seq
        self.ctx = libhm_amd.Context(seq)
        self.ncomp = 1 if seq.chroma_format == 0 else 3
        for k in range(2):
            h = self.ctx.acquire()
            assert h == k
            self.ctx.upload(h, synth.noise_planes(seq.width, seq.height, seq.bit_depth_luma, 5 + k, seq.chroma_format, seq.bit_depth_chroma))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.__exit__(*a)

    def decode(self, p, h=None, stages=7):
        """decompress p into h (a new handle when None) and run the loop filter (stages None: no filter call)"""
        h = self.ctx.acquire() if h is None else h
        self.ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs)])
        if stages is not None:
            self.ctx.filter_picture(h, p.pp, p.sao_raw, stages=stages)
        return h

    def check_grids(self, h, edge, sao, where=""):
        got = self.ctx.export_loopfilter([h])
        assert sorted(got) == ["edge", "sao"], where
        _same_edge(got["edge"][0], edge, where)
        s = got["sao"][0].cpu().numpy()
        assert s.dtype == np.int8 and s.shape == sao.shape, where
        for c in range(self.ncomp):                                  # (4:0:0: the chroma components are not written)
            assert np.array_equal(s[c], sao[c]), (where, "sao", c, [int((s[c, k] != sao[c, k]).sum()) for k in range(6)])
        return got


def _same_edge(t, edge, where=""):
    g = t.cpu().numpy()
    assert g.dtype == np.int16 and g.shape == edge.shape, (where, g.shape, edge.shape)
    bad = [(loopfilter.edge_names[k], int((g[k] != edge[k]).sum())) for k in range(13) if not np.array_equal(g[k], edge[k])]
    assert not bad, (where, bad)


def _status(fn):
    try:
        fn()
    except libhm_amd.HmgpuError as e:
        return e.status
    return abi.HMGPU_OK


# ------------------------------------------------------------------------------------------------ 1. every Bs case
@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("fmt", [1, 2, 3])
def test_every_bs_case_matches_the_model(oracle, fmt, bi):
    p = motion_picture(fmt, bi)
    counts = bs_ref.motion_units(p, *oracle.boundary_strengths(p.seq, p.slices, p.meta, p.pp))
    print("inter PU edge units:", counts)
    for k in ("Bs 0", "Bs 1 by motion", "Bs 1 by references"):
        assert counts[k] >= 100, (k, counts)
    edge, sao = lref.picture_model(oracle, p)
    for d in (0, 1):
        assert all((edge[lref.BS + d] == v).sum() >= 100 for v in (1, 2)) and (edge[lref.TC_CB + d] > 0).any()
    with Ctx(p.seq) as c:
        h = c.decode(p)
        got = c.check_grids(h, edge, sao, (fmt, bi))
        mask = loopfilter.edge_mask(got["edge"])
        assert mask.dtype == _torch().bool and np.array_equal(mask[0].cpu().numpy(), edge[:2] > 0)
        # the edge grid alone, before the picture was filtered: it needs no filter call
        h2 = c.decode(p, stages=None)
        one = c.ctx.export_loopfilter([h2, h], grids=("edge",))
        assert sorted(one) == ["edge"]
        _same_edge(one["edge"][0], edge)
        _same_edge(one["edge"][1], edge)
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 2. formats, CTU sizes, bit depths
@pytest.mark.parametrize("fmt,log2_ctu,bd,bdc", [(0, 6, 10, 10), (1, 4, 10, 10), (1, 5, 10, 10), (1, 6, 8, 8), (1, 6, 12, 12), (1, 6, 12, 10),
                                                 (2, 4, 10, 10), (3, 5, 10, 10)])
def test_formats_ctu_sizes_and_bit_depths(oracle, fmt, log2_ctu, bd, bdc):
    p = small_picture(0x2F0 + 16 * fmt + log2_ctu + bd + bdc, fmt, log2_ctu, bd, bdc, num_slices=2)
    edge, sao = lref.picture_model(oracle, p)
    assert (edge[lref.TC:lref.TC + 2] > 0).any() and (edge[lref.BETA:lref.BETA + 2] > 0).any()
    assert bool((edge[lref.TC_CB:] [:4] > 0).any()) == (fmt != 0)
    with Ctx(p.seq) as c:
        h = c.decode(p)
        c.check_grids(h, edge, sao, (fmt, log2_ctu, bd, bdc))
        # a crop in whole 8x8 areas, off the 64-sample squares the workgroups walk
        got = c.ctx.export_loopfilter([h], grids=("edge",), crop=(8, 24, 16, 8))
        _same_edge(got["edge"][0], edge[:, 4:edge.shape[1] - 2, 2:edge.shape[2] - 6], "crop")
        if fmt == 0:
            # the chroma components of the SAO grid stay untouched
            torch = _torch()
            out = {"sao": torch.full((1,) + sao.shape, CANARY, dtype=torch.int8, device="cuda")}
            c.ctx.export_loopfilter([h], grids=("sao",), out=out)
            s = out["sao"][0].cpu().numpy()
            assert np.array_equal(s[0], sao[0]) and (s[1:] == CANARY).all() and (sao[0, 0] >= 0).any()
            assert (edge[lref.TC_CB:lref.FLAGS] == 0).all()
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 3. slice constants
def _three_slices(lf_across_slices):
    """three slices whose fields are set here, before the oracle and the device see them: the first with deblocking disabled, the
    other two with tc / beta offsets of both signs; PPS chroma offsets non-zero everywhere"""
    p = synth.make_picture(W, H, 10, seed=0x351, bi=True, intra_frac=0.4, cbf_prob=0.4, num_refs=2, ref_handles=([0, 1], [1]), num_slices=3,
                           lf_across_slices=lf_across_slices)
    for sl, (dis, tc, beta, cb, cr) in zip(p.slices, ((1, 1, -1, 1, 1), (0, 2, -2, 3, -4), (0, -2, 2, -5, 2))):
        sl.deblocking_disable, sl.tc_offset_div2, sl.beta_offset_div2, sl.pps_cb_qp_offset, sl.pps_cr_qp_offset = dis, tc, beta, cb, cr
        assert sl.lf_across_slices == lf_across_slices
    return p


def _border_units(p, edge, d):
    """per direction: (slice of every block's CTU, the same of its P side, mask of the filtered units whose two sides lie in different slices)"""
    parts = np.asarray(p.meta_np["qp"]).shape[1]
    sl = lref.raster(p.seq, np.repeat(np.asarray(p.meta_np["slice_idx"], dtype=np.int64)[:, None], parts, axis=1))
    slp = np.full_like(sl, -1)
    if d == 0:
        slp[:, 1:] = sl[:, :-1]
    else:
        slp[1:, :] = sl[:-1, :]
    return sl, slp, (slp >= 0) & (sl != slp)


def test_slice_constants_are_those_of_the_q_side(oracle):
    # lf_across_slices = 0: no unit on a slice border is filtered; everything else carries its own slice's constants
    p = _three_slices(0)
    edge, sao = lref.picture_model(oracle, p)
    sl0 = _border_units(p, edge, 0)[0]
    assert (edge[lref.BS:lref.BS + 2][:, sl0 == 0] == 0).all() and all((edge[lref.BS][sl0 == k] > 0).any() for k in (1, 2))
    for d in (0, 1):
        assert (edge[lref.BS + d][_border_units(p, edge, d)[2]] == 0).all()
    with Ctx(p.seq) as c:
        c.check_grids(c.decode(p), edge, sao, "across 0")
        # the same slices with filtering across their borders: a unit on each border comes out with the Q side's constants, which
        # differ from what the P side's would give
        q = _three_slices(1)
        edge, sao = lref.picture_model(oracle, q)
        qp = edge[lref.QP:lref.QP + 2].astype(np.int64)
        for k in (1, 2):
            seen = 0
            for d in (0, 1):
                sl, slp, border = _border_units(q, edge, d)
                sel = border & (sl == k) & (edge[lref.BS + d] > 0)
                own, other = q.slices[k], q.slices[k - 1]
                tc = lambda s: lref.TC_TABLE[np.clip(qp[d] + 2 * (edge[lref.BS + d].astype(np.int64) - 1) + 2 * s.tc_offset_div2, 0, 53)] << 2
                beta = lambda s: lref.BETA_TABLE[np.clip(qp[d] + 2 * s.beta_offset_div2, 0, 51)] << 2
                assert np.array_equal(edge[lref.TC + d][sel], tc(own)[sel]) and np.array_equal(edge[lref.BETA + d][sel], beta(own)[sel])
                seen += int((beta(own)[sel] != beta(other)[sel]).sum())
            assert seen > 0, k
        c.check_grids(c.decode(q), edge, sao, "across 1")
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 4. exemptions
def _with_pcm_and_lossless(p, seed):
    """some intra 2Nx2N CUs become PCM CUs and some other CUs lossless"""
    m = dict(p.meta_np)
    n, parts = m["depth"].shape
    rng = np.random.RandomState(seed)
    z = np.arange(parts)[None, :]
    cu_first = z & ~((parts >> (2 * m["depth"].astype(np.int64))) - 1)
    per_cu = lambda r: np.take_along_axis(r, cu_first, axis=1)
    decoded = m["part_size"] != abi.SIZE_NONE
    pcm = (per_cu(rng.rand(n, parts)) < 0.5) & decoded & (m["pred_mode"] == abi.MODE_INTRA) & (m["part_size"] == abi.SIZE_2Nx2N) & (m["depth"] >= 1)
    m["ipcm"] = pcm.astype(np.uint8)
    m["tr_idx"] = np.where(pcm, 0, m["tr_idx"])
    for k in ("cbf_y", "cbf_u", "cbf_v"):
        m[k] = np.where(pcm, 1, m[k])
    m["bypass"] = ((per_cu(rng.rand(n, parts)) < 0.3) & decoded & ~pcm).astype(np.uint8)
    p.meta_np, p.meta = m, abi.MetaHolder(m)
    bd = [p.seq.bit_depth_luma, p.seq.bit_depth_chroma, p.seq.bit_depth_chroma]
    p.coeffs = abi.CoeffHolder(*p.coeffs.arrays, pcm=[rng.randint(0, 1 << bd[k], size=p.coeffs.arrays[k].shape).astype(np.int16) for k in range(3)])
    return p


def test_exempt_sides_of_lossless_and_pcm_cus(oracle):
    p = small_picture(0x4E1, w=264, h=136, intra_frac=0.5)
    p.seq.pcm_bit_depth_luma, p.seq.pcm_bit_depth_chroma, p.seq.pcm_loop_filter_disable = 10, 10, 1
    _with_pcm_and_lossless(p, 7)
    assert p.meta_np["ipcm"].any() and p.meta_np["bypass"].any()
    edge, sao = lref.picture_model(oracle, p)
    f = edge[lref.FLAGS].astype(np.int64)
    for d in (0, 1):
        sides = (f >> (2 * d)) & 3
        assert all((sides == v).any() for v in (0, 1, 2, 3)), d              # exempt P, exempt Q, both, neither
    # without pcm_loop_filter_disabled the PCM CUs are filtered like any other: fewer flags
    with Ctx(p.seq) as c:
        c.check_grids(c.decode(p), edge, sao, "exempt")
        c.ctx.sync()
    p.seq.pcm_loop_filter_disable = 0
    plain = lref.picture_model(oracle, p)[0]
    assert (plain[lref.FLAGS] != 0).sum() < (edge[lref.FLAGS] != 0).sum() and (plain[lref.FLAGS] != 0).any()
    with Ctx(p.seq) as c:
        c.check_grids(c.decode(p), plain, sao, "pcm filtered")
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 5. SAO
def test_sao_types_merges_and_offset_shift(oracle):
    p = small_picture(0x5A0, w=W, h=H, num_slices=2)
    n, cw = p.num_ctus, p.ctus_w
    sidx = np.asarray(p.meta_np["slice_idx"])
    left = [a for a in range(n) if a % cw and sidx[a] == sidx[a - 1]][::5]
    above = [a for a in range(n) if a >= cw and sidx[a] == sidx[a - cw] and a not in left][::7]
    assert len(left) >= 3 and len(above) >= 2
    for a in left:
        p.sao_raw[a, :, :] = 0
        p.sao_raw[a, :, 0], p.sao_raw[a, :, 1] = abi.SAO_MERGE, MERGE_LEFT
    for a in above:
        p.sao_raw[a, :, :] = 0
        p.sao_raw[a, :, 0], p.sao_raw[a, :, 1] = abi.SAO_MERGE, MERGE_ABOVE
    p.pp = abi.make_pic_params(sao_enabled=1, sao_offset_shift=(1, 2))
    edge, sao = lref.picture_model(oracle, p)
    flat = sao.reshape(3, 6, -1)
    assert sorted(set(int(v) for v in flat[0, 0])) == [-1, 0, 1, 2, 3, 4]                     # every SAO type, and off
    for a in left:
        assert np.array_equal(flat[:, :, a], flat[:, :, a - 1])
    for a in above:
        assert np.array_equal(flat[:, :, a], flat[:, :, a - cw])
    assert any((flat[:, 0, a] >= 0).any() for a in left) and any((flat[:, 0, a] >= 0).any() for a in above)
    assert (np.abs(flat[0, 2:]) > 7).any() and (np.abs(flat[1:, 2:]) > 14).any() and (flat[0, 2:] % 2 == 0).all() and (flat[1:, 2:] % 4 == 0).all()
    assert (flat[:, 1][flat[:, 0] == 4] > 0).any()
    with Ctx(p.seq) as c:
        c.check_grids(c.decode(p), edge, sao, "sao")
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 6. gates and refusals
def _canaries(c, n=1, dense=None):
    torch = _torch()
    seq = c.seq
    ctu = 1 << seq.log2_ctu_size
    shapes = {"edge": ((n, 13, seq.height // 4, seq.width // 4), torch.int16),
              "sao": ((n, 3, 6, (seq.height + ctu - 1) // ctu, (seq.width + ctu - 1) // ctu), torch.int8)}
    if dense is not None:
        shapes = {"loopfilter": ((n, 3) + tuple(dense), torch.uint8)}
    return {k: torch.full(s, CANARY, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}


def _untouched(out):
    _torch().cuda.synchronize()
    return all(bool((t == CANARY).all()) for t in out.values())


def test_gates(oracle):
    p = small_picture(0x6A1, w=264, h=136)
    assert (p.sao_raw[:, 0, 0] != abi.SAO_OFF).any()
    edge, sao = lref.picture_model(oracle, p)
    off = lref.sao_grid(p.seq, None, enabled=False)
    with Ctx(p.seq) as c:
        # no filter call yet: the edge grid is there, the SAO grid and the dense form are refused and nothing is written
        h = c.decode(p, stages=None)
        assert c.ctx.loopfilter_status([h], need_filter=False) == abi.HMGPU_OK and c.ctx.loopfilter_status([h]) == abi.HMGPU_EINVAL
        _same_edge(c.ctx.export_loopfilter([h], grids=("edge",))["edge"][0], edge)
        out = _canaries(c)
        assert _status(lambda: c.ctx.export_loopfilter([h], out=out)) == abi.HMGPU_EINVAL and _untouched(out)
        sao_only = {"sao": out["sao"]}
        assert _status(lambda: c.ctx.export_loopfilter([h], grids=("sao",), out=sao_only)) == abi.HMGPU_EINVAL and _untouched(out)
        dn = _canaries(c, dense=(136, 264))
        assert _status(lambda: c.ctx.export_loopfilter([h], "dense", out=dn)) == abi.HMGPU_EINVAL and _untouched(dn)
        # deblocking only: the SAO grid is all off, whatever the parameter buffer holds
        c.ctx.filter_picture(h, p.pp, p.sao_raw, stages=3)
        c.check_grids(h, edge, off, "stages 3")
        d = c.ctx.export_loopfilter([h], "dense")["loopfilter"][0].cpu().numpy()
        assert (d[2] == 0).all() and np.array_equal(d, lref.dense(p.seq, edge, off, (0, 0, 264, 136)))
        # the SAO stage on its own: now the types are there
        c.ctx.filter_picture(h, p.pp, p.sao_raw, stages=4)
        c.check_grids(h, edge, sao, "stages 4")
        # the handle reused by a picture without SAO: off, not the earlier picture's types
        q = small_picture(0x6A2, w=264, h=136, sao=False)
        assert q.pp.sao_enabled == 0
        qe, qs = lref.picture_model(oracle, q, sao_enabled=False)
        assert not np.array_equal(qe, edge)
        c.decode(q, h)
        c.check_grids(h, qe, qs, "reused")
        assert (qs[:, 0] == -1).all()
        # ... and after release / acquire, before its filter call, the SAO grid is refused again
        c.ctx.release(h)
        h3 = c.ctx.acquire()
        c.ctx.decompress_pictures([(h3, p.slices, p.meta, p.coeffs)])
        assert c.ctx.loopfilter_status([h3]) == abi.HMGPU_EINVAL
        # a partly covered picture: refused by the coverage rule, edge grid included
        h4 = c.ctx.acquire()
        c.ctx.decompress_slice(h4, 0, p.slice, p.meta, p.coeffs, 0, p.num_ctus // 2)
        out = _canaries(c)
        edge_only = {"edge": out["edge"]}
        assert c.ctx.loopfilter_status([h4], need_filter=False) == abi.HMGPU_EINVAL
        assert _status(lambda: c.ctx.export_loopfilter([h4], grids=("edge",), out=edge_only)) == abi.HMGPU_EINVAL and _untouched(out)
        # an uploaded picture has no decisions at all
        assert c.ctx.loopfilter_status([0], need_filter=False) == abi.HMGPU_EINVAL
        c.ctx.sync()


def test_refusals_leave_the_destinations_untouched(oracle):
    torch = _torch()
    p = small_picture(0x6B1, w=264, h=136)
    with Ctx(p.seq) as c:
        h = c.decode(p)
        L = libhm_amd.lib()
        st = torch.cuda.current_stream().cuda_stream
        out = _canaries(c, 2)
        e, s = out["edge"], out["sao"]
        h4, w4, ch, cw = 34, 66, 3, 5
        ptrs = [e.data_ptr(), s.data_ptr(), None]
        pitch, pstr, bstr = [w4 * 2, cw, 0], [h4 * w4 * 2, ch * cw, 0], [13 * h4 * w4 * 2, 18 * ch * cw, 0]
        ok = abi.make_loopfilter_desc()
        into = lambda desc=ok, pics=(h, h), ptrs=ptrs, pitch=pitch, pstr=pstr, bstr=bstr, **kw: _status(
            lambda: c.ctx.export_loopfilter_into(list(pics), desc, ptrs, pitch, pstr, bstr, 1, st, **kw))
        assert c.ctx.loopfilter_destination_status(2, ok, ptrs, pitch, pstr, bstr) == abi.HMGPU_OK
        # bad form; misaligned crop; n > 16; a scale (and a filter that is not nearest) with the grids; an invalid handle
        assert into(abi.make_loopfilter_desc(2)) == abi.HMGPU_EINVAL
        assert into(abi.make_loopfilter_desc(crop=(4, 0, 0, 0))) == abi.HMGPU_EINVAL
        assert into(pics=[h] * 17) == abi.HMGPU_EINVAL
        assert into(scale=abi.make_export_scale(64, 64, abi.SCALE_NEAREST)) == abi.HMGPU_EINVAL
        assert into(pics=(h, 63)) == abi.HMGPU_EINVAL
        # destination span: an allocation with room for two pictures less one element; then one picture fits it
        hip = _hip()
        raw, picb = C.c_void_p(), 13 * h4 * w4 * 2
        assert hip.hipMalloc(C.byref(raw), 2 * picb - 2) == 0
        try:
            assert hip.hipMemset(raw, CANARY, 2 * picb - 2) == 0
            short = [raw.value, None, None]
            assert c.ctx.loopfilter_destination_status(2, ok, short, pitch, pstr, bstr) == abi.HMGPU_EINVAL
            assert into(ptrs=short) == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            back = np.zeros(2 * picb - 2, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 2, 2) == 0 and (back == CANARY).all()
            assert into(pics=(h,), ptrs=short) == abi.HMGPU_OK
            torch.cuda.synchronize()
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 2, 2) == 0
            assert np.array_equal(back[:picb].view(np.int16).reshape(13, h4, w4), lref.picture_model(oracle, p)[0]) and (back[picb:] == CANARY).all()
        finally:
            hip.hipFree(raw)
        # strides below the extents they step over, a misaligned pointer, no destination at all, a slot of the other form
        assert into(pitch=[w4 * 2 - 2, cw, 0]) == abi.HMGPU_EINVAL and into(pstr=[h4 * w4 * 2 - 2, ch * cw, 0]) == abi.HMGPU_EINVAL
        assert into(bstr=[13 * h4 * w4 * 2, 18 * ch * cw - 1, 0]) == abi.HMGPU_EINVAL
        assert into(ptrs=[e.data_ptr() + 1, None, None]) == abi.HMGPU_EINVAL                  # int16 at an odd address
        assert into(ptrs=[None, None, None]) == abi.HMGPU_EINVAL
        assert into(ptrs=[e.data_ptr(), None, e.data_ptr()]) == abi.HMGPU_EINVAL              # the dense slot does not exist in this form
        # the dense form: a filter that is not nearest is unsupported; a grid destination with it is refused
        whole = [abi.make_export_window((0, 0, 0, 0))] * 2
        dense = abi.make_loopfilter_desc(abi.LOOPFILTER_DENSE)
        dn = _canaries(c, 2, dense=(64, 64))["loopfilter"]
        dargs = dict(ptrs=[None, None, dn.data_ptr()], pitch=[0, 0, 64], pstr=[0, 0, 64 * 64], bstr=[0, 0, 3 * 64 * 64], windows=whole)
        assert into(dense, scale=abi.make_export_scale(64, 64, abi.SCALE_BILINEAR), **dargs) == abi.HMGPU_EUNSUPPORTED
        assert into(dense, **dict(dargs, ptrs=[e.data_ptr(), None, dn.data_ptr()]), scale=abi.make_export_scale(64, 64, abi.SCALE_NEAREST)) == abi.HMGPU_EINVAL
        assert into(dense, **dict(dargs, windows=None), scale=abi.make_export_scale(64, 64, abi.SCALE_NEAREST)) == abi.HMGPU_EINVAL
        # a null description, straight at the C entry
        from libhm_amd import loopfilter as lf
        args = lf.c_args(ptrs, pitch, pstr, bstr)
        assert L.hmgpu_pictures_export_loopfilter(c.ctx._h, 2, abi.handle_array([h, h]), None, None, None, *args, 1, abi.addr(st)) == abi.HMGPU_EINVAL
        assert L.hmgpu_loopfilter_destination_check(c.ctx._h, 2, None, None, None, *args) == abi.HMGPU_EINVAL
        assert _untouched(out) and bool((dn == CANARY).all())
        # and the same arguments, valid, write both pictures
        assert into() == abi.HMGPU_OK and into(dense, scale=abi.make_export_scale(64, 64, abi.SCALE_NEAREST), **dargs) == abi.HMGPU_OK
        torch.cuda.synchronize()
        edge, sao = lref.picture_model(oracle, p)
        for i in range(2):
            _same_edge(e[i], edge)
            assert np.array_equal(s[i].cpu().numpy(), sao)
            assert np.array_equal(dn[i].cpu().numpy(), lref.dense(p.seq, edge, sao, (0, 0, 264, 136), (64, 64)))
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 7. the dense form
def test_dense_windows_flip_scale_and_types(oracle):
    torch = _torch()
    pics = [motion_picture(1, True), small_picture(0x7D1, w=W, h=H), small_picture(0x7D2, w=W, h=H, num_slices=3, lf_across_slices=0)]
    models = [lref.picture_model(oracle, p) for p in pics]
    assert all((m[1][0, 0] >= 0).any() and (m[1][0, 0] < 0).any() for m in models)
    pics[0].seq.max_pictures = 8
    with Ctx(pics[0].seq) as c:
        hs = [c.decode(p) for p in pics]
        # per-picture windows of different sizes at 0.5x of the first, the second mirrored and touching the right and bottom edges
        windows, flips, size = [(10, 6, 256, 160), (260, 164, 260, 164), (0, 0, W, H)], [False, True, False], (80, 128)
        want = [lref.dense(p.seq, m[0], m[1], w, size, f) for p, m, w, f in zip(pics, models, windows, flips)]
        assert all(all((w[k] != 0).any() and (w[k] == 0).any() for k in range(3)) for w in want)
        got = c.ctx.export_loopfilter(hs, "dense", size=size, windows=windows, flip=flips)["loopfilter"]
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 3, 80, 128)
        for i in range(3):
            assert np.array_equal(got[i].cpu().numpy(), want[i]), (i, [int((got[i, k].cpu().numpy() != want[i][k]).sum()) for k in range(3)])
        scale = (0.5, -2.0, 1.0 / 3.0)
        for dtype in (torch.float32, torch.float16, torch.bfloat16):
            f = c.ctx.export_loopfilter(hs, "dense", size=size, windows=windows, flip=flips, dtype=dtype, scale=scale)["loopfilter"]
            assert f.dtype == dtype
            for i in range(3):
                for k in range(3):
                    ref = torch.from_numpy((want[i][k].astype(np.float32) * np.float32(scale[k])).astype(np.float32)).to(dtype)
                    assert torch.equal(f[i, k].cpu(), ref), (dtype, i, k)
        # unscaled: windows of one size, odd widths, one touching the right and bottom picture edges (e >= width: no edge to report)
        windows = [(264, 168, 256, 160), (2, 2, 256, 160), (130, 84, 256, 160)]
        want = [lref.dense(p.seq, m[0], m[1], w, None, f) for p, m, w, f in zip(pics, models, windows, flips)]
        assert (want[0][0][:, -4:] == 0).all() and (want[0][1][-4:] == 0).all()
        got = c.ctx.export_loopfilter(hs, "dense", windows=windows, flip=flips)["loopfilter"]
        for i in range(3):
            assert np.array_equal(got[i].cpu().numpy(), want[i]), i
        # a window whose width is no multiple of the lane's eight samples
        one = c.ctx.export_loopfilter(hs[:1], "dense", windows=[(250, 100, 270, 50)], flip=[True])["loopfilter"]
        assert np.array_equal(one[0].cpu().numpy(), lref.dense(pics[0].seq, models[0][0], models[0][1], (250, 100, 270, 50), None, True))
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 8. strides
@pytest.mark.parametrize("shift", [2, 1])
def test_strided_destinations(oracle, shift):
    """out= views with a pitch, a channel stride and a batch stride of their own; shift 2: dword-aligned rows, 1: int16 stores"""
    torch = _torch()
    pics = [small_picture(0x8E1, w=264, h=136), small_picture(0x8E2, w=264, h=136, sao=True, num_slices=2)]
    models = [lref.picture_model(oracle, p) for p in pics]
    with Ctx(pics[0].seq) as c:
        hs = [c.decode(p) for p in pics]
        big_e = torch.full((3, 15, 34 + 3, 66 + 6), CANARY, dtype=torch.int16, device="cuda")
        big_s = torch.full((3, 20, 3 + 2, 5 + 3), CANARY, dtype=torch.int8, device="cuda")
        big_d = torch.full((3, 4, 50 + 2, 100 + 9), CANARY, dtype=torch.uint8, device="cuda")
        ve = big_e[1:3, 1:14, 2:36, shift:shift + 66]
        vs = big_s[0:2, 1:19].unflatten(1, (3, 6))[:, :, :, 1:4, 2:7]
        vd = big_d[0:2, 1:4, 1:51, shift:shift + 100]
        keep = [t.clone() for t in (big_e, big_s, big_d)]
        c.ctx.export_loopfilter(hs, out={"edge": ve, "sao": vs})
        windows = [(8, 4, 200, 100), (64, 36, 200, 100)]
        c.ctx.export_loopfilter(hs, "dense", size=(50, 100), windows=windows, out={"loopfilter": vd})
        torch.cuda.synchronize()
        for i in range(2):
            _same_edge(ve[i], models[i][0], ("edge view", i))
            assert np.array_equal(vs[i].cpu().numpy(), models[i][1]), ("sao view", i)
            assert np.array_equal(vd[i].cpu().numpy(), lref.dense(pics[i].seq, models[i][0], models[i][1], windows[i], (50, 100))), ("dense view", i)
        # the bytes around the views are unchanged
        for big, view, was in ((big_e, ve, keep[0]), (big_s, vs, keep[1]), (big_d, vd, keep[2])):
            view.fill_(CANARY)
            assert torch.equal(big, was)
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 9. end to end through libhmdec
FROM_PARSER = {"depth": "depth", "part_size": "part_size", "pred_mode": "pred_mode", "qp": "qp", "tr_idx": "tr_idx", "cbf_y": "cbf0",
               "cbf_u": "cbf1", "cbf_v": "cbf2", "mv0": "mv0", "mv1": "mv1", "ref_idx0": "ref_idx0", "ref_idx1": "ref_idx1",
               "bypass": "bypass", "ipcm": "ipcm", "slice_idx": "slice_idx", "tile_idx": "tile_idx"}
_models = {}


def stream_models(oracle, name):
    """POC -> (edge grid, SAO grid, seq) from the arrays a parse-only decoder leaves (hmdec_picture_array, hmdec_picture_slice_params,
    the "sao" array); no device involved; computed once per stream"""
    if name in _models:
        return _models[name]
    z = gu.load("stream_" + name)
    out = {}
    with hmdec.Decoder(parse_only=True) as d:
        def on_decoded(p):
            g = p.geometry()
            n = g["num_ctbs"]
            seq = abi.make_seq(g["width"], g["height"], g["bd_y"], g["bd_c"], log2_ctu=g["log2_ctb"], range_ext_flags=g["range_ext"])
            seq.pcm_bit_depth_luma, seq.pcm_bit_depth_chroma, seq.pcm_loop_filter_disable = g["pcm_bd_y"], g["pcm_bd_c"], g["pcm_lf_disable"]
            seq.chroma_format = g["chroma_format"]
            arrays = {k: p.array(v) for k, v in FROM_PARSER.items()}
            parts = len(arrays["depth"]) // n
            m = {k: (v.reshape(n, parts, 2) if k.startswith("mv") else v.reshape(n, -1) if v.size != n else v) for k, v in arrays.items()}
            slices, handle_of = [], {}
            for i in range(p.num_slices()):
                sp, _ = p.slice_params(i)
                sp.scaling_lists = None
                for l in range(2):                                  # the oracle compares reference pictures by handle: one per POC
                    for k in range(sp.num_ref_idx[l]):
                        sp.ref_pic[l][k] = handle_of.setdefault(int(sp.ref_poc[l][k]), len(handle_of))
                slices.append(sp)
            pp = abi.make_pic_params(sao_enabled=g["sao"], lf_across_tiles=g["lf_across_tiles"], sao_offset_shift=g["sao_shift"])
            meta = abi.MetaHolder(m)
            bv, bh = oracle.boundary_strengths(seq, slices, meta, pp)
            edge = lref.edge_grid(seq, slices, m["slice_idx"], m["qp"], lref.exempt_of(seq, m), bv, bh)
            sao = lref.sao_grid(seq, oracle.sao_reconstruct_params(seq, pp, meta, p.array("sao").reshape(n, 3, 35)) if g["sao"] else None, bool(g["sao"]))
            out[p.poc] = (edge, sao, seq, p.conformance_window())
        d.decode_stream(z["bitstream"], on_decoded=on_decoded)
    _models[name] = out
    return out


@pytest.mark.parametrize("name,kw", [("ra_main10_208x120", dict(threads=1)), ("ra_main10_208x120", dict(threads=3, devices=[0, 0])),
                                     ("intra_444_ccp_main10_208x120", dict(threads=1))], ids=["420", "420_two_contexts", "444"])
def test_streams_through_the_decoder(oracle, name, kw):
    z = gu.load("stream_" + name)
    want = stream_models(oracle, name)
    seen, held = [], []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            edge, sao, seq, crop = want[pic.poc]
            one = pic.loopfilter()
            assert sorted(one) == ["edge", "sao"]
            _same_edge(one["edge"], edge, (name, pic.poc))
            assert np.array_equal(one["sao"].cpu().numpy(), sao), (name, pic.poc)
            l, r, t, b = crop
            win = (l, t, seq.width - l - r, seq.height - t - b)
            dn = pic.loopfilter("dense")["loopfilter"].cpu().numpy()
            assert np.array_equal(dn, lref.dense(seq, edge, sao, win)), (name, pic.poc)
            # several pictures in one call equal the per-picture calls
            both = hmdec.export_loopfilter_batch([pic, pic])
            for slot in range(2):
                assert np.array_equal(both["edge"][slot].cpu().numpy(), one["edge"].cpu().numpy())
                assert np.array_equal(both["sao"][slot].cpu().numpy(), one["sao"].cpu().numpy())
            seen.append((pic.poc, bool((edge[lref.BS:lref.BS + 2] > 0).any()), bool((sao[:, 0] >= 0).any())))
        d.decode_stream(z["bitstream"], on_output=on_output)
        assert d.hash_mismatches == 0
    assert len(seen) == len(want) >= 1 and any(e for _, e, _ in seen)
    assert len(set(want[p][0].tobytes() for p in want)) > 1 or len(want) == 1
