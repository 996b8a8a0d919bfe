"""Residual export on the GPU (hmgpu_pictures_export_residual, k_residual.hip) behind Context.export_residual: every element bit for
bit against the model (tests/residual_ref.py: the C oracle's TU function per coded block of synth.coded_blocks()).  Pictures are
416x240 -- partial CTUs on both borders -- unless stated otherwise."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, export, frame_parallel as fp
from tests import motion_ref as mref
from tests import residual_ref as rref
from tests import synth

pytestmark = pytest.mark.gpu

W, H = 416, 240
NO_AMP = (0.1, 0.3, 0.3, 0.3, 0.0)
NAMES = ("y", "cb", "cr")
CANARY = 0x5A5A


def _torch():
    import torch
    return torch


def bits(t):
    """a tensor's elements on the host: int16 as it is, floats as bit patterns of their own width"""
    torch = _torch()
    if t.dtype == torch.int16:
        return t.cpu().numpy()
    view = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


def make_seq(w=W, h=H, log2_ctu=6, fmt=1, bd=10, bdc=None, max_pictures=10):
    seq = abi.make_seq(w, h, bd, bd if bdc is None else bdc, log2_ctu=log2_ctu, max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def picture(seq, seed, bi=False, intra_frac=0.0, **kw):
    kw.setdefault("mode_probs", NO_AMP if intra_frac >= 1.0 else (0.1, 0.3, 0.3, 0.2, 0.1))
    kw.setdefault("sao", False)
    return synth.make_picture(seq.width, seq.height, seq.bit_depth_luma, seed=seed, bi=bi, intra_frac=intra_frac, num_refs=2,
                              ref_handles=([0, 1], [1]), chroma_format=seq.chroma_format, log2_ctu=seq.log2_ctu_size,
                              bit_depth_chroma=seq.bit_depth_chroma, **kw)


def as_i_picture(p):
    """an all-intra synthetic picture as an I slice without reference lists"""
    sl = abi.clone_slice(p.slice)
    sl.slice_type = abi.I_SLICE
    sl.num_ref_idx[0] = sl.num_ref_idx[1] = 0
    p.slice, p.slices = sl, [sl]
    return p


def model(p, intra=True, seq=None):
    return rref.planes(p.seq if seq is None else seq, p.slices, p.meta_np, p.coeffs.arrays, intra)


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

    def decode(self, p, h=None):
        h = self.ctx.acquire() if h is None else h
        self.ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs)])
        return h

    def check_planes(self, h, want, components=(0, 1, 2), crop=(0, 0, 0, 0), where=""):
        got = self.ctx.export_residual([h], "planes", components, crop=crop)
        comps = [c for c in components if c < self.ncomp]
        assert sorted(got) == sorted(NAMES[c] for c in comps), where
        cut = rref.crop(want, crop)
        for c in comps:
            g = bits(got[NAMES[c]][0])
            assert g.shape == cut[c].shape, (where, c)
            assert np.array_equal(g, cut[c]), (where, c, crop, int((g != cut[c]).sum()))
        return got


# ------------------------------------------------------------------------------------------------ 1. PLANES against the model
@pytest.mark.parametrize("log2_ctu", [6, 5, 4])
def test_planes_match_the_model_on_p_b_and_i_pictures(log2_ctu):
    """P / B / I pictures at 10 / 60 % intra CUs with intra NxN, transform trees three deep, 2NxN / Nx2N / NxN and AMP PUs; the
    uncoded part of every plane is zero although the tiles hold the residual of the pictures decoded into the handle before"""
    seq = make_seq(log2_ctu=log2_ctu)
    kinds = [(False, 0.1, (0.4, 0.2, 0.2, 0.2)), (True, 0.6, (0.4, 0.2, 0.2, 0.2)), (True, 0.1, None), (False, 1.0, None)]
    with Ctx(seq) as c:
        h = c.ctx.acquire()
        for i, (bi, fr, parts) in enumerate(kinds):
            kw = dict(part_probs=parts, intra_nxn_prob=0.5, tr_depth_max=3, cbf_prob=0.6) if parts else dict(tr_depth_max=3, cbf_prob=0.4)
            p = picture(seq, 200 + 10 * log2_ctu + i, bi, fr, **kw)
            if fr >= 1.0:
                as_i_picture(p)
            c.decode(p, h)
            want = model(p)
            assert all(a.any() for a in want) and all((a == 0).mean() > 0.1 for a in want)
            c.check_planes(h, want, where=(log2_ctu, bi, fr))
        c.ctx.sync()


@pytest.mark.parametrize("bd,bdc,fmt", [(8, 8, 1), (10, 10, 1), (12, 12, 1), (10, 8, 1), (8, 10, 1), (10, 10, 0)])
def test_planes_at_every_depth_pair_and_in_400(bd, bdc, fmt):
    torch = _torch()
    seq = make_seq(bd=bd, bdc=bdc, fmt=fmt)
    with Ctx(seq) as c:
        p = picture(seq, 300 + bd + bdc + fmt, True, 0.3, tr_depth_max=2)
        h = c.decode(p)
        want = model(p)
        got = c.check_planes(h, want, where=(bd, bdc, fmt))
        if fmt == 0:
            # chroma destinations handed to the C entry point stay untouched; the Python layer has no chroma tensor to give
            assert sorted(got) == ["y"]
            y = torch.full((1, H, W), CANARY, dtype=torch.int16, device="cuda")
            cb = torch.full((2, 1, H // 2, W // 2), CANARY, dtype=torch.int16, device="cuda")
            desc = abi.make_residual_desc(abi.RESIDUAL_PLANES, 7)
            c.ctx.export_residual_into([h], desc, [y.data_ptr(), cb[0].data_ptr(), cb[1].data_ptr()], [W * 2, W, W], [0, 0, 0],
                                       [H * W * 2, H * W // 2, H * W // 2], 1, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(bits(y[0]), want[0]) and bool((cb == CANARY).all())
        c.ctx.sync()


def _rext_meta(p, flags):
    """transform skip, lossless CUs, explicit RDPCM modes and intra modes 10 / 26 all over the picture (as tests/test_gpu_fullsize.py)"""
    m = dict(p.meta_np)
    n = p.num_ctus
    rng = np.random.RandomState(flags)
    z = np.arange(256)[None, :]
    cu_first = z & ~((256 >> (2 * m["depth"])) - 1)
    per_cu = lambda r: np.take_along_axis(r, cu_first, axis=1)
    log2tu = 6 - m["depth"] - m["tr_idx"]
    m["bypass"] = (per_cu(rng.rand(n, 256)) < 0.3).astype(np.uint8)
    quad = rng.rand(n, 64) < 0.5
    tu_first = z & ~(np.maximum(256 >> (2 * (m["depth"] + m["tr_idx"])), 1) - 1)
    per_tu = lambda r: np.take_along_axis(r, tu_first, axis=1)
    skip = [per_tu(rng.rand(n, 256)) < 0.6, np.where(log2tu <= 3, np.repeat(quad, 4, axis=1), per_tu(rng.rand(n, 256)) < 0.5),
            np.where(log2tu <= 3, np.repeat(~quad, 4, axis=1), per_tu(rng.rand(n, 256)) < 0.5)]
    for c, k in enumerate(("ts_y", "ts_u", "ts_v")):
        ts = (skip[c] & (m["bypass"] == 0)).astype(np.uint8)
        rd = per_tu(rng.randint(0, 3, size=ts.shape)).astype(np.uint8)
        inter_untransformed = (m["pred_mode"] == 0) & ((ts != 0) | (m["bypass"] != 0))
        m[k] = ts | (np.where(inter_untransformed, rd, 0) << 1).astype(np.uint8)
    pick = per_cu(rng.rand(n, 256))
    m["intra_dir_l"] = np.where(pick < 0.3, 10, np.where(pick < 0.6, 26, m["intra_dir_l"])).astype(np.uint8)
    pick = per_cu(rng.rand(n, 256))
    m["intra_dir_c"] = np.where(pick < 0.25, 10, np.where(pick < 0.5, 26, m["intra_dir_c"])).astype(np.uint8)
    p.meta_np = m
    p.meta = abi.MetaHolder(m)
    return p


@pytest.mark.parametrize("flags", [15, 1, 2, 4, 8])
def test_planes_with_the_range_extension_tools(flags):
    """rotation, implicit and explicit RDPCM on transform-skip and lossless blocks of every size: all tools, then each alone"""
    seq = make_seq(bd=8)
    seq.range_ext_flags = flags
    with Ctx(seq) as c:
        p = picture(seq, 0x52 + flags, False, 0.4, mode_probs=(0.15, 0.25, 0.3, 0.3, 0), cbf_prob=0.9, tr_split_prob=0.4)
        p.seq.range_ext_flags = flags
        _rext_meta(p, flags)
        h = c.decode(p)
        want = model(p)
        c.check_planes(h, want, where=flags)
        if flags & 7:
            p.seq.range_ext_flags = 0
            assert any(not np.array_equal(a, b) for a, b in zip(model(p), want))         # the tools do something on this picture
        c.ctx.sync()


def test_planes_with_custom_scaling_lists_and_full_range_levels():
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 0x5CA1, False, 0.4, cbf_prob=0.85, tr_split_prob=0.5, num_slices=3)
        rng = np.random.RandomState(0x11575)
        lists = abi.ScalingLists()
        for sz in range(4):
            for l in range(6):
                lists.dc[sz][l] = int(rng.randint(1, 256)) if sz >= 2 else 16
                for i in range(64):
                    lists.coef[sz][l][i] = int(rng.randint(1, 256)) if i < (16 if sz == 0 else 64) else 16
        for sl in p.slices:
            sl.scaling_lists = C.pointer(lists)
        h = c.decode(p)
        want = model(p)
        c.check_planes(h, want, where="lists")
        for sl in p.slices:
            sl.scaling_lists = None
        assert any(not np.array_equal(a, b) for a, b in zip(model(p), want))
        # every level of a coded TU uniform over the full int16 range: residuals at both ends of int16
        q = picture(seq, 0x57E5, True, 0.2, coef_dist="stress", tr_depth_max=2)
        c.decode(q, h)
        want = model(q)
        assert want[0].min() < -20000 and want[0].max() > 20000
        c.check_planes(h, want, where="stress")
        c.ctx.sync()


def _with_pcm_and_lossless(p, seed):
    """some intra 2Nx2N CUs of at most 32x32 become PCM CUs -- their cbf bits stay set, which HM's parser never leaves: the flag alone
    must keep them out -- and some other CUs lossless"""
    m = dict(p.meta_np)
    n, parts = m["depth"].shape
    rng = np.random.RandomState(seed)
    z = np.arange(parts)[None, :]
    cu_first = z & ~((parts >> (2 * m["depth"].astype(np.int64))) - 1)
    per_cu = lambda r: np.take_along_axis(r, cu_first, axis=1)
    decoded = m["part_size"] != abi.SIZE_NONE
    pcm = (per_cu(rng.rand(n, parts)) < 0.4) & decoded & (m["pred_mode"] == abi.MODE_INTRA) & (m["part_size"] == abi.SIZE_2Nx2N) & (m["depth"] >= 1)
    m["ipcm"] = pcm.astype(np.uint8)
    m["tr_idx"] = np.where(pcm, 0, m["tr_idx"])
    for k in ("cbf_y", "cbf_u", "cbf_v"):
        m[k] = np.where(pcm, 1, m[k])
    m["bypass"] = ((per_cu(rng.rand(n, parts)) < 0.3) & decoded & ~pcm).astype(np.uint8)
    p.meta_np = m
    p.meta = abi.MetaHolder(m)
    bd = [p.seq.bit_depth_luma, p.seq.bit_depth_chroma, p.seq.bit_depth_chroma]
    p.coeffs = abi.CoeffHolder(*p.coeffs.arrays, pcm=[rng.randint(0, 1 << bd[k], size=p.coeffs.arrays[k].shape).astype(np.int16) for k in range(3)])
    return p


def _pcm_seq(**kw):
    seq = make_seq(**kw)
    seq.pcm_bit_depth_luma, seq.pcm_bit_depth_chroma = seq.bit_depth_luma, seq.bit_depth_chroma
    return seq


def test_planes_with_pcm_and_lossless_cus():
    seq = _pcm_seq()
    with Ctx(seq) as c:
        p = _with_pcm_and_lossless(picture(seq, 0x9C3, False, 0.5, cbf_prob=0.8), 3)
        assert p.meta_np["ipcm"].any() and p.meta_np["bypass"].any()
        h = c.decode(p)
        want = model(p)
        c.check_planes(h, want, where="pcm")
        # without the flag the same arrays would give those CUs a residual: the gate is what keeps them zero
        m = dict(p.meta_np)
        m["ipcm"] = np.zeros_like(m["ipcm"])
        loud = rref.planes(seq, p.slices, m, p.coeffs.arrays)
        assert any(not np.array_equal(a, b) for a, b in zip(loud, want))
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 2. crops, masks, views
def test_crops_component_masks_and_unaligned_views():
    """crops in multiples of 8 luma samples (chroma lanes cut in half), every component mask, and destinations that are views of
    larger canary-filled tensors at odd offsets: the element-wise stores; nothing outside the views changes"""
    torch = _torch()
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 401, True, 0.3, tr_depth_max=2)
        h = c.decode(p)
        want = model(p)
        for crop in ((8, 0, 0, 0), (0, 8, 8, 0), (24, 40, 16, 8), (64, 64, 32, 32), (200, 208, 120, 112), (16, 16, 0, 0)):
            c.check_planes(h, want, crop=crop, where="crop")
        for comps in ((0,), (1,), (2,), (0, 2), (1, 2)):
            c.check_planes(h, want, comps, crop=(8, 24, 0, 16), where="mask")
        for off, pad in (((1, 3), (5, 9)), ((0, 0), (2, 8))):
            crop = (8, 16, 8, 0)
            cut = rref.crop(want, crop)
            big = {NAMES[k]: torch.full((3, cut[k].shape[0] + pad[0], cut[k].shape[1] + pad[1]), CANARY, dtype=torch.int16, device="cuda") for k in range(3)}
            view = {k: big[k][0:2, off[0]:off[0] + cut[i].shape[0], off[1]:off[1] + cut[i].shape[1]] for i, k in enumerate(NAMES)}
            got = c.ctx.export_residual([h, h], "planes", crop=crop, out=view)
            torch.cuda.synchronize()
            for i, k in enumerate(NAMES):
                assert got[k] is view[k]
                for slot in range(2):
                    assert np.array_equal(bits(view[k][slot]), cut[i]), (k, slot, off)
                rest = big[k].clone()
                rest[0:2, off[0]:off[0] + cut[i].shape[0], off[1]:off[1] + cut[i].shape[1]].fill_(CANARY)
                assert bool((rest == CANARY).all()), (k, off)
        # a subset of the destinations: only what is given is written
        only = c.ctx.export_residual([h], "planes", out={"cr": torch.zeros((1, H // 2, W // 2), dtype=torch.int16, device="cuda")})
        assert list(only) == ["cr"] and np.array_equal(bits(only["cr"][0]), want[2])
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 3. stale tiles, stale groups
def test_stale_tiles_and_groups_of_a_reused_handle_read_as_zero():
    """one handle fed from one staging block: a dense B picture, a P picture twenty times sparser, an I picture, then a picture
    without intra_dir[] (its intra CUs are not reconstructed: no residual).  The tiles keep the earlier pictures' residual wherever
    the current one codes nothing; codedness comes from the arrays.  Then a PCM picture followed by one without the flag group: the
    intra blocks where the PCM CUs were come out again.  (This holds end to end; it does not isolate the export's own gate on the
    flag group, because every staging path clears or rewrites the device copy of that group -- DESIGN.md 9h.)"""
    seq = _pcm_seq()
    with Ctx(seq) as c:
        stg = c.ctx.staging_alloc()
        dense_b = picture(seq, 501, True, 0.1, cbf_prob=0.9, tr_depth_max=2)
        sparse_p = picture(seq, 502, False, 0.1, cbf_prob=0.045, tr_depth_max=2)
        i_pic = as_i_picture(picture(seq, 503, False, 1.0, cbf_prob=0.5))
        no_dir = picture(seq, 504, False, 0.5, cbf_prob=0.7)
        pcm = _with_pcm_and_lossless(picture(seq, 505, False, 0.6, cbf_prob=0.9), 5)
        no_flags = picture(seq, 506, False, 0.6, cbf_prob=0.9)
        h = None
        density = {}
        for name, p in (("B", dense_b), ("P", sparse_p), ("I", i_pic), ("nodir", no_dir), ("pcm", pcm), ("noflags", no_flags)):
            if h is not None:
                c.ctx.release(h)
            h2 = c.ctx.acquire()
            assert h is None or h2 == h
            h = h2
            c.ctx.sync()
            stg.fill(p.meta, p.coeffs)
            stg.set_groups(intra=name != "nodir", flags=name == "pcm")
            for k in range(3):
                stg.coeffs.pcm_sample[k] = abi._ptr(p.coeffs.pcm[k]) if name == "pcm" else None
            c.ctx.decompress_pictures([(h, p.slices, stg, stg)])
            m = dict(p.meta_np)
            if name != "pcm":
                for k in ("ts_y", "ts_u", "ts_v", "bypass", "ipcm"):
                    m[k] = None
            want = rref.planes(seq, p.slices, m, p.coeffs.arrays, intra=name != "nodir")
            c.check_planes(h, want, where=name)
            density[name] = float((want[0] != 0).mean())
        assert density["B"] > 20 * density["P"] > 0, density
        # the picture without intra_dir[] has intra CUs with coded blocks: all of them zero
        assert any(not np.array_equal(a, b) for a, b in zip(model(no_dir), model(no_dir, intra=False)))
        # the picture after the PCM one has coded intra blocks where that one had PCM CUs
        both = (pcm.meta_np["ipcm"] != 0) & (no_flags.meta_np["pred_mode"] == abi.MODE_INTRA) & (no_flags.meta_np["cbf_y"] != 0)
        assert both.any()
        c.ctx.sync()
        c.ctx.staging_free(stg)


def test_packed_input_and_slice_by_slice():
    torch = _torch()
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 601, True, 0.3, num_slices=4, tr_depth_max=2)
        want = model(p)
        ha = c.decode(p)
        a = c.check_planes(ha, want)
        hp = c.ctx.acquire()
        blob = libhm_amd.pack_input(seq, p.meta, p.coeffs)
        c.ctx.decompress_pictures_packed([(hp, p.slices, blob, None)])
        b = c.check_planes(hp, want, where="packed")
        for k in a:
            assert torch.equal(a[k], b[k]), k
        h2 = c.ctx.acquire()
        for k, (first, n) in enumerate(p.slice_ranges):
            c.ctx.decompress_slice(h2, k, p.slices[k], p.meta, p.coeffs, first, n)
            if k < len(p.slice_ranges) - 1:
                assert c.ctx.residual_status([h2]) == abi.HMGPU_EINVAL
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    c.ctx.export_residual([h2])
                assert e.value.status == abi.HMGPU_EINVAL
        assert c.ctx.residual_status([h2]) == abi.HMGPU_OK
        c.check_planes(h2, want, where="slice calls")
        c.ctx.sync()


def test_slice_calls_that_disagree_about_intra_dir_give_no_intra_residual():
    """a picture built slice by slice whose FIRST call comes without intra_dir[] and the others with it, in a handle whose tiles hold a
    dense picture's residual: the intra CUs of the first slice were never listed, so their tiles are stale.  The record is per picture:
    intra CUs carry a residual only when every covering call had the modes, so all of them come out as 0, the inter blocks as they are"""
    seq = make_seq()
    with Ctx(seq) as c:
        h = c.decode(picture(seq, 611, True, 0.0, cbf_prob=0.95))
        c.ctx.release(h)
        assert c.ctx.acquire() == h
        p = picture(seq, 612, False, 0.5, num_slices=3, cbf_prob=0.8)
        bare = abi.MetaHolder({k: v for k, v in p.meta_np.items() if k not in ("intra_dir_l", "intra_dir_c")})
        for k, (first, n) in enumerate(p.slice_ranges):
            c.ctx.decompress_slice(h, k, p.slices[k], bare if k == 0 else p.meta, p.coeffs, first, n)
        want = model(p, intra=False)
        assert any(not np.array_equal(a, b) for a, b in zip(want, model(p))) and want[0].any()
        c.check_planes(h, want, where="mixed intra_dir")
        c.ctx.sync()


@pytest.mark.parametrize("n", [1, 5, 16])
def test_batches_of_mixed_pictures(n):
    torch = _torch()
    seq = make_seq(max_pictures=8)
    with Ctx(seq) as c:
        ps = [picture(seq, 701, False, 0.1, tr_depth_max=2), picture(seq, 702, True, 0.4, tr_depth_max=2), as_i_picture(picture(seq, 703, False, 1.0))]
        hs = [c.decode(p) for p in ps]
        wants = [model(p) for p in ps]
        order = [(3 * i + i // 3) % 3 for i in range(n)]
        got = c.ctx.export_residual([hs[i] for i in order])
        for slot, i in enumerate(order):
            for k in range(3):
                assert np.array_equal(bits(got[NAMES[k]][slot]), wants[i][k]), (slot, k)
        d = c.ctx.export_residual([hs[i] for i in order], "dense", dtype=torch.float16, scale=(0.25, 0.5, 1.0))
        assert tuple(d["residual"].shape) == (n, 3, H, W)
        for slot, i in enumerate(order):
            assert np.array_equal(bits(d["residual"][slot]), rref.dense(wants[i], (0, 0, W, H), False, (H, W), dtype="float16", scale=(0.25, 0.5, 1.0))), slot
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 4. DENSE against the model
def test_dense_matches_the_model_and_the_other_exports_positions():
    """windows from export.random_resized_crop, an enlargement, an 8x reduction, flips; int16 and the three float types with a scale
    per component; a destination that is a slice of a larger tensor; and the positions: the pixel export (filter nearest) and the
    dense motion export of the same windows show the sample / the block at the very luma position the residual was taken from"""
    torch = _torch()
    seq = make_seq(bd=8)
    sc = (0.5, -0.37, 1.0 / 3.0)
    with Ctx(seq) as c:
        p = picture(seq, 801, True, 0.3, tr_depth_max=2, sao=False)
        h = c.decode(p)
        want = model(p)
        g = torch.Generator()
        g.manual_seed(7)
        wins, flips = export.random_resized_crop(6, W, H, generator=g)
        wins = [tuple(w) for w in wins] + [(2, 6, 8, 8), (0, 0, 416, 240), (10, 4, 400, 232)]
        flips = [bool(f) for f in flips] + [False, True, True]
        sizes = {(64, 64): list(range(9)), (30, 52): [7, 8], (37, 51): [0, 1, 6]}            # (30, 52): an 8x reduction of 416 / 240 / 400 / 232
        for size, idx in sizes.items():
            ws, fs = [wins[i] for i in idx], [flips[i] for i in idx]
            for dtype, name in ((None, "int16"), (torch.float32, "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
                got = c.ctx.export_residual([h] * len(ws), "dense", size=size, windows=ws, flip=fs, dtype=dtype, scale=None if dtype is None else sc)
                assert sorted(got) == ["residual"] and tuple(got["residual"].shape) == (len(ws), 3) + size
                for slot, (win, f) in enumerate(zip(ws, fs)):
                    assert np.array_equal(bits(got["residual"][slot]), rref.dense(want, win, f, size, dtype=name, scale=sc)), (size, name, slot, win, f)
        assert any(flips[:6]) and not all(flips[:6])
        # unscaled windows of one size, components (2, 0) -> order Y, Cr; into a slice of a larger tensor
        ws, fs = [(0, 0, 96, 64), (104, 56, 96, 64), (318, 174, 96, 64)], [False, True, False]
        big = torch.full((4, 5, 70, 100), CANARY, dtype=torch.int16, device="cuda")
        view = big[1:4, 2:4, 3:67, 4:100]
        c.ctx.export_residual([h] * 3, "dense", (2, 0), windows=ws, flip=fs, out={"residual": view})
        torch.cuda.synchronize()
        for slot, (win, f) in enumerate(zip(ws, fs)):
            assert np.array_equal(bits(view[slot]), rref.dense(want, win, f, (64, 96), components=(0, 2))), slot
        rest = big.clone()
        rest[1:4, 2:4, 3:67, 4:100].fill_(CANARY)
        assert bool((rest == CANARY).all())
        # positions: pixels, block info and residual of the same call arguments come from one luma position
        ws, fs, size = wins[:4] + [wins[6]], flips[:4] + [flips[6]], (64, 64)
        pix = c.ctx.export_batch([h] * 5, "planar", 8, size=size, filter="nearest", windows=ws, flip=fs)
        mot = c.ctx.export_motion([h] * 5, "dense", size=size, windows=ws, flip=fs)
        res = c.ctx.export_residual([h] * 5, "dense", size=size, windows=ws, flip=fs)
        final = c.ctx.download(h)
        grid = mref.grid(p.meta_np, p.slices, W, H, 6)
        for slot, ((x, y, w, hh), f) in enumerate(zip(ws, fs)):
            sx, sy = x + rref.nearest(w, 64), y + rref.nearest(hh, 64)
            luma, blk, r = final[0][np.ix_(sy, sx)], grid["block"][(slice(None),) + np.ix_(sy >> 2, sx >> 2)], want[0][np.ix_(sy, sx)]
            if f:
                luma, blk, r = luma[:, ::-1], blk[:, :, ::-1], r[:, ::-1]
            assert np.array_equal(pix[0][slot].cpu().numpy().astype(np.int64), luma), slot
            assert np.array_equal(mot["block"][slot].cpu().numpy(), blk), slot
            assert np.array_equal(bits(res["residual"][slot, 0]), r), slot
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 5. refusals
def _hip():
    """the HIP runtime this process already runs on"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            L.hipFree.argtypes = [C.c_void_p]
            L.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            return L
    raise RuntimeError("no HIP runtime loaded")


@pytest.mark.parametrize("fmt", [2, 3])
def test_422_and_444_are_refused_before_anything_is_enqueued(fmt):
    torch = _torch()
    seq = make_seq(208, 120, fmt=fmt)
    with Ctx(seq) as c:
        p = picture(seq, 900 + fmt, True, 0.2)
        h = c.decode(p)
        y = torch.full((1, 120, 208), CANARY, dtype=torch.int16, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        args = ([y.data_ptr(), None, None], [416, 0, 0], [0, 0, 0], [120 * 416, 0, 0])
        for desc, sc, win in ((abi.make_residual_desc(abi.RESIDUAL_PLANES, 1), None, None),
                              (abi.make_residual_desc(abi.RESIDUAL_DENSE, 1), None, [abi.make_export_window((0, 0, 0, 0))])):
            assert c.ctx.residual_destination_status(1, desc, *args, scale=sc, windows=win) == abi.HMGPU_EUNSUPPORTED
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_residual_into([h], desc, *args, 1, stream, sc, win)
            assert e.value.status == abi.HMGPU_EUNSUPPORTED
        torch.cuda.synchronize()
        c.ctx.sync()
        assert bool((y == CANARY).all())


def test_refusals_leave_the_destinations_untouched():
    torch = _torch()
    seq = make_seq(200, 120)
    w, h = 200, 120
    with Ctx(seq) as c:
        p = picture(seq, 951, True, 0.2, num_slices=2)
        good = c.decode(p)
        want = model(p)
        fresh = c.ctx.acquire()
        uploaded = c.ctx.acquire()
        c.ctx.decompress_pictures([(uploaded, p.slices, p.meta, p.coeffs)])
        c.ctx.upload(uploaded, synth.noise_planes(w, h, 10, 9))
        half = c.ctx.acquire()
        a, n = p.slice_ranges[0]
        c.ctx.decompress_slice(half, 0, p.slices[0], p.meta, p.coeffs, a, n)
        # a handle that was fully decoded -- coverage complete, arrays and tiles hold that picture's residual -- and then received other
        # planes (region to region on the context's stream, then hmgpu_picture_commit_received): the old occupant's residual must not
        # come out for the new planes
        received = c.decode(p)
        assert c.ctx.residual_status([received]) == abi.HMGPU_OK
        with torch.cuda.stream(torch.cuda.ExternalStream(c.ctx.stream_handle())):
            src = fp.region_tensor(c.ctx, 0)
            rcv = fp.region_tensor(c.ctx, received, receive=True)
            assert src.numel() == rcv.numel() and src.data_ptr() != rcv.data_ptr()
            rcv.copy_(src)
        c.ctx.commit_received(received)
        assert c.ctx.residual_status([received]) == abi.HMGPU_EINVAL
        dst = {"y": torch.full((2, h, w), CANARY, dtype=torch.int16, device="cuda"),
               "cb": torch.full((2, h // 2, w // 2), CANARY, dtype=torch.int16, device="cuda"),
               "cr": torch.full((2, h // 2, w // 2), CANARY, dtype=torch.int16, device="cuda")}
        dd = {"residual": torch.full((2, 3, 32, 48), CANARY, dtype=torch.int16, device="cuda")}

        def untouched():
            torch.cuda.synchronize()
            c.ctx.sync()
            return all(bool((t == CANARY).all()) for t in list(dst.values()) + list(dd.values()))

        for bad in (fresh, uploaded, half, received, 1, 63, -1):           # (handle 1: an uploaded reference picture; 63 / -1: no picture)
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_residual([good, bad], out=dst)
            assert e.value.status == abi.HMGPU_EINVAL, bad
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_residual([bad, good], "dense", size=(32, 48), out=dd)
            assert e.value.status == abi.HMGPU_EINVAL, bad
            assert untouched(), bad
        # a filter other than nearest
        stream = torch.cuda.current_stream().cuda_stream
        desc_d = abi.make_residual_desc(abi.RESIDUAL_DENSE, 7)
        whole = [abi.make_export_window((0, 0, 0, 0))] * 2
        dargs = ([dd["residual"].data_ptr(), None, None], [96, 0, 0], [32 * 96, 0, 0], [3 * 32 * 96, 0, 0])
        for f in (abi.SCALE_BILINEAR, abi.SCALE_BICUBIC, abi.SCALE_AREA):
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_residual_into([good, good], desc_d, *dargs, 1, stream, abi.make_export_scale(48, 32, f), whole)
            assert e.value.status == abi.HMGPU_EUNSUPPORTED
        # ... which is refused before the pictures are looked at: the same call for a picture without a residual
        with pytest.raises(libhm_amd.HmgpuError) as e:
            c.ctx.export_residual_into([uploaded], desc_d, *dargs, 1, stream, abi.make_export_scale(48, 32, abi.SCALE_BILINEAR), whole[:1])
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        assert untouched()
        assert c.ctx.residual_destination_status(2, desc_d, *dargs, scale=abi.make_export_scale(48, 32, abi.SCALE_NEAREST), windows=whole) == abi.HMGPU_OK
        # a destination that does not lie inside one allocation: room for two pictures less one element; a pointer of no device
        desc = abi.make_residual_desc(abi.RESIDUAL_PLANES, 1)
        picb = h * w * 2
        args = ([w * 2, 0, 0], [0, 0, 0], [picb, 0, 0])
        hip = _hip()
        raw = C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), 2 * picb - 2) == 0
        try:
            assert hip.hipMemset(raw, 0x5A, 2 * picb - 2) == 0
            ptrs = [raw.value, None, None]
            assert c.ctx.residual_destination_status(2, desc, ptrs, *args) == abi.HMGPU_EINVAL
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_residual_into([good, good], desc, ptrs, *args, 1, stream)
            assert e.value.status == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            c.ctx.sync()
            back = np.zeros(2 * picb - 2, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 2, 2) == 0
            assert (back == 0x5A).all()
            c.ctx.export_residual_into([good], desc, ptrs, *args, 1, stream)                      # one picture fits
            torch.cuda.synchronize()
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 2, 2) == 0
            assert np.array_equal(back[:picb].view(np.int16).reshape(h, w), want[0]) and (back[picb:] == 0x5A).all()
        finally:
            hip.hipFree(raw)
        host = np.zeros(2 * picb, np.uint8)
        assert c.ctx.residual_destination_status(2, desc, [host.ctypes.data, None, None], *args) == abi.HMGPU_EINVAL       # not device memory
        if torch.cuda.device_count() > 1:
            other = torch.zeros((2, h, w), dtype=torch.int16, device="cuda:1")
            assert c.ctx.residual_destination_status(2, desc, [other.data_ptr(), None, None], *args) == abi.HMGPU_EINVAL   # another device's
        # strides below the extents they step over, misalignment, no destination, a destination of a component that is not selected
        t = dst["y"]
        ok = [t.data_ptr(), None, None]
        assert c.ctx.residual_destination_status(2, desc, ok, *args) == abi.HMGPU_OK
        assert c.ctx.residual_destination_status(2, desc, ok, [w * 2 - 2, 0, 0], args[1], args[2]) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(2, desc, ok, args[0], args[1], [picb - 2, 0, 0]) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(2, desc, ok, [w * 2 + 1, 0, 0], args[1], [picb + 2 * h, 0, 0]) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(2, desc, [t.data_ptr() + 1, None, None], *args) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(2, desc, [None] * 3, *args) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(1, desc, [None, dst["cb"].data_ptr(), None], [0, w, 0], [0, 0, 0], [0, picb // 4, 0]) == abi.HMGPU_EINVAL
        assert c.ctx.residual_destination_status(2, desc_d, [dd["residual"].data_ptr(), None, None], dargs[1], [32 * 96 - 2, 0, 0], dargs[3],
                                                 windows=[abi.make_export_window((0, 104, 0, 56))] * 2) == abi.HMGPU_EINVAL   # (48 x 64 windows: a plane stride below a plane)
        assert c.ctx.residual_destination_status(2, desc_d, [dd["residual"].data_ptr(), dst["cb"].data_ptr(), None], *dargs[1:],
                                                 scale=abi.make_export_scale(48, 32, 0), windows=whole) == abi.HMGPU_EINVAL   # DENSE has one slot
        assert untouched()
        # the good picture still exports
        c.check_planes(good, want)


# ------------------------------------------------------------------------------------------------ 6. the one large case
def test_one_1080p_b_picture_through_both_forms():
    torch = _torch()
    seq = make_seq(1920, 1080)
    with Ctx(seq) as c:
        p = picture(seq, 1080, True, 0.1)
        h = c.decode(p)
        want = model(p)
        c.check_planes(h, want, where="1080p")
        got = c.ctx.export_residual([h, h], "dense", size=(270, 480), windows=[(0, 0, 1920, 1080), (320, 180, 1280, 720)], flip=[False, True],
                                    dtype=torch.bfloat16, scale=(1 / 512, 1 / 512, 1 / 512))
        for slot, (win, f) in enumerate((((0, 0, 1920, 1080), False), ((320, 180, 1280, 720), True))):
            assert np.array_equal(bits(got["residual"][slot]), rref.dense(want, win, f, (270, 480), dtype="bfloat16", scale=(1 / 512,) * 3)), slot
        c.ctx.sync()
