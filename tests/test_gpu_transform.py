"""Transform export on the GPU (hmgpu_pictures_export_transform, k_transform.hip) behind Context.export_transform: the levels, the
de-quantised coefficients and the info grid, every element bit for bit against the model (tests/transform_ref.py: numpy on the blocks
of synth.coded_blocks()).  Pictures are 416x240 -- partial CTUs on both borders -- unless stated otherwise; the picture makers are
those of tests/test_gpu_residual.py."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi
from tests import synth
from tests import test_gpu_residual as base
from tests import transform_ref as tref

pytestmark = pytest.mark.gpu

W, H = base.W, base.H
NAMES = ("y", "cb", "cr")
CANARY = 0x5A5A
make_seq, picture, as_i_picture, Ctx, bits = base.make_seq, base.picture, base.as_i_picture, base.Ctx, base.bits


def _torch():
    import torch
    return torch


def model(p, value, meta=None, seq=None):
    seq, meta = p.seq if seq is None else seq, p.meta_np if meta is None else meta
    if value == "levels":
        return tref.levels_planes(seq, meta, p.coeffs.arrays)
    return tref.coeff_planes(seq, p.slices, meta, p.coeffs.arrays)


def nonvacuous(planes, ncomp=3):
    """the conditions every model plane in use has to meet: it holds non-zero elements and more than 10 % of it is zero"""
    return all(a.any() and (a == 0).mean() > 0.1 for a in planes[:ncomp])


def check(c, h, p, meta=None, intra_dir=True, where="", values=("levels", "coeffs")):
    """both values and the info grid of picture h against the model of p; returns the model planes per value"""
    meta = p.meta_np if meta is None else meta
    wants = {}
    for value in values:
        want = model(p, value, meta, c.seq)
        assert nonvacuous(want, c.ncomp), (where, value)
        got = c.ctx.export_transform([h], value)
        assert sorted(got) == sorted([NAMES[k] for k in range(c.ncomp)] + ["info"]), where
        for k in range(c.ncomp):
            g = bits(got[NAMES[k]][0])
            assert g.shape == want[k].shape, (where, value, k)
            assert np.array_equal(g, want[k]), (where, value, k, int((g != want[k]).sum()))
        info = tref.info_grid(c.seq, meta, intra_dir)
        g = got["info"][0].cpu().numpy()
        assert g.shape == info.shape and np.array_equal(g, info), (where, value, [int((g[k] != info[k]).sum()) for k in range(6)])
        wants[value] = want
    return wants


# ------------------------------------------------------------------------------------------------ 1. against the model
@pytest.mark.parametrize("log2_ctu", [6, 5, 4])
def test_p_b_and_i_pictures_match_the_model(log2_ctu):
    """P / B / I pictures at 10 / 60 % intra CUs with intra NxN, transform trees three deep, 2NxN / Nx2N / NxN and AMP PUs, all into
    one handle: the uncoded part of every plane is zero although the dense level arrays keep the earlier pictures' levels"""
    seq = make_seq(log2_ctu=log2_ctu)
    kinds = [(False, 0.1, (0.4, 0.2, 0.2, 0.2)), (True, 0.6, (0.4, 0.2, 0.2, 0.2)), (True, 0.1, None), (False, 1.0, None)]
    with Ctx(seq) as c:
        h = c.ctx.acquire()
        for i, (bi, fr, parts) in enumerate(kinds):
            kw = dict(part_probs=parts, intra_nxn_prob=0.5, tr_depth_max=3, cbf_prob=0.6) if parts else dict(tr_depth_max=3, cbf_prob=0.4)
            p = picture(seq, 1200 + 10 * log2_ctu + i, bi, fr, **kw)
            if fr >= 1.0:
                as_i_picture(p)
            c.decode(p, h)
            w = check(c, h, p, where=(log2_ctu, bi, fr))
            assert any(not np.array_equal(a, b) for a, b in zip(w["levels"], w["coeffs"]))
        c.ctx.sync()


@pytest.mark.parametrize("fmt,bd,bdc,ccp", [(0, 10, 10, 0), (1, 8, 8, 0), (1, 10, 10, 0), (1, 12, 12, 0), (1, 10, 8, 0), (1, 8, 10, 0),
                                             (2, 10, 10, 0), (3, 10, 10, 0), (3, 10, 10, 0.5)])
def test_every_format_and_depth_pair(fmt, bd, bdc, ccp):
    seq = make_seq(bd=bd, bdc=bdc, fmt=fmt)
    with Ctx(seq) as c:
        p = picture(seq, 1300 + bd + bdc + 7 * fmt, True, 0.3, tr_depth_max=2, ccp_prob=ccp)
        assert not ccp or np.asarray(p.meta_np["ccp_u"]).any()
        h = c.decode(p)
        check(c, h, p, where=(fmt, bd, bdc, ccp))
        if fmt == 0:
            # chroma destinations handed to the C entry point stay untouched
            torch = _torch()
            y = torch.full((1, H, W), CANARY, dtype=torch.int16, device="cuda")
            cb = torch.full((2, 1, H // 2, W // 2), CANARY, dtype=torch.int16, device="cuda")
            c.ctx.export_transform_into([h], abi.make_transform_desc(abi.TRANSFORM_LEVELS, 7), [y.data_ptr(), cb[0].data_ptr(), cb[1].data_ptr(), None],
                                        [W * 2, W, W, 0], [0] * 4, [H * W * 2, H * W // 2, H * W // 2, 0], 1, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(bits(y[0]), model(p, "levels")[0]) and bool((cb == CANARY).all())
        c.ctx.sync()


def test_custom_scaling_lists_with_full_range_levels_then_flat_scaling():
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 0x5CA2, True, 0.4, tr_split_prob=0.5, num_slices=3, coef_dist="stress", tr_depth_max=2)
        rng = np.random.RandomState(0x11576)
        lists = abi.ScalingLists()
        for sz in range(4):
            for l in range(6):
                lists.dc[sz][l] = int(rng.randint(1, 256)) if sz >= 2 else 16
                for i in range(64):
                    lists.coef[sz][l][i] = int(rng.randint(1, 256)) if i < (16 if sz == 0 else 64) else 16
        for sl in p.slices:
            sl.scaling_lists = C.pointer(lists)
        h = c.decode(p)
        want = check(c, h, p, where="lists")["coeffs"]
        assert want[0].min() < -20000 and want[0].max() > 20000
        for sl in p.slices:
            sl.scaling_lists = None
        assert any(not np.array_equal(a, b) for a, b in zip(model(p, "coeffs"), want))
        q = picture(seq, 0x5CA3, False, 0.3, tr_depth_max=2)
        c.decode(q, h)
        check(c, h, q, where="flat after lists")
        c.ctx.sync()


def test_transform_skip_lossless_and_pcm_cus_then_a_picture_without_the_flags():
    seq = base._pcm_seq(bd=8)
    seq.range_ext_flags = 7
    with Ctx(seq) as c:
        p = picture(seq, 0x53, False, 0.4, mode_probs=(0.15, 0.25, 0.3, 0.3, 0), cbf_prob=0.8, tr_split_prob=0.4)
        p.seq.range_ext_flags = 7
        base._rext_meta(p, 7)
        m = p.meta_np
        assert all((m[k] & 1).any() for k in ("ts_y", "ts_u", "ts_v")) and m["bypass"].any()
        h = c.decode(p)
        w = check(c, h, p, where="rext")
        info = tref.info_grid(seq, m)
        assert ((info[3] & 7) != 0).any() and ((info[3] & 8) != 0).any()
        # the tools act after this stage: the same levels whatever the flags, other coefficients without transform skip / bypass
        plain = dict(m, ts_y=None, ts_u=None, ts_v=None, bypass=None)
        assert all(np.array_equal(a, b) for a, b in zip(model(p, "levels", plain), w["levels"]))
        assert any(not np.array_equal(a, b) for a, b in zip(model(p, "coeffs", plain), w["coeffs"]))
        q = base._with_pcm_and_lossless(picture(seq, 0x9C4, False, 0.5, cbf_prob=0.8), 4)
        assert q.meta_np["ipcm"].any() and q.meta_np["bypass"].any()
        c.decode(q, h)
        w = check(c, h, q, where="pcm")
        assert ((tref.info_grid(seq, q.meta_np)[3] & 16) != 0).any()
        loud = model(q, "levels", dict(q.meta_np, ipcm=None))
        assert any(not np.array_equal(a, b) for a, b in zip(loud, w["levels"]))            # the flag alone keeps the PCM CUs zero
        r = picture(seq, 0x9C5, False, 0.6, cbf_prob=0.8)
        bare = {k: v for k, v in r.meta_np.items() if k not in ("ts_y", "ts_u", "ts_v", "bypass", "ipcm")}
        r.meta = abi.MetaHolder(bare)
        c.decode(r, h)
        check(c, h, r, meta=bare, where="no flag group")
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 2. input paths, stale state
@pytest.mark.parametrize("fmt", [1, 0])
def test_dense_compact_packed_and_slice_by_slice_inputs_agree(fmt):
    """the same picture through four input paths.  Compact levels take their offsets from a prefix sum over the CTU's coded blocks; the
    slice-by-slice picture keeps only its last call's TU lists, which a kernel driven from them would export alone"""
    torch = _torch()
    seq = make_seq(fmt=fmt)
    with Ctx(seq) as c:
        p = picture(seq, 1601 + fmt, True, 0.3, num_slices=4, tr_depth_max=3, intra_nxn_prob=0.4)
        ha = c.decode(p)
        check(c, ha, p, where="dense")
        a = c.ctx.export_transform([ha], "coeffs")
        hc = c.ctx.acquire()
        c.ctx.decompress_pictures([(hc, p.slices, p.meta, libhm_amd.pack_levels(seq, p.meta, p.coeffs))])
        check(c, hc, p, where="compact")
        hp = c.ctx.acquire()
        c.ctx.decompress_pictures_packed([(hp, p.slices, libhm_amd.pack_input(seq, p.meta, p.coeffs), None)])
        check(c, hp, p, where="packed")
        hs = c.ctx.acquire()
        for k, (first, n) in enumerate(p.slice_ranges):
            c.ctx.decompress_slice(hs, k, p.slices[k], p.meta, p.coeffs, first, n)
            if k < len(p.slice_ranges) - 1:
                assert c.ctx.transform_status([hs]) == abi.HMGPU_EINVAL
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    c.ctx.export_transform([hs])
                assert e.value.status == abi.HMGPU_EINVAL
        assert c.ctx.transform_status([hs]) == abi.HMGPU_OK
        check(c, hs, p, where="slice calls")
        for hx in (hc, hp, hs):
            b = c.ctx.export_transform([hx], "coeffs")
            assert all(torch.equal(a[k], b[k]) for k in a)
        c.ctx.sync()


def test_a_picture_decoded_without_intra_dir_exports_its_intra_cus():
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 1604, False, 0.5, cbf_prob=0.7)
        bare = {k: v for k, v in p.meta_np.items() if k not in ("intra_dir_l", "intra_dir_c")}
        p.meta = abi.MetaHolder(bare)
        h = c.decode(p)
        check(c, h, p, intra_dir=False, where="no intra_dir")
        info = tref.info_grid(seq, p.meta_np, False)
        intra = info[0] >= 0
        assert (info[4] == -1).all() and (info[5] == -1).all()
        # coefficients of intra CUs are there: coded luma blocks in intra CUs
        pm = np.asarray(p.meta_np["pred_mode"])
        assert any(b["comp"] == 0 and pm[b["ctu"], b["z"]] == abi.MODE_INTRA for b in tref.blocks(seq, p.meta_np)) and intra.any()
        with_dir = tref.info_grid(seq, p.meta_np, True)
        assert (with_dir[4] >= 0).any()
        c.ctx.sync()


def test_a_reused_handle_exports_nothing_of_its_earlier_pictures():
    """one handle fed from one staging block: a densely coded B picture, a P picture twenty times sparser, a PCM picture and one without
    the flag group (whose device copies are then not read).  The dense level array keeps the earlier levels wherever the current
    picture codes nothing: every uncovered element must be 0"""
    seq = base._pcm_seq()
    with Ctx(seq) as c:
        stg = c.ctx.staging_alloc()
        dense_b = picture(seq, 1501, True, 0.1, cbf_prob=0.9, tr_depth_max=2)
        sparse_p = picture(seq, 1502, False, 0.1, cbf_prob=0.045, tr_depth_max=2)
        pcm = base._with_pcm_and_lossless(picture(seq, 1505, False, 0.6, cbf_prob=0.9), 5)
        no_flags = picture(seq, 1506, False, 0.6, cbf_prob=0.9)
        h = c.ctx.acquire()
        density = {}
        for name, p in (("B", dense_b), ("P", sparse_p), ("pcm", pcm), ("noflags", no_flags)):
            c.ctx.sync()
            stg.fill(p.meta, p.coeffs)
            stg.set_groups(intra=True, flags=name == "pcm")
            for k in range(3):
                stg.coeffs.pcm_sample[k] = abi._ptr(p.coeffs.pcm[k]) if name == "pcm" else None
            c.ctx.decompress_pictures([(h, p.slices, stg, stg)])
            m = dict(p.meta_np)
            if name != "pcm":
                for k in ("ts_y", "ts_u", "ts_v", "bypass", "ipcm"):
                    m[k] = None
            want = tref.levels_planes(seq, m, p.coeffs.arrays)
            got = c.ctx.export_transform([h], "levels")
            for k in range(3):
                assert np.array_equal(bits(got[NAMES[k]][0]), want[k]), (name, k)
            assert np.array_equal(got["info"][0].cpu().numpy(), tref.info_grid(seq, m)), name
            density[name] = float((want[0] != 0).mean())
        assert density["B"] > 20 * density["P"] > 0, density
        c.ctx.sync()
        c.ctx.staging_free(stg)


# ------------------------------------------------------------------------------------------------ 3. destinations
def test_component_masks_views_misaligned_bases_and_single_destinations():
    torch = _torch()
    seq = make_seq()
    with Ctx(seq) as c:
        p = picture(seq, 1401, True, 0.3, tr_depth_max=2)
        h = c.decode(p)
        want = model(p, "coeffs")
        assert nonvacuous(want)
        info = tref.info_grid(seq, p.meta_np)
        for comps in ((0,), (1,), (2,), (0, 2), (1, 2)):
            got = c.ctx.export_transform([h], "coeffs", comps)
            assert sorted(got) == sorted([NAMES[k] for k in comps] + ["info"])
            assert all(np.array_equal(bits(got[NAMES[k]][0]), want[k]) for k in comps)
        # views of larger canary-filled tensors; odd offsets leave the base misaligned: the element-wise stores
        shapes = [(H, W), (H // 2, W // 2), (H // 2, W // 2), (H // 4, W // 4)]
        for off, pad in (((1, 3), (5, 9)), ((0, 0), (2, 8)), ((2, 1), (3, 1))):
            big, view = {}, {}
            for k, name in enumerate(NAMES + ("info",)):
                hh, ww = shapes[k]
                lead = (3, 7) if name == "info" else (3,)
                big[name] = torch.full(lead + (hh + pad[0], ww + pad[1]), CANARY if k < 3 else 0x5A, dtype=torch.int16 if k < 3 else torch.int8, device="cuda")
                view[name] = big[name][(slice(0, 2), slice(1, 7))[:len(lead)] + (slice(off[0], off[0] + hh), slice(off[1], off[1] + ww))]
            got = c.ctx.export_transform([h, h], "coeffs", out=view)
            torch.cuda.synchronize()
            for k, name in enumerate(NAMES + ("info",)):
                assert got[name] is view[name]
                for slot in range(2):
                    g = bits(view[name][slot]) if k < 3 else view[name][slot].cpu().numpy()
                    assert np.array_equal(g, want[k] if k < 3 else info), (name, slot, off)
                rest = big[name].clone()
                rest[(slice(0, 2), slice(1, 7))[:big[name].dim() - 2] + (slice(off[0], off[0] + shapes[k][0]), slice(off[1], off[1] + shapes[k][1]))].fill_(CANARY if k < 3 else 0x5A)
                assert bool((rest == (CANARY if k < 3 else 0x5A)).all()), (name, off)
        # each destination alone: only what is given is written
        for k, name in enumerate(NAMES + ("info",)):
            t = torch.zeros((1,) + ((6,) if k == 3 else ()) + shapes[k], dtype=torch.int16 if k < 3 else torch.int8, device="cuda")
            only = c.ctx.export_transform([h], "coeffs", out={name: t})
            assert list(only) == [name]
            g = bits(t[0]) if k < 3 else t[0].cpu().numpy()
            assert np.array_equal(g, want[k] if k < 3 else info), name
        c.ctx.sync()


@pytest.mark.parametrize("value", ["levels", "coeffs"])
def test_float_types_with_a_negative_scale(value):
    torch = _torch()
    seq = make_seq(bd=8)
    sc = (0.5, -0.37, 1.0 / 3.0)
    with Ctx(seq) as c:
        p = picture(seq, 1801, True, 0.3, tr_depth_max=2)
        h = c.decode(p)
        want = model(p, value)
        assert nonvacuous(want)
        for dtype, name in ((torch.float32, "float32"), (torch.float16, "float16"), (torch.bfloat16, "bfloat16")):
            got = c.ctx.export_transform([h], value, dtype=dtype, scale=sc)
            for k in range(3):
                ref = tref.convert(want[k], sc[k], name)
                assert np.array_equal(bits(got[NAMES[k]][0]), ref), (name, k)
            zero = tref.convert(np.zeros(1, dtype=np.int16), sc[1], name)[0]
            assert zero != 0 and (bits(got["cb"][0]) == zero).any()                              # -0 for the elements no block covers
        c.ctx.sync()


@pytest.mark.parametrize("n", [1, 3, 16])
def test_batches_of_mixed_pictures(n):
    seq = make_seq(max_pictures=8)
    with Ctx(seq) as c:
        ps = [picture(seq, 1701, False, 0.1, tr_depth_max=2), picture(seq, 1702, True, 0.4, tr_depth_max=2), as_i_picture(picture(seq, 1703, False, 1.0))]
        hs = [c.decode(p) for p in ps]
        wants = [model(p, "coeffs") for p in ps]
        infos = [tref.info_grid(seq, p.meta_np) for p in ps]
        assert all(nonvacuous(w) for w in wants)
        order = [(3 * i + i // 3) % 3 for i in range(n)]
        got = c.ctx.export_transform([hs[i] for i in order], "coeffs")
        assert tuple(got["info"].shape) == (n, 6, H // 4, W // 4)
        for slot, i in enumerate(order):
            for k in range(3):
                assert np.array_equal(bits(got[NAMES[k]][slot]), wants[i][k]), (slot, k)
            assert np.array_equal(got["info"][slot].cpu().numpy(), infos[i]), slot
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_destinations_untouched():
    torch = _torch()
    w, h = 200, 120
    seq = make_seq(w, h)
    with Ctx(seq) as c:
        p = picture(seq, 1951, True, 0.2, num_slices=2)
        good = c.decode(p)
        fresh = c.ctx.acquire()
        uploaded = c.ctx.acquire()
        c.ctx.decompress_pictures([(uploaded, p.slices, p.meta, p.coeffs)])
        c.ctx.upload(uploaded, synth.noise_planes(w, h, 10, 9))
        half = c.ctx.acquire()
        a, n = p.slice_ranges[0]
        c.ctx.decompress_slice(half, 0, p.slices[0], p.meta, p.coeffs, a, n)                     # partial coverage
        dst = {"y": torch.full((2, h, w), CANARY, dtype=torch.int16, device="cuda"),
               "cb": torch.full((2, h // 2, w // 2), CANARY, dtype=torch.int16, device="cuda"),
               "cr": torch.full((2, h // 2, w // 2), CANARY, dtype=torch.int16, device="cuda"),
               "info": torch.full((2, 6, h // 4, w // 4), 0x5A, dtype=torch.int8, device="cuda")}

        def untouched():
            torch.cuda.synchronize()
            c.ctx.sync()
            return all(bool((t == (0x5A if k == "info" else CANARY)).all()) for k, t in dst.items())

        for bad in (fresh, uploaded, half, 1, 63, -1):
            assert c.ctx.transform_status([good, bad]) == abi.HMGPU_EINVAL
            for pics in ([good, bad], [bad, good]):
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    c.ctx.export_transform(pics, out=dst)
                assert e.value.status == abi.HMGPU_EINVAL, bad
            assert untouched(), bad
        stream = torch.cuda.current_stream().cuda_stream
        picb, cpicb, ipl = h * w * 2, h * w // 2, (h // 4) * (w // 4)
        ptrs = [dst[k].data_ptr() for k in ("y", "cb", "cr", "info")]
        args = ([w * 2, w, w, w // 4], [0, 0, 0, ipl], [picb, cpicb, cpicb, 6 * ipl])
        ok = abi.make_transform_desc(abi.TRANSFORM_COEFFS, 7)
        assert c.ctx.transform_destination_status(2, ok, ptrs, *args) == abi.HMGPU_OK

        def desc(value=1, components=7, sample_type=abi.SAMPLE_UINT, scale=(1.0, 1.0, 1.0), reserved=None):
            d = abi.make_transform_desc(value, components, sample_type, scale)
            if reserved is not None:
                d.reserved[reserved] = 1
            return d

        bad_descs = [(desc(value=2), abi.HMGPU_EINVAL), (desc(value=-1), abi.HMGPU_EINVAL), (desc(components=0), abi.HMGPU_EINVAL),
                     (desc(components=8), abi.HMGPU_EINVAL), (desc(reserved=0), abi.HMGPU_EINVAL), (desc(reserved=5), abi.HMGPU_EINVAL),
                     (desc(sample_type=abi.SAMPLE_F16, scale=(1.0, float("nan"), 1.0)), abi.HMGPU_EINVAL),
                     (desc(sample_type=abi.SAMPLE_F32, scale=(float("inf"), 1.0, 1.0)), abi.HMGPU_EINVAL),
                     (desc(sample_type=9), abi.HMGPU_EUNSUPPORTED), (desc(sample_type=-1), abi.HMGPU_EUNSUPPORTED)]
        for d, status in bad_descs:
            assert c.ctx.transform_destination_status(2, d, ptrs, *args) == status
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_transform_into([good, good], d, ptrs, *args, 1, stream)
            assert e.value.status == status
        with pytest.raises(libhm_amd.HmgpuError) as e:                                            # the plan comes before the pictures
            c.ctx.export_transform_into([uploaded], desc(sample_type=9), ptrs, *args, 1, stream)
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        with pytest.raises(libhm_amd.HmgpuError) as e:                                            # 17 pictures
            c.ctx.export_transform_into([good] * 17, ok, ptrs, *args, 1, stream)
        assert e.value.status == abi.HMGPU_EINVAL
        assert untouched()
        # destination rules
        st = lambda pp, a0=args[0], a1=args[1], a2=args[2], d=ok, n=2: c.ctx.transform_destination_status(n, d, pp, a0, a1, a2)
        assert st([None] * 4) == abi.HMGPU_EINVAL                                                  # no destination
        assert st(ptrs, d=desc(components=5)) == abi.HMGPU_EINVAL                                  # Cb given but not selected
        assert st([ptrs[0], None, None, None], d=desc(components=5)) == abi.HMGPU_OK
        assert st(ptrs, a0=[w * 2 - 2, w, w, w // 4]) == abi.HMGPU_EINVAL                          # a pitch below a row
        assert st(ptrs, a0=[w * 2 + 1, w, w, w // 4], a2=[picb + h, cpicb, cpicb, 6 * ipl]) == abi.HMGPU_EINVAL    # an odd pitch
        assert st(ptrs, a2=[picb - 2, cpicb, cpicb, 6 * ipl]) == abi.HMGPU_EINVAL                  # a batch stride below a picture
        assert st(ptrs, a1=[0, 0, 0, ipl - 1]) == abi.HMGPU_EINVAL                                 # an info channel stride below a channel
        assert st(ptrs, a2=[picb, cpicb, cpicb, 6 * ipl - 1]) == abi.HMGPU_EINVAL
        assert st([ptrs[0] + 1] + ptrs[1:]) == abi.HMGPU_EINVAL                                    # a misaligned int16 base
        host = np.zeros(2 * picb, np.uint8)
        assert st([host.ctypes.data, None, None, None]) == abi.HMGPU_EINVAL                        # not device memory
        with pytest.raises(libhm_amd.HmgpuError) as e:
            c.ctx.export_transform_into([good, good], ok, [host.ctypes.data, None, None, None], *args, 1, stream)
        assert e.value.status == abi.HMGPU_EINVAL
        assert untouched()
        # the good picture still exports, into the same tensors
        c.ctx.export_transform([good, good], "coeffs", out=dst)
        want = model(p, "coeffs")
        assert all(np.array_equal(bits(dst[NAMES[k]][1]), want[k]) for k in range(3))
        assert np.array_equal(dst["info"][0].cpu().numpy(), tref.info_grid(seq, p.meta_np))
        c.ctx.sync()
