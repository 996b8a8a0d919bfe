"""Motion and block export on the GPU (hmgpu_pictures_export_motion, k_motion.hip) behind Context.export_motion,
hmdec.export_motion_batch, Picture.motion and Decoder.frames(motion=): every plane bit for bit against the numpy model
(tests/motion_ref.py) -- both forms, every CTU size, stale list groups in reused handles, slices with their own reference lists,
batches into strided views with guard bytes, packed input, the refusals, and the decoder."""
import ctypes as C

import numpy as np
import pytest

import libhm_amd
from libhm_amd import abi, hmdec, motion
from tests import golden_util as gu
from tests import motion_ref as mref
from tests import synth

pytestmark = pytest.mark.gpu

NO_AMP = (0.1, 0.3, 0.3, 0.3, 0.0)          # (AMP CUs are inter only: an all-intra picture has none)


def _torch():
    import torch
    return torch


def bits(t):
    """a tensor's elements on the host: integers as they are, floats as bit patterns of their own width"""
    torch = _torch()
    if t.dtype in (torch.int8, torch.int16, torch.int32):
        return t.cpu().numpy()
    view = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(view).cpu().numpy().view({2: np.uint16, 4: np.uint32}[t.element_size()])


def make_seq(w, h, log2_ctu=6, fmt=1, max_pictures=10):
    seq = abi.make_seq(w, h, 10, 10, log2_ctu=log2_ctu, max_pictures=max_pictures)
    seq.chroma_format = fmt
    return seq


def picture(seq, seed, bi=False, intra_frac=0.0, **kw):
    kw.setdefault("mode_probs", NO_AMP if intra_frac >= 1.0 else (0.1, 0.3, 0.3, 0.2, 0.1))
    return synth.make_picture(seq.width, seq.height, 10, seed=seed, bi=bi, intra_frac=intra_frac, num_refs=2, ref_handles=([0, 1], [1]),
                              chroma_format=seq.chroma_format, log2_ctu=seq.log2_ctu_size, **kw)


def as_i_picture(p):
    """an all-intra synthetic picture as an I slice without reference lists"""
    sl = abi.clone_slice(p.slice)
    sl.slice_type = abi.I_SLICE
    sl.num_ref_idx[0] = sl.num_ref_idx[1] = 0
    p.slice, p.slices = sl, [sl]
    return p


class Ctx:
    """a context with two uploaded reference pictures (handles 0 and 1)"""

    def __init__(self, seq):
        self.seq = seq
        self.ctx = libhm_amd.Context(seq)
        for k in range(2):
            h = self.ctx.acquire()
            assert h == k
            self.ctx.upload(h, synth.noise_planes(seq.width, seq.height, 10, 5 + k, seq.chroma_format))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.__exit__(*a)

    def decode(self, p, h=None):
        h = self.ctx.acquire() if h is None else h
        self.ctx.decompress_pictures([(h, p.slices, p.meta, p.coeffs)])
        return h

    def want_blocks(self, p, lists=3, crop=(0, 0, 0, 0)):
        return mref.blocks(p.meta_np, p.slices, self.seq.width, self.seq.height, self.seq.log2_ctu_size, lists, crop)

    def check_blocks(self, h, p, lists=(0, 1), crop=(0, 0, 0, 0), where=""):
        got = self.ctx.export_motion([h], "blocks", lists, crop=crop)
        want = self.want_blocks(p, motion.lists_mask(lists), crop)
        for k in ("mv", "ref_poc", "block"):
            assert got[k].shape[1:] == want[k].shape, (where, k)
            assert np.array_equal(bits(got[k][0]), want[k]), (where, k, lists, crop)
        return got


# ------------------------------------------------------------------------------------------------ 1. BLOCKS against the model
GEOMETRIES = [(200, 120, 6, 1), (104, 56, 5, 1), (104, 56, 4, 1), (104, 56, 5, 3), (200, 120, 6, 0)]


@pytest.mark.parametrize("w,h,log2_ctu,fmt", GEOMETRIES)
def test_blocks_match_the_model(w, h, log2_ctu, fmt):
    """P and B pictures with no, some and only intra CUs; partial CTUs on both borders; all three planes, every lists mask, and a
    crop whose left edge is no multiple of four blocks"""
    seq = make_seq(w, h, log2_ctu, fmt)
    kinds = [(bi, fr) for bi in (False, True) for fr in (0.0, 0.3, 1.0)] if fmt == 1 else [(True, 0.3)]
    with Ctx(seq) as c:
        for i, (bi, fr) in enumerate(kinds):
            p = picture(seq, 100 + i, bi, fr)
            hnd = c.decode(p)
            for lists in ((0,), (1,), (0, 1)):
                got = c.check_blocks(hnd, p, lists, where=(w, h, log2_ctu, fmt, bi, fr))
            if bi and fr < 1.0:
                assert bool((got["mv"][0, 1] != 0).any()) and bool((got["ref_poc"] == abi.MOTION_NO_REF).any())
            c.check_blocks(hnd, p, (0, 1), (4, 8, 8, 4), where="crop")
            c.check_blocks(hnd, p, (1,), (16, 0, 0, 12), where="crop16")
            c.ctx.release(hnd)


def test_stale_groups_of_a_reused_handle_are_not_read():
    """a B picture, then a P picture, then an I picture in ONE handle, each from a staging block: calls without B slices do not copy
    the list-1 group, so the device still holds the B picture's list-1 vectors -- the slice type keeps them out"""
    seq = make_seq(200, 120)
    with Ctx(seq) as c:
        stg = c.ctx.staging_alloc()
        pb, pp, pi = picture(seq, 1, True, 0.1), picture(seq, 2, False, 0.1), as_i_picture(picture(seq, 3, False, 1.0))
        h = None
        for name, p in (("B", pb), ("P", pp), ("I", pi)):
            if h is not None:
                c.ctx.release(h)
            h2 = c.ctx.acquire()
            assert h is None or h2 == h
            h = h2
            c.ctx.sync()
            stg.fill(p.meta, p.coeffs)
            c.ctx.decompress_pictures([(h, p.slices, stg, stg)])
            got = c.check_blocks(h, p, (0, 1), where=name)
            l1_used = bool((got["ref_poc"][0, 1] != abi.MOTION_NO_REF).any())
            assert l1_used == (name == "B")
            if name != "B":
                assert not bool(got["mv"][0, 1].any())
            if name == "I":
                assert not bool(got["mv"].any()) and bool((got["ref_poc"] == abi.MOTION_NO_REF).all()) and bool((got["block"][0, 0] == 1).all())
        c.ctx.sync()
        c.ctx.staging_free(stg)


def test_five_slices_with_their_own_reference_lists():
    seq = make_seq(200, 120)
    with Ctx(seq) as c:
        p = picture(seq, 11, True, 0.2, num_slices=5)
        for k, sl in enumerate(p.slices):
            for l in range(2):
                for i in range(sl.num_ref_idx[l]):
                    sl.ref_poc[l][i] = 1000 * k + 100 * l + i - 37
        h = c.decode(p)
        got = c.check_blocks(h, p)
        assert len(np.unique(bits(got["ref_poc"]))) >= 6
        # the same picture slice by slice: no side information until the last CTU range has been handed over
        h2 = c.ctx.acquire()
        for k, (a, n) in enumerate(p.slice_ranges):
            with_all = k == len(p.slice_ranges) - 1
            c.ctx.decompress_slice(h2, k, p.slices[k], p.meta, p.coeffs, a, n)
            if not with_all:
                with pytest.raises(libhm_amd.HmgpuError) as e:
                    c.ctx.export_motion([h2])
                assert e.value.status == abi.HMGPU_EINVAL
        c.check_blocks(h2, p, where="slice calls")


# ------------------------------------------------------------------------------------------------ 2. batches, strides, guard bytes
CANARY = {"mv": 0x5A5A, "ref_poc": 0x5A5A5A5A, "block": 0x5A}


@pytest.mark.parametrize("pad,off", [((0, 14), (0, 0)), ((3, 5), (1, 2))])
def test_batch_equals_single_calls_and_respects_strides(pad, off):
    """P, B, I and a P picture from a staging block in one call, a repeated handle, into views of larger canary-filled tensors: rows,
    planes and batch entries further apart than they need be (once with 64-element rows at offset 0: the vector stores; once at an
    odd offset: the scalar ones); nothing outside the views changes"""
    torch = _torch()
    seq = make_seq(200, 120)
    h4, w4 = 30, 50
    with Ctx(seq) as c:
        ps = [picture(seq, 21, False, 0.1), picture(seq, 22, True, 0.3), as_i_picture(picture(seq, 23, False, 1.0)), picture(seq, 24, False, 0.0)]
        hs = [c.decode(p) for p in ps[:3]]
        stg = c.ctx.staging_alloc()
        stg.fill(ps[3].meta, ps[3].coeffs)
        hs.append(c.ctx.acquire())
        c.ctx.decompress_pictures([(hs[3], ps[3].slices, stg, stg)])
        singles = [c.ctx.export_motion([h]) for h in hs]
        order = [0, 1, 2, 3, 1]
        big = {"mv": torch.full((6, 2, 2, h4 + pad[0], w4 + pad[1]), CANARY["mv"], dtype=torch.int16, device="cuda"),
               "ref_poc": torch.full((6, 3, h4 + pad[0], w4 + pad[1]), CANARY["ref_poc"], dtype=torch.int32, device="cuda"),
               "block": torch.full((6, 5, h4 + pad[0], w4 + pad[1]), CANARY["block"], dtype=torch.int8, device="cuda")}
        sl = (slice(off[0], off[0] + h4), slice(off[1], off[1] + w4))
        out = {"mv": big["mv"][(slice(0, 5), slice(None), slice(None)) + sl], "ref_poc": big["ref_poc"][(slice(0, 5), slice(0, 2)) + sl],
               "block": big["block"][(slice(0, 5), slice(0, 4)) + sl]}
        got = c.ctx.export_motion([hs[i] for i in order], out=out)
        torch.cuda.synchronize()
        for k in out:
            assert got[k] is out[k]
            for slot, i in enumerate(order):
                assert torch.equal(out[k][slot], singles[i][k][0]), (k, slot)
                assert np.array_equal(bits(out[k][slot]), c.want_blocks(ps[i])[k]), (k, slot)
            rest = big[k].clone()
            lead = {"mv": (slice(0, 5), slice(None), slice(None)), "ref_poc": (slice(0, 5), slice(0, 2)), "block": (slice(0, 5), slice(0, 4))}[k]
            rest[lead + sl].fill_(CANARY[k])
            assert bool((rest == CANARY[k]).all()), k
        # a subset of the destinations: only what is given is written
        only = c.ctx.export_motion([hs[1]], lists=(1,), out={"ref_poc": torch.zeros((1, 1, h4, w4), dtype=torch.int32, device="cuda")})
        assert list(only) == ["ref_poc"] and np.array_equal(bits(only["ref_poc"][0]), c.want_blocks(ps[1], 2)["ref_poc"])
        c.ctx.sync()
        c.ctx.staging_free(stg)


def test_packed_input_exports_the_same_planes():
    seq = make_seq(200, 120)
    with Ctx(seq) as c:
        for i, (bi, fr) in enumerate(((True, 0.3), (False, 0.1))):
            p = picture(seq, 31 + i, bi, fr)
            ha = c.decode(p)
            hp = c.ctx.acquire()
            blob = libhm_amd.pack_input(seq, p.meta, p.coeffs)
            c.ctx.decompress_pictures_packed([(hp, p.slices, blob, None)])
            a, b = c.check_blocks(ha, p), c.check_blocks(hp, p, where="packed")
            for k in a:
                assert _torch().equal(a[k], b[k]), k
            c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 3. DENSE against the model
SCALED = [((0, 0, 200, 120), False), ((36, 20, 96, 64), True), ((2, 6, 8, 8), False)]       # -> 64 x 64; the last: 8x, origin no multiple of 4
UNSCALED = [((0, 0, 96, 64), False), ((104, 56, 96, 64), True)]


def _check_dense(c, h, p, windows, size, dtype, st, lists=(0, 1)):
    torch = _torch()
    got = c.ctx.export_motion([h] * len(windows), "dense", lists, size=size, windows=[w for w, _ in windows], flip=[f for _, f in windows],
                              dtype=dtype)
    mask = motion.lists_mask(lists)
    assert sorted(got) == sorted(["flow%d" % l for l in range(2) if (mask >> l) & 1] + ["ref_poc", "block"])
    for slot, (win, flip) in enumerate(windows):
        want = mref.dense(p.meta_np, p.slices, c.seq.width, c.seq.height, c.seq.log2_ctu_size, win, size, flip, st, mask)
        for k in got:
            assert got[k].dtype == (dtype if k.startswith("flow") else torch.int32 if k == "ref_poc" else torch.int8)
            assert np.array_equal(bits(got[k][slot]), want[k]), (k, slot, win, flip, size, st)
    return got


def test_dense_matches_the_model_bit_for_bit():
    torch = _torch()
    seq = make_seq(200, 120)
    with Ctx(seq) as c:
        p = picture(seq, 41, True, 0.3)
        h = c.decode(p)
        for dtype, st in ((torch.float32, abi.SAMPLE_F32), (torch.float16, abi.SAMPLE_F16), (torch.bfloat16, abi.SAMPLE_BF16)):
            got = _check_dense(c, h, p, SCALED, (64, 64), dtype, st)
            assert bool((got["flow0"] != 0).any()) and bool((got["flow1"] != 0).any())
            _check_dense(c, h, p, UNSCALED, None, dtype, st)
            _check_dense(c, h, p, SCALED[:2], (37, 51), dtype, st, lists=(1,))           # partial groups, rows that are not 16-byte multiples
        _check_dense(c, h, p, [((4, 2, 192, 64), True)], (2, 6), torch.float16, abi.SAMPLE_F16)   # the 32x reduction
        # alignment with the pixel export: the block under every output sample is the block of the luma position the scaled pixel
        # export reads for it (its nearest table), mirrored slots reversed
        g = mref.grid(p.meta_np, p.slices, 200, 120, 6)
        got = c.ctx.export_motion([h] * 3, "dense", size=(64, 64), windows=[w for w, _ in SCALED], flip=[f for _, f in SCALED])
        for slot, ((x, y, w, hh), flip) in enumerate(SCALED):
            desc = abi.make_export_desc(abi.EXPORT_RGB, 8, 1, 0, (x, 200 - x - w, y, 120 - y - hh), 1, 0)
            sc = abi.make_export_scale(64, 64, abi.SCALE_NEAREST)
            fx, cx, _ = libhm_amd.export_scale_taps(seq, desc, sc, 0, 0)
            fy, cy, _ = libhm_amd.export_scale_taps(seq, desc, sc, 0, 1)
            assert (cx == 1).all() and (cy == 1).all()
            pick = np.ix_((y + fy) >> 2, (x + fx) >> 2)
            blk, ref = g["block"][(slice(None),) + pick], g["ref_poc"][(slice(None),) + pick]
            if flip:
                blk, ref = blk[:, :, ::-1], ref[:, :, ::-1]
            assert np.array_equal(bits(got["block"][slot]), blk) and np.array_equal(bits(got["ref_poc"][slot]), ref), slot
        # the unscaled pair (one slot mirrored): the pixel export copies luma sample (x + ox, y + oy), the block is the one under it
        got = c.ctx.export_motion([h] * 2, "dense", windows=[w for w, _ in UNSCALED], flip=[f for _, f in UNSCALED])
        for slot, ((x, y, w, hh), flip) in enumerate(UNSCALED):
            pick = np.ix_((y + np.arange(hh)) >> 2, (x + np.arange(w)) >> 2)
            blk, ref = g["block"][(slice(None),) + pick], g["ref_poc"][(slice(None),) + pick]
            if flip:
                blk, ref = blk[:, :, ::-1], ref[:, :, ::-1]
            assert np.array_equal(bits(got["block"][slot]), blk) and np.array_equal(bits(got["ref_poc"][slot]), ref), slot
        # and the pixel export accepts the same windows, flips and size
        rgb = c.ctx.export_batch([h] * 3, "rgb", 8, size=(64, 64), filter="nearest", windows=[w for w, _ in SCALED], flip=[f for _, f in SCALED])
        assert tuple(rgb.shape) == (3, 3, 64, 64)
        c.ctx.sync()


# ------------------------------------------------------------------------------------------------ 4. refusals
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


def test_refusals_leave_the_destination_untouched():
    torch = _torch()
    seq = make_seq(200, 120)
    h4, w4 = 30, 50
    with Ctx(seq) as c:
        p = picture(seq, 51, True, 0.2, num_slices=2)
        good = c.decode(p)
        fresh = c.ctx.acquire()
        uploaded = c.ctx.acquire()
        c.ctx.decompress_pictures([(uploaded, p.slices, p.meta, p.coeffs)])
        c.ctx.upload(uploaded, synth.noise_planes(200, 120, 10, 9))
        half = c.ctx.acquire()
        a, n = p.slice_ranges[0]
        c.ctx.decompress_slice(half, 0, p.slices[0], p.meta, p.coeffs, a, n)
        dst = {"mv": torch.full((2, 2, 2, h4, w4), CANARY["mv"], dtype=torch.int16, device="cuda"),
               "ref_poc": torch.full((2, 2, h4, w4), CANARY["ref_poc"], dtype=torch.int32, device="cuda"),
               "block": torch.full((2, 4, h4, w4), CANARY["block"], dtype=torch.int8, device="cuda")}

        def untouched():
            torch.cuda.synchronize()
            c.ctx.sync()
            return all(bool((dst[k] == CANARY[k]).all()) for k in dst)

        for bad in (fresh, uploaded, half, 1, 63, -1):           # (handle 1: an uploaded reference picture; 63 / -1: no picture)
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_motion([good, bad], out=dst)
            assert e.value.status == abi.HMGPU_EINVAL, bad
            assert untouched(), bad
        # a destination that does not lie inside one allocation: room for two pictures less one element
        desc = abi.make_motion_desc(abi.MOTION_BLOCKS, 3)
        stream = torch.cuda.current_stream().cuda_stream
        t = dst["ref_poc"]
        plane, picb = h4 * w4 * 4, 2 * h4 * w4 * 4
        args = ([0, 0, w4 * 4, 0], [0, 0, plane, 0], [0, 0, picb, 0])
        hip = _hip()
        raw = C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), 2 * picb - 4) == 0
        try:
            assert hip.hipMemset(raw, 0x5A, 2 * picb - 4) == 0
            ptrs = [None, None, raw.value, None]
            assert c.ctx.motion_destination_status(2, desc, ptrs, *args) == abi.HMGPU_EINVAL
            with pytest.raises(libhm_amd.HmgpuError) as e:
                c.ctx.export_motion_into([good, good], desc, ptrs, *args, 1, stream)
            assert e.value.status == abi.HMGPU_EINVAL
            torch.cuda.synchronize()
            c.ctx.sync()
            back = np.zeros(2 * picb - 4, np.uint8)
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 4, 2) == 0
            assert (back == 0x5A).all()
            c.ctx.export_motion_into([good], desc, ptrs, *args, 1, stream)                        # one picture fits
            torch.cuda.synchronize()
            assert hip.hipMemcpy(back.ctypes.data, raw, 2 * picb - 4, 2) == 0
            assert np.array_equal(back[:picb].view(np.int32).reshape(2, h4, w4), c.want_blocks(p)["ref_poc"]) and (back[picb:] == 0x5A).all()
        finally:
            hip.hipFree(raw)
        # strides below the extents they step over, a misaligned pointer, no destination at all
        ok = [None, None, t.data_ptr(), None]
        assert c.ctx.motion_destination_status(2, desc, ok, *args) == abi.HMGPU_OK
        for bad_args in (([0, 0, w4 * 4 - 4, 0], args[1], args[2]), (args[0], [0, 0, plane - 4, 0], args[2]), (args[0], args[1], [0, 0, picb - 4, 0])):
            assert c.ctx.motion_destination_status(2, desc, ok, *bad_args) == abi.HMGPU_EINVAL
        assert c.ctx.motion_destination_status(2, desc, [None, None, t.data_ptr() + 2, None], *args) == abi.HMGPU_EINVAL
        assert c.ctx.motion_destination_status(2, desc, [None] * 4, *args) == abi.HMGPU_EINVAL
        assert c.ctx.motion_destination_status(1, desc, [None, dst["mv"].data_ptr(), None, None], [0, w4 * 2, 0, 0], [0, h4 * w4 * 2, 0, 0],
                                               [0, 4 * h4 * w4 * 2, 0, 0]) == abi.HMGPU_EINVAL      # (BLOCKS has no second vector slot)
        assert untouched()
        # the pictures are checked before the plan: a dense export of the uploaded picture whose scale asks for a filter the export does
        # not have (by the plan alone: HMGPU_EUNSUPPORTED)
        dense = abi.make_motion_desc(abi.MOTION_DENSE, 3, abi.SAMPLE_F32)
        whole = [abi.make_export_window((0, 0, 0, 0))]
        bilinear = abi.make_export_scale(w4, h4, abi.SCALE_BILINEAR)
        with pytest.raises(libhm_amd.HmgpuError) as e:
            c.ctx.export_motion_into([uploaded], dense, ok, *args, 1, stream, bilinear, whole)
        assert e.value.status == abi.HMGPU_EINVAL
        with pytest.raises(libhm_amd.HmgpuError) as e:
            c.ctx.export_motion_into([good], dense, ok, *args, 1, stream, bilinear, whole)
        assert e.value.status == abi.HMGPU_EUNSUPPORTED
        assert untouched()
        # the good picture still exports
        c.check_blocks(good, p)


# ------------------------------------------------------------------------------------------------ 5. through libhmdec
def _model_of(pic, lists=3):
    g = pic.geometry()
    n = g["num_ctbs"]
    meta = {k: pic.array(k).reshape(n, -1) for k in ("depth", "part_size", "pred_mode", "qp", "ref_idx0", "ref_idx1")}
    meta["mv0"], meta["mv1"] = pic.array("mv0").reshape(n, -1, 2), pic.array("mv1").reshape(n, -1, 2)
    meta["slice_idx"] = pic.array("slice_idx")
    slices = [pic.slice_params(i)[0] for i in range(pic.num_slices())]
    return meta, slices, g


@pytest.mark.parametrize("kw", [dict(threads=1), dict(threads=3), dict(threads=1, devices=[0, 0])], ids=["t1", "t3", "two_contexts"])
@pytest.mark.parametrize("name", ["ra_main10_208x120", "ldp_main8_416x240"])
def test_decoder_pictures_export_their_motion(name, kw):
    """every output picture of two fixture streams: hmdec.export_motion_batch equals the model on the parser's own arrays"""
    z = gu.load("stream_" + name)
    seen = []
    with hmdec.Decoder(device=0, device_output=True, **kw) as d:
        def on_output(pic):
            meta, slices, g = _model_of(pic)
            want = mref.blocks(meta, slices, g["width"], g["height"], g["log2_ctb"])
            got = hmdec.export_motion_batch([pic])
            for k in want:
                assert np.array_equal(bits(got[k][0]), want[k]), (name, pic.poc, k)
            one = pic.motion(lists=(0,))
            assert np.array_equal(bits(one["mv"]), want["mv"][:1]) and one["block"].shape == want["block"].shape
            seen.append((pic.poc, bool(want["mv"].any())))
        d.decode_stream(z["bitstream"], on_output=on_output)
        assert d.hash_mismatches == 0
    assert len(seen) >= 3 and any(moving for _, moving in seen)


def test_frames_yield_motion_beside_the_pictures():
    """Decoder.frames(batch=4, motion=..., windows=fn): the motion dict of every item equals separate per-picture calls with the
    windows and flips fn returned for that batched call; motion=True gives the block grids"""
    torch = _torch()
    name = "ra_main10_208x120"
    z = gu.load("stream_" + name)
    rng = np.random.RandomState(5)
    calls = []

    def fn(n):
        wins = [(int(2 * rng.randint(0, 40)), int(2 * rng.randint(0, 20)), 96, 64) for _ in range(n)]
        flips = [bool(rng.randint(0, 2)) for _ in range(n)]
        calls.append((wins, flips))
        return wins, flips

    with hmdec.Decoder(device=0, device_output=True) as d:
        dense = [(pocs, rgb.clone(), {k: t.clone() for k, t in m.items()})
                 for pocs, rgb, m in d.frames(z["bitstream"], batch=4, windows=fn, size=(32, 48), filter="nearest",
                                              motion=dict(form=abi.MOTION_DENSE, dtype=torch.float16))]      # (the form as its code)
        for bad in (dict(form="dense", windows=[(0, 0, 96, 64)]), dict(form="dense", flip=[True]), dict(out={})):
            with pytest.raises(ValueError):
                next(d.frames(z["bitstream"], batch=4, windows=fn if "out" not in bad else None, size=(32, 48), filter="nearest", motion=bad))
    with hmdec.Decoder(device=0, device_output=True) as d:
        grids = [(pocs, {k: t.clone() for k, t in m.items()}) for pocs, _, m in d.frames(z["bitstream"], batch=4, motion=True)]
    windows = [wf for wins, flips in calls for wf in zip(wins, flips)]                  # in output order, one per picture
    order = [poc for pocs, _, _ in dense for poc in pocs]
    assert order == [poc for pocs, _ in grids for poc in pocs] and len(windows) == len(order)
    want_dense, want_grid = {}, {}
    with hmdec.Decoder(device=0, device_output=True) as d:
        def on_output(pic):
            win, flip = windows[order.index(pic.poc)]
            want_dense[pic.poc] = {k: t.clone() for k, t in pic.motion("dense", size=(32, 48), window=win, flip=flip, dtype=torch.float16).items()}
            want_grid[pic.poc] = {k: t.clone() for k, t in pic.motion().items()}
            meta, slices, g = _model_of(pic)
            m = mref.dense(meta, slices, g["width"], g["height"], g["log2_ctb"], win, (32, 48), flip, abi.SAMPLE_F16)
            for k in want_dense[pic.poc]:
                assert np.array_equal(bits(want_dense[pic.poc][k]), m[k]), (pic.poc, k)
        d.decode_stream(z["bitstream"], on_output=on_output)
    for pocs, rgb, m in dense:
        assert rgb.shape[0] == len(pocs) and sorted(m) == ["block", "flow0", "flow1", "ref_poc"]
        for slot, poc in enumerate(pocs):
            for k in m:
                assert m[k].shape[0] == len(pocs) and torch.equal(m[k][slot], want_dense[poc][k]), (poc, k)
    for pocs, m in grids:
        assert sorted(m) == ["block", "mv", "ref_poc"]
        for slot, poc in enumerate(pocs):
            for k in m:
                assert torch.equal(m[k][slot], want_grid[poc][k]), (poc, k)
