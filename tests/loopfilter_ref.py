"""A numpy model of the loop-filter export (include/hmgpu.h "loop-filter export"): what the edge grid, the SAO grid and
the dense form hold for a picture given as HM's per-partition arrays.  The boundary strengths come from the oracle
(oracle.boundary_strengths: z-scan per partition, already 0 where the unit is not filtered -- no edge, deblocking disabled for the Q
side's slice, a neighbour that is unavailable across a slice or tile border) and are folded to the grid of 4x4 blocks as tests/bs_ref.py
does; tc and beta come from the two tables of H.265 8.7.2 (Table 8-12), written out below as data, and the slice's offsets; chroma tc
from the chroma QP mapping of the format (Table 8-10 for 4:2:0, min(qPi, 51) otherwise); the SAO grid from the oracle's reconstructed
parameters (oracle.sao_reconstruct_params)."""
import numpy as np

# H.265 Table 8-12: tC' and beta' by Q
TC_TABLE = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7,
                     8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24], dtype=np.int64)
BETA_TABLE = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30,
                       32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64], dtype=np.int64)
# H.265 Table 8-10 (ChromaArrayType 1): QpC by qPi 0 .. 57
CHROMA_QP_420 = np.array(list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + [q - 6 for q in range(44, 58)], dtype=np.int64)
assert TC_TABLE.size == 54 and BETA_TABLE.size == 52 and CHROMA_QP_420.size == 58

EDGE_CHANNELS, SAO_CHANNELS = 13, 6
BS, QP, TC, BETA, TC_CB, TC_CR = 0, 2, 4, 6, 8, 10            # + 0 vertical, + 1 horizontal
FLAGS = 12
SAO_OFF_MODE, SAO_BO = 0, 4


def zscan_xy(parts):
    z = np.arange(parts)
    x = np.zeros(parts, dtype=np.int64)
    y = np.zeros(parts, dtype=np.int64)
    for b in range(8):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def raster(seq, a, fill=0):
    """[num_ctus, parts] in z order -> the picture's grid of 4x4 luma blocks [H / 4, W / 4]"""
    a = np.asarray(a).astype(np.int64)
    ctu = 1 << seq.log2_ctu_size
    cw = (seq.width + ctu - 1) // ctu
    n, parts = a.shape
    zx, zy = zscan_xy(parts)
    bx = (np.arange(n) % cw)[:, None] * (ctu // 4) + zx[None, :]
    by = (np.arange(n) // cw)[:, None] * (ctu // 4) + zy[None, :]
    ok = (bx < seq.width // 4) & (by < seq.height // 4)
    out = np.full((seq.height // 4, seq.width // 4), fill, dtype=np.int64)
    out[by[ok], bx[ok]] = a[ok]
    return out


def chroma_qp(qpi, fmt):
    """the chroma QP the deblocking filter derives from qPi = mean luma QP + PPS offset (xEdgeFilterChroma)"""
    qpi = np.asarray(qpi, dtype=np.int64)
    if fmt == 1:
        return np.where(qpi >= 58, qpi - 6, np.where(qpi >= 0, CHROMA_QP_420[np.clip(qpi, 0, 57)], qpi))
    return np.where(qpi >= 0, np.minimum(qpi, 51), qpi)


def _shift(a, axis):
    """the P side of every block: the block to the left (axis 1) / above (axis 0); the first column / row faces nothing (0)"""
    out = np.zeros_like(a)
    if axis == 1:
        out[:, 1:] = a[:, :-1]
    else:
        out[1:, :] = a[:-1, :]
    return out


def edge_grid(seq, slices, slice_idx, qp, exempt, bs_ver, bs_hor):
    """int16 [13, H / 4, W / 4].  slices: the abi.SliceParams of the picture; slice_idx [num_ctus]; qp, exempt (lossless CU, or PCM CU
    with pcm_loop_filter_disable), bs_ver, bs_hor [num_ctus, parts] in z order, the last two the oracle's"""
    h4, w4 = seq.height // 4, seq.width // 4
    fmt = seq.chroma_format
    csx, csy = (1 if fmt in (1, 2) else 0), (1 if fmt == 1 else 0)
    by, bx = np.meshgrid(np.arange(h4), np.arange(w4), indexing="ij")
    parts = np.asarray(qp).shape[1]
    per_ctu = lambda v: raster(seq, np.repeat(np.asarray(v, dtype=np.int64)[:, None], parts, axis=1))
    sidx = np.asarray(slice_idx, dtype=np.int64)
    field = lambda name: per_ctu(np.array([getattr(slices[int(s)], name) for s in sidx]))
    tc_off, beta_off, cb_off, cr_off = field("tc_offset_div2"), field("beta_offset_div2"), field("pps_cb_qp_offset"), field("pps_cr_qp_offset")
    q, ex = raster(seq, qp), raster(seq, exempt)
    out = np.zeros((EDGE_CHANNELS, h4, w4), dtype=np.int64)
    for d, bs_z in enumerate((bs_ver, bs_hor)):
        on_grid = (bx % 2 == 0) if d == 0 else (by % 2 == 0)
        bs = np.where(on_grid, raster(seq, bs_z), 0)
        assert bs.max() <= 2
        on = bs > 0
        qp_avg = (_shift(q, 1 - d) + q + 1) >> 1
        tc = TC_TABLE[np.clip(qp_avg + 2 * (bs - 1) + 2 * tc_off, 0, 53)] << (seq.bit_depth_luma - 8)
        beta = BETA_TABLE[np.clip(qp_avg + 2 * beta_off, 0, 51)] << (seq.bit_depth_luma - 8)
        # the chroma filter acts where Bs is 2 on the chroma plane's own 8-sample grid: 16 luma samples across a subsampled direction
        step = (8 << csx) if d == 0 else (8 << csy)
        chroma_on = (bs == 2) & (((bx if d == 0 else by) * 4) % step == 0) & (fmt != 0)
        out[BS + d] = bs
        out[QP + d] = np.where(on, qp_avg, 0)
        out[TC + d] = np.where(on, tc, 0)
        out[BETA + d] = np.where(on, beta, 0)
        for c, off in ((TC_CB, cb_off), (TC_CR, cr_off)):
            tcc = TC_TABLE[np.clip(chroma_qp(qp_avg + off, 1 if fmt == 0 else fmt) + 2 + 2 * tc_off, 0, 53)] << (seq.bit_depth_chroma - 8)
            out[c + d] = np.where(chroma_on, tcc, 0)
        out[FLAGS] |= np.where(on, (_shift(ex, 1 - d) != 0) * 1 + (ex != 0) * 2, 0) << (2 * d)
    return out.astype(np.int16)


def exempt_of(seq, meta_np):
    """[num_ctus, parts]: the partition's CU keeps its samples in the loop filters"""
    z = np.zeros(np.asarray(meta_np["depth"]).shape, dtype=bool)
    byp = np.asarray(meta_np["bypass"]) != 0 if meta_np.get("bypass") is not None else z
    pcm = np.asarray(meta_np["ipcm"]) != 0 if meta_np.get("ipcm") is not None else z
    return byp | (pcm & bool(seq.pcm_loop_filter_disable))


def sao_grid(seq, rec, enabled=True):
    """int8 [3, 6, ctus_h, ctus_w] from the oracle's reconstructed parameters rec [num_ctus, 3, 35] (mode, type, aux, offset[32]);
    enabled False: the picture's last filter call ran no SAO stage.  4:0:0: the chroma components are None-like -- callers compare
    component 0 only"""
    ctu = 1 << seq.log2_ctu_size
    cw, ch = (seq.width + ctu - 1) // ctu, (seq.height + ctu - 1) // ctu
    out = np.zeros((3, SAO_CHANNELS, ch, cw), dtype=np.int64)
    out[:, 0] = -1
    if not enabled:
        return out.astype(np.int8)
    rec = np.asarray(rec).reshape(ch, cw, 3, 35)
    for comp in range(3):
        r = rec[:, :, comp]
        mode, typ, aux, off = r[..., 0], r[..., 1], r[..., 2], r[..., 3:]
        on = mode != SAO_OFF_MODE
        bo = on & (typ == SAO_BO)
        eo = on & ~bo
        out[comp, 0] = np.where(on, typ, -1)
        out[comp, 1] = np.where(bo, aux & 31, 0)
        for i in range(4):
            band = np.take_along_axis(off, ((aux + i) % 32)[..., None], axis=-1)[..., 0]
            out[comp, 2 + i] = np.where(bo, band, np.where(eo, off[..., (0, 1, 3, 4)[i]], 0))
    assert np.abs(out).max() < 128
    return out.astype(np.int8)


def nearest_src(o, n_in, n_out):
    """the integer nearest rule of the dense forms: output o of n_out -> source sample of n_in"""
    return np.minimum(((2 * np.asarray(o, dtype=np.int64) + 1) * n_in) // (2 * n_out), n_in - 1)


def dense(seq, edge, sao, window, size=None, flip=False):
    """uint8-valued int64 [3, oh, ow] from the picture's edge grid [13, H / 4, W / 4] and SAO grid [3, 6, ch, cw]; window (x, y, w, h)
    in luma samples; size (oh, ow) or None (the window's)"""
    x0, y0, w, h = window
    oh, ow = (h, w) if size is None else size
    xs = x0 + nearest_src(np.arange(ow), w, ow)
    ys = y0 + nearest_src(np.arange(oh), h, oh)
    if flip:
        xs = xs[::-1]
    X, Y = np.meshgrid(xs, ys)
    out = np.zeros((3, oh, ow), dtype=np.int64)
    e = (X + 4) & ~7
    out[0] = np.where((e == 0) | (e >= seq.width), 0, edge[BS][Y >> 2, np.minimum(e, seq.width - 4) >> 2])
    e = (Y + 4) & ~7
    out[1] = np.where((e == 0) | (e >= seq.height), 0, edge[BS + 1][np.minimum(e, seq.height - 4) >> 2, X >> 2])
    out[2] = sao[0, 0][Y >> seq.log2_ctu_size, X >> seq.log2_ctu_size].astype(np.int64) + 1
    return out


def dense_brute(seq, edge, sao, window, size=None, flip=False):
    """dense() sample by sample, in the words of the header: for the tests of the model itself"""
    x0, y0, w, h = window
    oh, ow = (h, w) if size is None else size
    out = np.zeros((3, oh, ow), dtype=np.int64)
    for oy in range(oh):
        y = y0 + min(((2 * oy + 1) * h) // (2 * oh), h - 1)
        for oc in range(ow):
            ox = ow - 1 - oc if flip else oc
            x = x0 + min(((2 * ox + 1) * w) // (2 * ow), w - 1)
            e = (x + 4) & ~7
            if e != 0 and e < seq.width:
                out[0, oy, oc] = edge[BS][y >> 2, e >> 2]
            e = (y + 4) & ~7
            if e != 0 and e < seq.height:
                out[1, oy, oc] = edge[BS + 1][e >> 2, x >> 2]
            out[2, oy, oc] = int(sao[0, 0][y >> seq.log2_ctu_size, x >> seq.log2_ctu_size]) + 1
    return out


def picture_model(oracle, p, sao_enabled=True):
    """(edge grid, SAO grid) of a tests/synth.py picture p, the oracle given"""
    bv, bh = oracle.boundary_strengths(p.seq, p.slices, p.meta, p.pp)
    m = p.meta_np
    sidx = m["slice_idx"] if m.get("slice_idx") is not None else np.zeros(p.num_ctus, dtype=np.int64)
    edge = edge_grid(p.seq, p.slices, sidx, m["qp"], exempt_of(p.seq, m), bv, bh)
    sao = sao_grid(p.seq, oracle.sao_reconstruct_params(p.seq, p.pp, p.meta, p.sao_raw) if sao_enabled else None, sao_enabled)
    return edge, sao
