"""Pattern pictures for the loop filters: pictures whose reconstruction is EXACTLY a crafted picture, so that what deblocking and SAO see is
chosen sample by sample instead of being whatever motion compensation of noise leaves behind (on which the luma filter almost never fires).

  * build(): a picture of 8x8 CUs (2Nx2N, tr_idx 0, every cbf 0, zero motion) in P slices with two references whose device pictures both hold
    the crafted picture `pat`; ref_idx0 alternates like a checkerboard, so that every CU edge has Bs 1 (different reference pictures) and the
    reconstruction is `pat`.  A chosen subset of the CUs is PCM (intra, pcm_sample = pat at the coding bit depth): Bs 2 and chroma deblocking
    on known samples.  Lossless CUs, QP per CU, slices, tiles and the per-slice deblocking controls are options.
  * luma_plane() / chroma_plane(): crafted content laid out per edge unit (4 lines x p3 .. q3), varying along x for vertical edges
    (filter stage 1); the picture for horizontal edges (stage 2) is built in the transposed frame and turned.  The families are
    constructed from each unit's own tc and beta, not drawn.
  * classify_luma() / classify_chroma(): a numpy restatement of the unit decisions (TComLoopFilter.cpp:587-650, 759-891), used ONLY to
    assert that a picture holds the cases its test is about.  Expected samples always come from the oracle.
numpy + libhm_amd.abi only."""
import functools

import numpy as np

from libhm_amd import abi

TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24])
BETA_TABLE = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 66, 2)))
CHROMA_SCALE_420 = np.array(list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + list(range(38, 52)))
assert len(TC_TABLE) == 54 and len(BETA_TABLE) == 52 and len(CHROMA_SCALE_420) == 58


def subsampling(chroma_format):
    """(csx, csy) of the chroma planes; 4:0:0 keeps 4:2:0-shaped planes (hmgpu_seq_params)"""
    fmt = 1 if chroma_format == 0 else chroma_format
    return (0 if fmt == 3 else 1), (1 if fmt == 1 else 0)


def _zxy(parts):
    z = np.arange(parts)
    x = np.zeros(parts, dtype=np.int64)
    y = np.zeros(parts, dtype=np.int64)
    for b in range(8):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


class PatternPicture:
    pass


SLICE_DEFAULTS = dict(slice_type=abi.P_SLICE, deblocking_disable=0, lf_across_slices=1, tc_offset_div2=0, beta_offset_div2=0, pps_cb_qp_offset=0,
                      pps_cr_qp_offset=0, swap_refs=False)


def build(width, height, pat, bd=10, bdc=None, chroma_format=1, log2_ctu=6, pcm=None, bypass=None, pcm_loop_filter_disable=0, qp=None,
          slice_starts=(0,), slice_opts=None, tile_idx=None, lf_across_tiles=1, sao_raw=None, sao_offset_shift=(0, 0), ref_handles=(0, 1)):
    """pat: three int16 planes.  pcm / bypass / qp: per 8x8 CU, arrays [height / 8, width / 8] (default: none, none, 32).  slice_starts: first
    CTU (raster address) of each slice; slice_opts: one dict per slice over SLICE_DEFAULTS (slice_type I: every CU of the slice must be PCM;
    swap_refs: the slice lists the two references in the other order); tile_idx: per CTU.  Returns a PatternPicture: .seq, .slices,
    .slice_ranges, .meta, .coeffs (with the PCM samples), .pp, .sao_raw (None: SAO disabled in .pp) and the per-CU grids it was made from."""
    assert width % 8 == 0 and height % 8 == 0
    csx, csy = subsampling(chroma_format)
    bdc = bd if bdc is None else bdc
    ctu, parts = 1 << log2_ctu, 1 << (2 * log2_ctu - 4)
    cw, ch = (width + ctu - 1) // ctu, (height + ctu - 1) // ctu
    n = cw * ch
    gh, gw = height // 8, width // 8
    pcm = np.zeros((gh, gw), dtype=bool) if pcm is None else np.asarray(pcm, dtype=bool)
    bypass = np.zeros((gh, gw), dtype=bool) if bypass is None else np.asarray(bypass, dtype=bool)
    qp = np.full((gh, gw), 32, dtype=np.int64) if qp is None else np.asarray(qp, dtype=np.int64)
    assert pcm.shape == bypass.shape == qp.shape == (gh, gw)
    assert qp.min() >= -6 * (bd - 8) and qp.max() <= 51
    zx, zy = _zxy(parts)
    px = (np.arange(n) % cw)[:, None] * ctu + 4 * zx[None, :]
    py = (np.arange(n) // cw)[:, None] * ctu + 4 * zy[None, :]
    inside = (px < width) & (py < height)
    cx, cy = np.minimum(px // 8, gw - 1), np.minimum(py // 8, gh - 1)

    def per_part(grid, outside):
        return np.where(inside, grid[cy, cx], outside)
    is_pcm = per_part(pcm, False)
    slice_idx = np.zeros(n, dtype=np.uint16)
    starts = list(slice_starts)
    assert starts[0] == 0 and starts == sorted(set(starts)) and starts[-1] < n
    for k, a in enumerate(starts):
        slice_idx[a:] = k
    opts = [dict(SLICE_DEFAULTS, **(o or {})) for o in (slice_opts or [None] * len(starts))]
    assert len(opts) == len(starts)
    tile = np.zeros(n, dtype=np.uint16) if tile_idx is None else np.asarray(tile_idx, dtype=np.uint16)
    slice_of_part = slice_idx[:, None] * np.ones((1, parts), dtype=np.int64)
    for k, o in enumerate(opts):
        if o["slice_type"] == abi.I_SLICE:
            assert is_pcm[(slice_of_part == k) & inside].all(), "an I slice is made of PCM CUs here"
    m = {"depth": np.where(inside, log2_ctu - 3, 0), "part_size": np.where(inside, abi.SIZE_2Nx2N, abi.SIZE_NONE),
         "pred_mode": is_pcm.astype(np.int64), "qp": per_part(qp, 0), "tr_idx": np.zeros((n, parts), dtype=np.int64),
         "cbf_y": np.zeros((n, parts), dtype=np.int64), "cbf_u": np.zeros((n, parts), dtype=np.int64), "cbf_v": np.zeros((n, parts), dtype=np.int64),
         "mv0": np.zeros((n, parts, 2), dtype=np.int64), "mv1": np.zeros((n, parts, 2), dtype=np.int64),
         "ref_idx0": np.where(inside & ~is_pcm, (cx + cy) & 1, -1), "ref_idx1": np.full((n, parts), -1, dtype=np.int64),
         "intra_dir_l": np.ones((n, parts), dtype=np.int64), "intra_dir_c": np.full((n, parts), 36, dtype=np.int64),
         "bypass": per_part(bypass, False).astype(np.int64), "ipcm": is_pcm.astype(np.int64), "slice_idx": slice_idx, "tile_idx": tile}
    # levels: none.  PCM samples: `pat` in the layout of the levels (every CU's block at (16 * z) >> (csx + csy), rows of the block's own width)
    elems = [ctu * ctu, ctu * ctu >> (csx + csy), ctu * ctu >> (csx + csy)]
    pcm_s = []
    for comp in range(3):
        sx, sy = (csx, csy) if comp else (0, 0)
        bw, bh = 8 >> sx, 8 >> sy
        cwc, chc = ctu >> sx, ctu >> sy
        padded = np.zeros((ch * chc, cw * cwc), dtype=np.int16)
        src = np.asarray(pat[comp], dtype=np.int16)
        padded[:src.shape[0], :src.shape[1]] = src
        blocks = padded.reshape(ch, chc, cw, cwc).transpose(0, 2, 1, 3).reshape(n, chc, cwc)
        out = np.zeros((n, elems[comp]), dtype=np.int16)
        for z in range(0, parts, 4):
            x8, y8 = int(zx[z]) // 2, int(zy[z]) // 2
            off = (16 * z) >> ((sx + sy) if comp else 0)
            out[:, off:off + bw * bh] = blocks[:, y8 * bh:(y8 + 1) * bh, x8 * bw:(x8 + 1) * bw].reshape(n, bw * bh)
        pcm_s.append(out)
    p = PatternPicture()
    p.width, p.height, p.bit_depth, p.bit_depth_chroma, p.chroma_format, p.log2_ctu = width, height, bd, bdc, chroma_format, log2_ctu
    p.csx, p.csy, p.num_ctus, p.ctus_w, p.ctus_h = csx, csy, n, cw, ch
    p.seq = abi.make_seq(width, height, bd, bdc, log2_ctu=log2_ctu, max_pictures=8)
    p.seq.chroma_format = chroma_format
    p.seq.pcm_loop_filter_disable = pcm_loop_filter_disable
    p.seq.pcm_bit_depth_luma, p.seq.pcm_bit_depth_chroma = bd, bdc
    p.slices, p.slice_ranges = [], []
    for k, o in enumerate(opts):
        refs = list(ref_handles)[::-1] if o["swap_refs"] else list(ref_handles)
        pocs = [100 + h for h in refs]
        l0 = ([], []) if o["slice_type"] == abi.I_SLICE else (refs, pocs)
        l1 = (refs[:1], pocs[:1]) if o["slice_type"] == abi.B_SLICE else ([], [])
        sl = abi.make_slice(o["slice_type"], (l0[0], l1[0]), (l0[1], l1[1]), pps_cb=o["pps_cb_qp_offset"], pps_cr=o["pps_cr_qp_offset"],
                            cb_qp_offset=o["pps_cb_qp_offset"], cr_qp_offset=o["pps_cr_qp_offset"], deblocking_disable=o["deblocking_disable"],
                            beta_offset_div2=o["beta_offset_div2"], tc_offset_div2=o["tc_offset_div2"], lf_across_slices=o["lf_across_slices"],
                            lf_across_tiles=lf_across_tiles)
        p.slices.append(sl)
        end = starts[k + 1] if k + 1 < len(starts) else n
        p.slice_ranges.append((starts[k], end - starts[k]))
    p.slice = p.slices[0]
    p.slice_opts = opts
    p.meta_np = m
    p.meta = abi.MetaHolder(m)
    p.coeffs = abi.CoeffHolder(*[np.zeros((n, e), dtype=np.int16) for e in elems], pcm=pcm_s)
    p.pp = abi.make_pic_params(sao_enabled=0 if sao_raw is None else 1, lf_across_tiles=lf_across_tiles, sao_offset_shift=sao_offset_shift)
    p.sao_raw = np.zeros((n, 3, 35), dtype=np.int32) if sao_raw is None else np.asarray(sao_raw, dtype=np.int32)
    p.pat = [np.ascontiguousarray(a, dtype=np.int16) for a in pat]
    p.pcm, p.bypass, p.qp = pcm, bypass, qp
    p.pcm_loop_filter_disable = pcm_loop_filter_disable
    # per CU: the slice and the tile of its CTU
    shift = log2_ctu - 3
    ctu_of_cu = (np.arange(gh)[:, None] >> shift) * cw + (np.arange(gw)[None, :] >> shift)
    p.cu_slice, p.cu_tile = slice_idx[ctu_of_cu].astype(np.int64), tile[ctu_of_cu].astype(np.int64)
    p.cu_ref = np.add.outer(np.arange(gh), np.arange(gw)) & 1              # ref_idx0 of the inter CUs
    return p


# ------------------------------------------------------------------------------------------------ the parameters of every edge unit
class EdgeUnits:
    """what decides the filtering of the edge units of one direction, in the frame in which the edges are vertical (the picture itself for
    direction "ver", its transpose for "hor"): arrays [2 * CU rows, CU columns - 1], entry (u, e - 1) = the four lines u of the edge at 8 * e"""


def _t(a, direction):
    return a if direction == "ver" else a.T


def edge_units(bd, bdc, chroma_format, qp, pcm, bypass, cu_slice, slice_opts, pcm_loop_filter_disable, direction, bs=None, handle=None):
    """bs: Bs per unit where the caller knows better (the oracle's, which knows about borders and disabled slices); default 2 beside a PCM CU,
    else 1 where the two CUs predict from different pictures (handle: per CU; default: the checkerboard of build(), which differs across
    every edge) and 0 where from the same (zero motion everywhere)"""
    qp, pcm, bypass, cu_slice = (_t(np.asarray(a), direction) for a in (qp, pcm, bypass, cu_slice))
    if handle is None:
        handle = np.add.outer(np.arange(qp.shape[0]), np.arange(qp.shape[1])) & 1
    else:
        handle = _t(np.asarray(handle), direction)
    two = lambda a: np.repeat(a, 2, axis=0)
    opt = lambda key: np.array([o[key] for o in slice_opts])[cu_slice[:, 1:]]
    u = EdgeUnits()
    u.direction = direction
    u.qp = two((qp[:, :-1] + qp[:, 1:] + 1) >> 1)
    u.bs = two(np.where(pcm[:, :-1] | pcm[:, 1:], 2, (handle[:, :-1] != handle[:, 1:]).astype(np.int64))) if bs is None else np.asarray(bs)
    exempt = bypass | (pcm & bool(pcm_loop_filter_disable))
    u.p_exempt, u.q_exempt = two(exempt[:, :-1]), two(exempt[:, 1:])
    tc_off, beta_off = two(opt("tc_offset_div2")), two(opt("beta_offset_div2"))
    u.tc = TC_TABLE[np.clip(u.qp + 2 * (u.bs - 1) + 2 * tc_off, 0, 53)] << (bd - 8)
    u.beta = BETA_TABLE[np.clip(u.qp + 2 * beta_off, 0, 51)] << (bd - 8)
    # chroma (Bs 2 only; xEdgeFilterChroma :759-775)
    fmt = 1 if chroma_format == 0 else chroma_format
    u.tc_c = []
    for key in ("pps_cb_qp_offset", "pps_cr_qp_offset"):
        q = u.qp + two(opt(key))
        mapped = CHROMA_SCALE_420[np.clip(q, 0, 57)] if fmt == 1 else np.minimum(q, 51)
        q = np.where(q >= 58, q - 6 if fmt == 1 else np.minimum(q, 51), np.where(q >= 0, mapped, q))
        u.tc_c.append(TC_TABLE[np.clip(q + 2 + 2 * tc_off, 0, 53)] << (bdc - 8))
    return u


def units_of(p, direction, bs=None):
    return edge_units(p.bit_depth, p.bit_depth_chroma, p.chroma_format, p.qp, p.pcm, p.bypass, p.cu_slice, p.slice_opts, p.pcm_loop_filter_disable,
                      direction, bs)


def bs_units(p, bs_ver, bs_hor, direction):
    """the oracle's boundary strengths ([num_ctus, parts], z order) as the Bs of the edge units of `direction` (EdgeUnits frame)"""
    parts = 1 << (2 * p.log2_ctu - 4)
    zx, zy = _zxy(parts)
    pw = 1 << (p.log2_ctu - 2)
    grid = np.zeros((p.ctus_h * pw, p.ctus_w * pw), dtype=np.int64)
    src = bs_ver if direction == "ver" else bs_hor
    a = np.arange(p.num_ctus)
    grid[(a // p.ctus_w)[:, None] * pw + zy[None, :], (a % p.ctus_w)[:, None] * pw + zx[None, :]] = src
    grid = grid[:p.height // 4, :p.width // 4]
    return grid[:, 2::2] if direction == "ver" else grid[2::2, :].T


# ------------------------------------------------------------------------------------------------ crafted content
N_LUMA_RECIPES = 13


def _luma_recipe(r, k, tc, beta, bd):
    """lines of one edge unit relative to an anchor: (int array [4, 8] of p3 p2 p1 p0 q0 q1 q2 q3, anchor: "any" / "low" (the smallest value is
    sample value 0) / "high" (the largest is the maximum)), or None where tc / beta leave no room for the family.  k: a running number that
    varies what is free"""
    side = (beta + (beta >> 1)) >> 3
    z = [0, 0, 0, 0]
    anchor = "any"
    if tc == 0:
        return None
    if r == 0:                                   # weak, delta clipped at tc
        L = [z + [4 * tc] * 4] * 4
    elif r == 1:                                 # weak, delta within tc: p3 alone keeps the unit from being strong
        L = [[-max(beta >> 3, 1), 0, 0, 0] + [tc] * 4] * 4
    elif r in (2, 3, 4):                         # second derivative on one side / both: dEq only (2: P curved), dEp only (3: Q curved), neither (4)
        c = (side + 3) // 4
        if c == 0 or (4 if r < 4 else 8) * c >= beta:
            return None
        s = 4 * tc
        pside = [0, 0, c, 0] if r in (2, 4) else z
        qside = [s, s + c, s, s] if r in (3, 4) else [s] * 4
        L = [pside + qside] * 4
    elif r == 5:                                 # lines 0 / 3 inside |delta| < 10 tc, line 1 or 2 (or both) outside: flat sides, delta = (6 s + 8) >> 4
        a, b = z + [4 * tc] * 4, z + [27 * tc] * 4
        L = [a, b if k % 3 != 1 else a, b if k % 3 != 0 else a, a]
    elif r == 6:                                 # delta against the step: p0 + delta falls below 0 (negated: q0 - delta above the maximum)
        x = max(beta >> 3, 3) + (k >> 2) % 3
        if (3 * x + 8) >> 4 >= 10 * tc:
            return None
        L, anchor = [z + [0, x, 2 * x, 3 * x]] * 4, "low"
    elif r == 7:                                 # 12 bits: 9 (q0 - p0) - 3 (q1 - p1) + 8 above 32767 (the true delta 2060 or less: filtered iff tc >= 207)
        if bd != 12 or tc < 207:
            return None
        i, j = (k >> 2) % 8, (k >> 5) % 4
        L, anchor = [[2800 + j, 2800 + j, 1400 + j, j, 4095 - i, 2700 - i, 1305 - i, 1305 - i]] * 4, "low"
    elif r == 8:                                 # strong, every change within 2 tc
        s = min(2 * tc, ((5 * tc + 1) >> 1) - 1)
        if s < 1 or (beta >> 3) < 1:
            return None
        L = [z + [s] * 4] * 4
    elif r in (9, 12):                           # strong, the 2 tc limit cuts p0: as much slope and second derivative on P as the decisions allow
        p2 = (beta >> 3) - 1
        d = ((beta >> 2) - 1) // 2
        s = ((5 * tc + 1) >> 1) - 1
        if p2 < 1 or d < 0 or s < 1:
            return None
        L = [[p2, p2, (p2 + d) // 2, 0] + [s] * 4] * 4
    elif r == 10:                                # d >= beta
        L = [[0, 0, beta + 1, 0] + [4 * tc] * 4] * 4
    else:                                        # weak with small second derivatives on both sides: p1 / q1 corrections that stay inside tc / 2
        L = [[3, 1, 0, 0, 2 * tc + 3, 2 * tc + 3, 2 * tc + 4, 2 * tc + 6]] * 4
        if 6 >= beta:
            return None
    L = np.array(L, dtype=np.int64)
    if k & 1:
        L = -L
        anchor = {"low": "high", "high": "low"}.get(anchor, anchor)
    if k & 2:
        L = L[:, ::-1]
    return L, anchor


def _place(L, anchor, k, mx):
    lo, hi = int(L.min()), int(L.max())
    if hi - lo > mx:
        return None
    if anchor == "any":
        anchor = ("low", "high", "mid")[(k >> 2) % 3]
    shift = -lo if anchor == "low" else (mx - hi if anchor == "high" else (mx - hi - lo) // 2)
    return L + shift


def luma_plane(height, width, bd, units):
    """a luma plane (frame of `units`: edges vertical) whose edge units run through the families of _luma_recipe, each built from the unit's
    own tc and beta; a unit whose tc is 0 holds a plain step.  The first and last four columns belong to no edge and stay mid-grey."""
    mx = (1 << bd) - 1
    plane = np.full((height, width), 1 << (bd - 1), dtype=np.int64)
    nu, ne = units.tc.shape
    count = 0
    for u in range(nu):
        for e in range(ne):
            tc, beta = int(units.tc[u, e]), int(units.beta[u, e])
            cell = None
            for attempt in range(N_LUMA_RECIPES):
                got = _luma_recipe((count + attempt) % N_LUMA_RECIPES, count // N_LUMA_RECIPES, tc, beta, bd)
                if got is not None:
                    cell = _place(got[0], got[1], count // N_LUMA_RECIPES, mx)
                if cell is not None:
                    break
            if cell is None:                      # tc == 0 (or no room at all): a step that any filtering would show
                s = 6 << (bd - 8)
                cell = _place(np.array([[0, 0, 0, 0, s, s, s, s]] * 4) * (1 if count & 1 else -1), "any", count, mx)
            plane[4 * u:4 * u + 4, 8 * e + 4:8 * e + 12] = cell
            count += 1
    return plane.astype(np.int16)


def chroma_plane(height, width, bdc, units, comp, cs_across, cs_along):
    """a chroma plane (height x width chroma samples, frame of `units`) for the edges on the plane's 8-sample grid: per unit (the 4 >> cs_along
    lines of a 4x4 luma partition) p1 p0 q0 q1 with delta inside tc, clipped at tc, and p0 + delta / q0 - delta beyond 0 / the maximum"""
    mx = (1 << bdc) - 1
    plane = np.full((height, width), 1 << (bdc - 1), dtype=np.int64)
    n = 4 >> cs_along
    tcs = units.tc_c[comp - 1]
    count = 0
    for u in range(height // n):
        for k in range(1, (width - 4) // 8 + 1):
            e = k << cs_across                      # the luma edge this chroma edge belongs to
            if e - 1 >= tcs.shape[1] or u >= tcs.shape[0]:
                continue
            tc = max(int(tcs[u, e - 1]), 1)
            r, v = count % 4, count // 4
            if r == 0:
                L, anchor = [0, 0, 0, 0, tc, tc, tc, tc], "any"
            elif r == 1:
                L, anchor = [0, 0, 0, 0, 4 * tc, 4 * tc, 4 * tc, 4 * tc], "any"
            elif r == 2:
                L, anchor = [0, 0, 0, 0, 0, 5 + 8 * (v % 3) * tc, 0, 0], "low"
            else:
                L, anchor = [0, 0, 5 + 8 * (v % 3) * tc, 0, 0, 0, 0, 0], "low"
            L = np.array([L] * n, dtype=np.int64)
            if v & 1:
                L = -L
                anchor = {"low": "high"}.get(anchor, anchor)
            cell = _place(L, anchor, v, mx)
            if cell is None:
                cell = _place(np.array([[0, 0, 0, 0, 1, 1, 1, 1]] * n), "any", v, mx)
            plane[n * u:n * u + n, 8 * k - 4:8 * k + 4] = cell
            count += 1
    return plane.astype(np.int16)


def crafted_planes(width, height, bd, bdc, chroma_format, units):
    """the three planes of the picture for units.direction"""
    csx, csy = subsampling(chroma_format)
    if units.direction == "ver":
        return [luma_plane(height, width, bd, units)] + [chroma_plane(height >> csy, width >> csx, bdc, units, c, csx, csy) for c in (1, 2)]
    return [luma_plane(width, height, bd, units).T.copy()] + [chroma_plane(width >> csx, height >> csy, bdc, units, c, csy, csx).T.copy() for c in (1, 2)]


# ------------------------------------------------------------------------------------------------ what a picture holds (coverage only)
def classify_luma(plane, bd, units):
    """counts of edge units per class (dict), from the unfiltered luma plane (units' frame) and the units' parameters"""
    h, w = plane.shape
    mx = (1 << bd) - 1
    U = plane[:, 4:w - 4].astype(np.int64).reshape(h // 4, 4, w // 8 - 1, 8).transpose(0, 2, 1, 3)        # [unit row, edge, line, sample]
    m = [U[..., i] for i in range(8)]                                                                      # each [unit row, edge, line]
    tc, beta, bs = units.tc, units.beta, units.bs
    dp, dq = np.abs(m[1] - 2 * m[2] + m[3]), np.abs(m[4] - 2 * m[5] + m[6])
    d0, d3 = dp[..., 0] + dq[..., 0], dp[..., 3] + dq[..., 3]
    d = d0 + d3
    side = (beta + (beta >> 1)) >> 3
    dep, deq = (dp[..., 0] + dp[..., 3]) < side, (dq[..., 0] + dq[..., 3]) < side

    def strong_line(i, dd):
        return ((np.abs(m[0][..., i] - m[3][..., i]) + np.abs(m[7][..., i] - m[4][..., i]) < (beta >> 3)) & (2 * dd < (beta >> 2)) &
                (np.abs(m[3][..., i] - m[4][..., i]) < ((tc * 5 + 1) >> 1)))
    sw = strong_line(0, d0) & strong_line(3, d3)
    act = (bs > 0) & (tc > 0) & (d < beta)
    t3 = tc[..., None]
    # strong filter before its +-2 tc limit
    n = {3: (m[1] + 2 * m[2] + 2 * m[3] + 2 * m[4] + m[5] + 4) >> 3, 4: (m[2] + 2 * m[3] + 2 * m[4] + 2 * m[5] + m[6] + 4) >> 3,
         2: (m[1] + m[2] + m[3] + m[4] + 2) >> 2, 5: (m[3] + m[4] + m[5] + m[6] + 2) >> 2,
         1: (2 * m[0] + 3 * m[1] + m[2] + m[3] + m[4] + 4) >> 3, 6: (m[3] + m[4] + m[5] + 3 * m[6] + 2 * m[7] + 4) >> 3}
    limited = np.zeros(sw.shape, dtype=bool)
    for i, v in n.items():
        limited |= (np.abs(v - m[i]) > 2 * t3).any(axis=-1)
    wide = 9 * (m[4] - m[3]) - 3 * (m[5] - m[2]) + 8
    delta = wide >> 4
    on = np.abs(delta) < 10 * t3
    dc = np.clip(delta, -t3, t3)
    tc2 = t3 >> 1
    d1 = np.clip((((m[1] + m[3] + 1) >> 1) - m[2] + dc) >> 1, -tc2, tc2)
    d2 = np.clip((((m[6] + m[4] + 1) >> 1) - m[5] - dc) >> 1, -tc2, tc2)
    res = [m[3] + dc, m[4] - dc, np.where(dep[..., None], m[2] + d1, m[2]), np.where(deq[..., None], m[5] + d2, m[5])]
    weak = act & ~sw
    some = weak & on.any(axis=-1)
    changes = (act & sw) | some
    pe, qe = units.p_exempt, units.q_exempt
    out = {"tc = 0": (bs > 0) & (tc == 0), "d >= beta": (bs > 0) & (tc > 0) & (d >= beta),
           "strong, 2tc limit active": act & sw & limited, "strong, 2tc limit inactive": act & sw & ~limited,
           "weak, dEp and dEq": some & dep & deq, "weak, dEp only": some & dep & ~deq, "weak, dEq only": some & ~dep & deq, "weak, neither": some & ~dep & ~deq,
           "weak, lines 0 and 3 inside 10tc, line 1 or 2 outside": weak & on[..., 0] & on[..., 3] & ~(on[..., 1] & on[..., 2]),
           "delta clipped at +tc": weak & (on & (delta > t3)).any(axis=-1), "delta clipped at -tc": weak & (on & (delta < -t3)).any(axis=-1),
           "result clipped at 0": weak & np.any([(on & (r < 0)).any(axis=-1) for r in res], axis=0),
           "result clipped at max": weak & np.any([(on & (r > mx)).any(axis=-1) for r in res], axis=0),
           "delta beyond 16 bits before the shift": weak & (on & (np.abs(wide) > 32767)).any(axis=-1),
           "P side exempt only": changes & pe & ~qe, "Q side exempt only": changes & ~pe & qe, "both sides exempt": changes & pe & qe,
           "Bs 1": bs == 1, "Bs 2": bs == 2}
    return {k: int(v.sum()) for k, v in out.items()}


def classify_chroma(plane, bdc, units, comp, cs_across, cs_along):
    """the same for one chroma plane: units with Bs 2 on the plane's 8-sample grid"""
    h, w = plane.shape
    mx = (1 << bdc) - 1
    n = 4 >> cs_along
    out = {"chroma: delta clipped": 0, "chroma: delta not clipped": 0, "chroma: result clipped at 0": 0, "chroma: result clipped at max": 0,
           "chroma: P side exempt only": 0, "chroma: Q side exempt only": 0}
    ks = np.arange(1, (w - 4) // 8 + 1)
    ks = ks[(ks << cs_across) - 1 < units.bs.shape[1]]
    e = (ks << cs_across) - 1
    nu = min(h // n, units.bs.shape[0])
    cells = np.stack([plane[:nu * n, 8 * k - 2:8 * k + 2].astype(np.int64).reshape(nu, n, 4) for k in ks], axis=1)       # [unit, edge, line, p1 p0 q0 q1]
    tc = units.tc_c[comp - 1][:nu][:, e][..., None]
    bs2 = (units.bs[:nu][:, e] == 2)
    raw = (((cells[..., 2] - cells[..., 1]) << 2) + cells[..., 0] - cells[..., 3] + 4) >> 3
    dc = np.clip(raw, -tc, tc)
    pe, qe = units.p_exempt[:nu][:, e], units.q_exempt[:nu][:, e]
    lo = ((cells[..., 1] + dc < 0) & ~pe[..., None]) | ((cells[..., 2] - dc < 0) & ~qe[..., None])
    hi = ((cells[..., 1] + dc > mx) & ~pe[..., None]) | ((cells[..., 2] - dc > mx) & ~qe[..., None])
    live = bs2 & (tc[..., 0] > 0)
    out["chroma: delta clipped"] = int((live & (np.abs(raw) > tc).any(axis=-1)).sum())
    out["chroma: delta not clipped"] = int((live & ((np.abs(raw) <= tc) & (raw != 0)).any(axis=-1)).sum())
    out["chroma: result clipped at 0"] = int((live & lo.any(axis=-1)).sum())
    out["chroma: result clipped at max"] = int((live & hi.any(axis=-1)).sum())
    moved = live & (dc != 0).any(axis=-1)
    out["chroma: P side exempt only"] = int((moved & pe & ~qe).sum())
    out["chroma: Q side exempt only"] = int((moved & ~pe & qe).sum())
    return out


# ------------------------------------------------------------------------------------------------ the pictures of the arithmetic tests
def qp_cycle(bd):
    """QPs for the CUs of a picture: the whole legal range -6 (bd - 8) .. 51 once, then the part in which the filters act (tc > 0 at Bs 1 from
    QP 18, at the most negative tc offset from 30) several times over, so that inert units stay a small share"""
    return np.array(list(range(-6 * (bd - 8), 52)) + 5 * list(range(24, 52)) + 3 * list(range(36, 52)))


def arith_grids(width, height, bd, log2_ctu):
    """per-CU inputs of the arithmetic pictures: QP cycling along the rows; every third CU of a diagonal PCM (Bs 2; both parities of x and y,
    so that their edges fall on the chroma grid of every format); one CU in eleven lossless, in every fourth row two side by side;
    three slices (the second starting mid-row) with the tc / beta offsets at 0 / 0, -6 / +6 and +6 / -6 and different chroma QP offsets"""
    gh, gw = height // 8, width // 8
    y, x = np.mgrid[0:gh, 0:gw]
    cyc = qp_cycle(bd)
    qp = cyc[(y * 37 + x) % len(cyc)]
    pcm = (x + 2 * y) % 3 == 0
    bypass = ((5 * x + 3 * y) % 11 == 0) | (((5 * (x - 1) + 3 * y) % 11 == 0) & (y % 4 == 0)) | (((5 * x + 3 * (y - 1)) % 11 == 0) & (x % 4 == 0))
    ctu = 1 << log2_ctu
    cw, ch = (width + ctu - 1) // ctu, (height + ctu - 1) // ctu
    starts = [0, (ch // 3) * cw + cw // 2, (2 * ch // 3) * cw]
    opts = [dict(pps_cb_qp_offset=0, pps_cr_qp_offset=3), dict(tc_offset_div2=-6, beta_offset_div2=6, pps_cb_qp_offset=-12, pps_cr_qp_offset=12),
            dict(tc_offset_div2=6, beta_offset_div2=-6, pps_cb_qp_offset=7, pps_cr_qp_offset=-5)]
    return qp, pcm, bypass, starts, opts


@functools.lru_cache(maxsize=None)
def arith_picture(width, height, bd, bdc, chroma_format, log2_ctu, direction, sao_seed=None):
    """the pattern picture of the deblocking-arithmetic tests for one direction ("ver": content varies along x, for filter stage 1; "hor": the
    same construction in the transposed frame, for stage 2).  Cached: the CPU and GPU tests of one shape share it; nobody may change it."""
    qp, pcm, bypass, starts, opts = arith_grids(width, height, bd, log2_ctu)
    shell = build(width, height, [np.zeros((8, 8), dtype=np.int16)] * 3, bd, bdc, chroma_format, log2_ctu, pcm, bypass, 0, qp, starts, opts)     # (for the per-CU slice map)
    units = edge_units(bd, bdc, chroma_format, qp, pcm, bypass, shell.cu_slice, shell.slice_opts, 0, direction)
    pat = crafted_planes(width, height, bd, bdc, chroma_format, units)
    sao = None if sao_seed is None else random_sao(shell.num_ctus, sao_seed, chroma_format, bd, bdc)
    return build(width, height, pat, bd, bdc, chroma_format, log2_ctu, pcm, bypass, 0, qp, starts, opts, sao_raw=sao)


def random_sao(n, seed, chroma_format, bd, bdc):
    """seeded raw SAO parameters, every type on every component, offsets up to the largest HM codes for the depth (7 << (min(bd, 10) - 5))"""
    rng = np.random.RandomState(seed)
    raw = np.zeros((n, 3, 35), dtype=np.int32)
    for comp in range(3 if chroma_format else 1):
        maxo = (1 << (min(bdc if comp else bd, 10) - 5)) - 1
        kind = rng.randint(0, 6, size=n)                                  # 0 off, 1 BO, 2.. EO classes
        raw[:, comp, 0] = np.where(kind == 0, abi.SAO_OFF, abi.SAO_NEW)
        raw[:, comp, 1] = np.where(kind == 1, abi.SAO_BO, np.maximum(kind - 2, 0))
        band = rng.randint(0, 32, size=n)
        raw[:, comp, 2] = np.where(kind == 1, band, 0)
        offs = rng.randint(-maxo, maxo + 1, size=(n, 4))
        for a in range(n):
            if kind[a] == 1:
                for i in range(4):
                    raw[a, comp, 3 + (band[a] + i) % 32] = offs[a, i]
            elif kind[a] >= 2:
                raw[a, comp, 3:8] = [abs(offs[a, 0]), abs(offs[a, 1]), 0, -abs(offs[a, 2]), -abs(offs[a, 3])]
    return raw


def near_edge_changed(before, after, direction):
    """share of the luma samples within 4 of an 8x8 edge of `direction` (all but the outermost four columns / rows) that differ"""
    a, b = (before, after) if direction == "ver" else (before.T, after.T)
    return float((a[:, 4:-4] != b[:, 4:-4]).mean())


# ------------------------------------------------------------------------------------------------ variants of the arithmetic picture
def exempt_grids(width, height):
    """lossless, PCM and ordinary CUs interleaved without a period along either axis (kind 0 PCM, 1 lossless, 2 ordinary): with
    pcm_loop_filter_disable both of the first two are exempt from deblocking and SAO, and exempt P / exempt Q / both / neither occur on the
    edges of both directions, beside PCM CUs (Bs 2: chroma) and away from them"""
    y, x = np.mgrid[0:height // 8, 0:width // 8]
    kind = (x * 7 + y * 13 + (x * y) % 5 + (x // 3) * (y // 2)) % 3
    return kind == 0, kind == 1


@functools.lru_cache(maxsize=None)
def variant_picture(width, height, bd, bdc, chroma_format, log2_ctu, direction, variant, ref_handles=(0, 1), sao_seed=7):
    """the arithmetic picture's content and QPs with other CUs: variant "exempt" (exempt_grids, pcm_loop_filter_disable = 1) or "plain" (no
    PCM, no lossless CU; the same sequence parameters, so that both fit one context).  One slice, SAO on.  Cached, read-only."""
    qp = arith_grids(width, height, bd, log2_ctu)[0]
    pcm, bypass = exempt_grids(width, height) if variant == "exempt" else (np.zeros_like(qp, dtype=bool), np.zeros_like(qp, dtype=bool))
    opts = [dict(pps_cb_qp_offset=2, pps_cr_qp_offset=-3)]
    units = edge_units(bd, bdc, chroma_format, qp, pcm, bypass, np.zeros_like(qp), [dict(SLICE_DEFAULTS, **opts[0])], 1, direction)
    pat = crafted_planes(width, height, bd, bdc, chroma_format, units)
    n = (-(-width >> log2_ctu)) * (-(-height >> log2_ctu))
    return build(width, height, pat, bd, bdc, chroma_format, log2_ctu, pcm, bypass, 1, qp, (0,), opts, sao_raw=random_sao(n, sao_seed, chroma_format, bd, bdc),
                 ref_handles=ref_handles)


# ------------------------------------------------------------------------------------------------ SAO arithmetic
def sao_content(height, width, bd, salt):
    """a plane for SAO: 8x8 cells that run through the 32 bands (any 32 consecutive cells of a row hold them all), inside a cell a three-level
    texture one apart -- every pair of signs towards the two neighbours of every edge class --, sample value 0 in cells of band 0 and the maximum
    in cells of band 31"""
    y, x = np.mgrid[0:height, 0:width]
    bw = 1 << (bd - 5)
    band = (x // 8 + 5 * (y // 8) + salt) % 32
    tex = ((x * x * x + 5 * y * y + x * y + salt) % 11) % 3
    jitter = np.where(band % 2 == 0, 0, bw - 3)
    return (band * bw + jitter + tex).astype(np.int16)


def sao_layout(cw, ch):
    """CTU geometry of the SAO pictures: a 2 x 2 tile grid split after CTU column cw // 2 and after the first CTU row; three slices, the second
    starting mid-row in CTU row 1, the third at CTU 2 of the last row, lf_across_slices 1 / 0 / 1 (at the border of slices 0 and 1 the earlier
    slice says yes and the later no, at the border of 1 and 2 the other way round).  Returns (tile index per CTU, slice starts, merges: CTU
    address -> 0 left / 1 above, CTUs forced OFF)"""
    split = cw // 2 + 1
    a = np.arange(cw * ch)
    tile = ((a % cw) >= split).astype(np.int64) + 2 * ((a // cw) >= 1)
    starts = [0, cw + cw // 2, (ch - 1) * cw + 2]
    merges = {}
    for x in range(1, split):                      # a whole row of the left tile merges left from its first CTU
        merges[2 * cw + x] = 0
    for y in range(2, 5):                          # the first column of the right tile: rows 2 .. 4 merge above, from row 1
        merges[y * cw + split] = 1
    for x in range(split + 1, cw):                 # ... and row 4 of the right tile merges left from the end of that chain
        merges[4 * cw + x] = 0
    off = [3 * cw + 1]
    merges[3 * cw + 2] = 0                         # a merge that resolves to OFF
    return tile, starts, merges, off


def sao_entries(variant, maxo):
    """the NEW parameter sets a variant runs through, as (type, band start, offset[32]): "bo": every band start 0 .. 31 (29 .. 31 wrap round to
    band 0) with offsets at +- the largest coded value, then OFF; "eo0" .. "eo3": the four edge classes in turn, starting at the variant's
    number, offsets of HM's legal signs at the largest magnitudes"""
    out = []
    if variant == "bo":
        for s in range(32):
            o = np.zeros(32, dtype=np.int32)
            vals = [maxo, -maxo, maxo if s % 2 else -maxo, -maxo + s % 3]
            for i in range(4):
                o[(s + i) % 32] = vals[i]
            out.append((abi.SAO_BO, s, o))
        out.append(None)
    else:
        for k in range(8):
            o = np.zeros(32, dtype=np.int32)
            v = k // 4
            o[:5] = [maxo, maxo - v, 0, -(maxo - v), -maxo]
            out.append(((k + int(variant[2])) % 4, 0, o))
    return out


@functools.lru_cache(maxsize=None)
def sao_picture(width, height, bd, bdc, chroma_format, log2_ctu, variant, bad_merge=None):
    """the pattern picture of the SAO tests: deblocking disabled in every slice, so that SAO reads the crafted picture.  Components run through
    sao_entries() from different starting points (different types per CTU); merges as in sao_layout().  12 / 10 bits: sao_offset_shift 2 luma / 0
    chroma (the resolved luma offsets reach +-124).  bad_merge: "slice" / "tile_left" / "tile_above" adds one merge across such a border, which
    no decoder may accept.  Cached, read-only."""
    ctu = 1 << log2_ctu
    cw, ch = -(-width // ctu), -(-height // ctu)
    n = cw * ch
    csx, csy = subsampling(chroma_format)
    pat = [sao_content(height, width, bd, 0), sao_content(height >> csy, width >> csx, bdc, 11), sao_content(height >> csy, width >> csx, bdc, 23)]
    tile, starts, merges, off = sao_layout(cw, ch)
    merges = dict(merges)
    if bad_merge == "slice":
        merges[starts[1]] = 0                      # the first CTU of slice 1 from the last of slice 0
    elif bad_merge == "tile_left":
        merges[2 * cw + cw // 2 + 1] = 0           # the first CTU of the right tile from the left tile (same slice)
    elif bad_merge == "tile_above":
        merges[cw + 2] = 1                         # CTU row 1 from row 0: the other tile row, the same slice
    raw = np.zeros((n, 3, 35), dtype=np.int32)
    shift = (2, 0) if (bd, bdc) == (12, 10) else (0, 0)
    for comp in range(3 if chroma_format else 1):
        entries = sao_entries(variant, (1 << (min(bdc if comp else bd, 10) - 5)) - 1)
        i = (0, 11, 23)[comp] if variant == "bo" else comp
        for a in range(n):
            if a in merges:
                raw[a, comp, 0], raw[a, comp, 1] = abi.SAO_MERGE, merges[a]
                continue
            e = None if a in off else entries[i % len(entries)]
            i += a not in off
            if e is None:
                raw[a, comp, 0] = abi.SAO_OFF
            else:
                raw[a, comp, 0], raw[a, comp, 1], raw[a, comp, 2] = abi.SAO_NEW, e[0], e[1]
                raw[a, comp, 3:] = e[2]
    opts = [dict(deblocking_disable=1, lf_across_slices=f) for f in (1, 0, 1)]
    p = build(width, height, pat, bd, bdc, chroma_format, log2_ctu, None, None, 0, None, starts, opts, tile_idx=tile, lf_across_tiles=0, sao_raw=raw,
              sao_offset_shift=shift)
    p.merges, p.sao_off = merges, off
    return p


def sao_coverage(p, rec):
    """what an SAO picture holds, from its raw parameters, the reconstructed ones (`rec`: the oracle's, [num_ctus, 3, 35]) and the content: a dict"""
    ctu = 1 << p.log2_ctu
    out = {"band starts": [], "bands under BO": [], "sign pairs": [], "min": [], "max": []}
    for comp in range(3 if p.chroma_format else 1):
        sx, sy = (p.csx, p.csy) if comp else (0, 0)
        bd = p.bit_depth_chroma if comp else p.bit_depth
        plane = p.pat[comp].astype(np.int64)
        starts, bands = set(), set()
        pairs = {k: set() for k in range(4)}
        for a in range(p.num_ctus):
            mode, typ, aux = (int(v) for v in rec[a, comp, :3])
            if mode == abi.SAO_OFF:
                continue
            y0, x0 = (a // p.ctus_w) * (ctu >> sy), (a % p.ctus_w) * (ctu >> sx)
            blk = plane[y0:y0 + (ctu >> sy), x0:x0 + (ctu >> sx)]
            if typ == abi.SAO_BO:
                starts.add(aux)
                bands |= set(np.unique(blk >> (bd - 5)))
            else:
                dy, dx = ((0, 1), (1, 0), (1, 1), (1, -1))[typ]
                c = blk[1:-1, 1:-1]
                na = blk[1 - dy:blk.shape[0] - 1 - dy, 1 - dx:blk.shape[1] - 1 - dx]
                nb = blk[1 + dy:blk.shape[0] - 1 + dy, 1 + dx:blk.shape[1] - 1 + dx]
                pairs[typ] |= set(zip(np.sign(c - na).ravel().tolist(), np.sign(c - nb).ravel().tolist()))
        out["band starts"].append(starts)
        out["bands under BO"].append(bands)
        out["sign pairs"].append(pairs)
        out["min"].append(int(plane.min()))
        out["max"].append(int(plane.max()))
    return out


# ------------------------------------------------------------------------------------------------ controls on filter-active content
def controls_layout(cw, ch):
    """3 x 2 tiles (the lower row of tiles two CTUs high, its border inside slice 3); five slices that start mid-row: P, I (all PCM), B with the
    two references listed the other way round and deblocking disabled, P (references the same way), B; lf_across_slices alternates 1 0 1 0 1, so that the later slice forbids filtering across the borders 0|1 and 2|3 and
    allows it across 1|2 and 3|4; tc / beta and chroma QP offsets towards the ends of their ranges"""
    a = np.arange(cw * ch)
    tx = ((a % cw) >= cw // 3).astype(np.int64) + ((a % cw) >= 2 * cw // 3)
    tile = tx + 3 * ((a // cw) >= ch - 2)
    starts = [0, cw + 2, 2 * cw + cw // 2, 3 * cw + 1, (ch - 2) * cw + cw - 2]
    opts = [dict(slice_type=abi.P_SLICE, lf_across_slices=1, tc_offset_div2=2, beta_offset_div2=-1, pps_cb_qp_offset=5, pps_cr_qp_offset=-7),
            dict(slice_type=abi.I_SLICE, lf_across_slices=0, tc_offset_div2=-3, beta_offset_div2=6, pps_cb_qp_offset=-12, pps_cr_qp_offset=12),
            dict(slice_type=abi.B_SLICE, lf_across_slices=1, tc_offset_div2=6, beta_offset_div2=3, pps_cb_qp_offset=12, pps_cr_qp_offset=-12, swap_refs=True, deblocking_disable=1),
            dict(slice_type=abi.P_SLICE, lf_across_slices=0, tc_offset_div2=-6, beta_offset_div2=-6, pps_cb_qp_offset=1, swap_refs=True),
            dict(slice_type=abi.B_SLICE, lf_across_slices=1, tc_offset_div2=0, beta_offset_div2=5, pps_cb_qp_offset=-4, pps_cr_qp_offset=9)]
    return tile, starts, opts


@functools.lru_cache(maxsize=None)
def controls_picture(width, height, bd, bdc, chroma_format, log2_ctu, direction, lf_across_tiles, allow=False):
    """every control of build() in one picture on the crafted content of `direction`: controls_layout(), QP per CU over the whole range,
    lossless and PCM CUs, SAO.  allow: the same picture with every control set to "filter" (all slices deblocked and filtered across, tiles
    too) -- what the borders would look like if a decoder ignored the controls.  Cached, read-only."""
    ctu = 1 << log2_ctu
    cw, ch = -(-width // ctu), -(-height // ctu)
    tile, starts, opts = controls_layout(cw, ch)
    qp, pcm, bypass = arith_grids(width, height, bd, log2_ctu)[:3]
    shell = build(width, height, [np.zeros((8, 8), dtype=np.int16)] * 3, bd, bdc, chroma_format, log2_ctu, None, None, 0, qp, starts)
    pcm = pcm | (shell.cu_slice == 1)
    if allow:
        opts = [dict(o, lf_across_slices=1, deblocking_disable=0) for o in opts]
        lf_across_tiles = 1
    full = [dict(SLICE_DEFAULTS, **o) for o in opts]
    handle = np.where(np.array([o["swap_refs"] for o in full])[shell.cu_slice], 1 - shell.cu_ref, shell.cu_ref)
    units = edge_units(bd, bdc, chroma_format, qp, pcm, bypass, shell.cu_slice, full, 0, direction, handle=handle)
    pat = crafted_planes(width, height, bd, bdc, chroma_format, units)
    return build(width, height, pat, bd, bdc, chroma_format, log2_ctu, pcm, bypass, 0, qp, starts, opts, tile_idx=tile, lf_across_tiles=lf_across_tiles,
                 sao_raw=random_sao(cw * ch, 31, chroma_format, bd, bdc))
