// k_residual.hip -- the decoded residual of finished pictures written into caller-owned device memory
// (hmgpu_pictures_export_residual, include/hmgpu.h "residual export").
//   source: the residual tiles k_itx filled (PicDev::resid: 8x8 samples per 128-byte tile, row r in the 16-byte slot resid_slot(r)) and
//           HM's per-partition arrays, which say where a coded transform block lies
//   PLANES: int16 planes, each component at its own resolution          DENSE: one value per output sample of a window export
// A tile only holds what k_itx wrote for THIS picture inside coded transform blocks; everywhere else it holds whatever an earlier
// occupant of the handle left there.  Whether a 4x4 quadrant is covered therefore comes from the arrays alone -- the cbf chain down to the
// unit's transform depth, the rule by which k_prep lists the TUs (k_prep.hip) -- and an uncovered quadrant is written as 0, whatever the
// tile holds.  A luma row slot spans two partitions z, z + 1 of one 8x8 area; a chroma row slot (4:2:0) the chroma blocks of two 8x8
// areas, flagged at their first partitions z, z + 4 (the 4x4 chroma block under four 4x4 luma TUs is flagged there as well).
// Pure gathers, bound by HBM; no LDS, no arithmetic beyond the index maps and, for float elements, one product per sample.
//   PLANES  one lane per row slot (8 samples), 256 lanes per 64 x 32 samples of a component: the eight rows of a wave are one row of
//           tiles, so every 128-byte line a wave loads is used up by it, and eight lanes store 128 contiguous bytes of a row
//   DENSE   one lane per eight output samples of a row; a slot (and its two flags) is loaded once per run of samples that share it
#include "hmgpu_dev.h"
#include "quant_core.h"                            // resid_elem: the output element, shared with k_transform.hip

namespace hmgpu {

namespace {

// is the transform block over partition i coded?  ps / pm / dp / tr / cbf / pcm: the partition's bytes
__device__ inline bool coded(int log2ctu, int gate, int ps, int pm, int dp, int tr, int cbf, int pcm) {
  const int log2tu = log2ctu - dp - tr;
  const bool intra = pm == HMGPU_MODE_INTRA;
  const bool listed = ps != HMGPU_SIZE_NONE && log2tu >= 2 && log2tu <= 5 && (!intra || ((gate & kResidIntra) && !pcm));
  return listed && cbf_coded(cbf, tr & 7);
}

// the row slot of component `comp` that holds component sample (8 * sx8 .. 8 * sx8 + 7, y), with the halves no coded block covers zeroed.
// No load depends on another: the tile slot and the bytes of both partitions are issued together.
__device__ inline u32x4 load_slot(const ResidSrc& s, const ResidArgs& a, int comp, int sx8, int y) {
  const int16_t* tiles = comp == 0 ? s.resid[0] : comp == 1 ? s.resid[1] : s.resid[2];
  const uint8_t* cbfp = comp == 0 ? s.cbf[0] : comp == 1 ? s.cbf[1] : s.cbf[2];
  const int rtw = comp == 0 ? a.rtw[0] : a.rtw[1];
  const u32x4 v = ldg4(tiles + ((size_t)((y >> 3) * rtw + sx8) * 8 + resid_slot(y)) * 8);
  // the two 4x4 blocks of the slot: luma blocks (2 sx8, y >> 2), (2 sx8 + 1, y >> 2); chroma: the 8x8 luma areas at (4 sx8, (y >> 2) * 2), (4 sx8 + 2, ..)
  const int bx = comp ? 4 * sx8 : 2 * sx8, by = comp ? (y >> 2) * 2 : y >> 2, dz = comp ? 4 : 1;
  const Part pt = part_of(bx, by, a.log2ctu, a.ctus_w);
  const size_t p = (size_t)pt.ctu * a.parts + pt.z;
  int ps[2], pm[2], dp[2], tr[2], cb[2], pc[2] = {0, 0};
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const size_t q = p + i * dz;
    ps[i] = ldg(s.part_size + q); pm[i] = ldg(s.pred_mode + q); dp[i] = ldg(s.depth + q); tr[i] = ldg(s.tr_idx + q); cb[i] = ldg(cbfp + q);
    if (s.gate & kResidFlags) pc[i] = ldg(s.ipcm + q);
  }
  const bool c0 = coded(a.log2ctu, s.gate, ps[0], pm[0], dp[0], tr[0], cb[0], pc[0]);
  const bool c1 = coded(a.log2ctu, s.gate, ps[1], pm[1], dp[1], tr[1], cb[1], pc[1]);
  u32x4 r;
  r.x = c0 ? v.x : 0u; r.y = c0 ? v.y : 0u; r.z = c1 ? v.z : 0u; r.w = c1 ? v.w : 0u;
  return r;
}

// sample i (0 .. 7) of a slot, sign-extended
__device__ inline int slot_sample(const u32x4& v, int i) {
  const uint32_t w = (i & 4) ? ((i & 2) ? v.w : v.z) : ((i & 2) ? v.y : v.x);
  return (int16_t)((i & 1) ? (w >> 16) : (w & 0xffffu));
}

}  // namespace

// grid: x = 64-sample columns, y = 32-row bands of luma followed by those of chroma (Cb and Cr by the same lane), z = picture
__global__ void __launch_bounds__(256) k_residual_planes(const ResidArgs a, int luma_bands) {
  const int pic = blockIdx.z;
  const bool chroma = (int)blockIdx.y >= luma_bands;
  const int cs = chroma ? 1 : 0;
  const int band = chroma ? blockIdx.y - luma_bands : blockIdx.y;
  // the cropped window of this component, in its samples
  const int wx0 = a.x0 >> cs, wy0 = a.y0 >> cs, ww = a.w >> cs, wh = a.h >> cs;
  const int x = (wx0 & ~63) + (blockIdx.x * 8 + (threadIdx.x & 7)) * 8;        // the lane's eight samples: one row slot
  const int y = (wy0 & ~31) + band * 32 + (threadIdx.x >> 3);
  if (y < wy0 || y >= wy0 + wh || x + 8 <= wx0 || x >= wx0 + ww) return;
  const ResidSrc& s = a.src[pic];
  const int col = x - wx0, row = y - wy0;                                       // col may be -4 (chroma, a crop of half a slot)
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) mask |= (col + i >= 0 && col + i < ww ? 1u : 0u) << i;
  u32x4 v[2];
  const int c_lo = chroma ? 1 : 0, c_hi = chroma ? 2 : 0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int comp = c_lo + k;
    if (comp > c_hi || !a.dst[comp] || !((a.comps >> comp) & 1)) continue;
    v[k] = load_slot(s, a, comp, x >> 3, y);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int comp = c_lo + k;
    if (comp > c_hi || !a.dst[comp] || !((a.comps >> comp) & 1)) continue;
    uint8_t* d = a.dst[comp] + pic * a.bstride[comp] + row * a.pitch[comp] + (ptrdiff_t)col * 2;
    if (((a.vec >> comp) & 1) && mask == 0xffu) { stg4(d, v[k]); continue; }
#pragma unroll
    for (int i = 0; i < 8; i++) if ((mask >> i) & 1) stg(reinterpret_cast<int16_t*>(d) + i, (int16_t)slot_sample(v[k], i));
  }
}

template <int ELEM>
__global__ void __launch_bounds__(256) k_residual_dense(const ResidArgs a) {
  constexpr int BYTES = elem_bytes<ELEM>();
  const int pic = blockIdx.z;
  const int c0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * 8;                   // destination columns c0 .. c0 + 7 of row oy
  const int oy = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (c0 >= a.W || oy >= a.H) return;
  const ResidSrc& s = a.src[pic];
  const SideWin w = a.win[pic];
  const bool flip = (a.flip >> pic) & 1;
  const int sy = w.top + nearest_src(oy, w.h, a.H);
  const int n = min(8, a.W - c0);
  int sx[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int ox = flip ? a.W - 1 - (c0 + j) : c0 + j;                         // the mirror acts on the source index: stores ascend
    sx[j] = w.left + nearest_src(max(ox, 0), w.w, a.W);
  }
#pragma unroll
  for (int comp = 0; comp < 3; comp++) {
    if (!((a.comps >> comp) & 1)) continue;
    const int cs = comp ? 1 : 0;
    const float sc = comp == 0 ? a.scale[0] : comp == 1 ? a.scale[1] : a.scale[2];
    const int ch = comp == 0 ? a.chan[0] : comp == 1 ? a.chan[1] : a.chan[2];
    const int py = sy >> cs;
    uint32_t o[8];
    u32x4 v = {0u, 0u, 0u, 0u};
    int last = -1;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      o[j] = 0;
      if (j < n) {
        const int px = sx[j] >> cs;
        if ((px >> 3) != last) { last = px >> 3; v = load_slot(s, a, comp, last, py); }
        o[j] = resid_elem<ELEM>(slot_sample(v, px & 7), sc);
      }
    }
    uint8_t* d = a.dst[0] + pic * a.bstride[0] + ch * a.pstride[0] + oy * a.pitch[0] + (ptrdiff_t)c0 * BYTES;
    if ((a.vec & 1) && n == 8) {
      if constexpr (BYTES == 2) stg4(d, u32x4{o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16});
      else { stg4(d, u32x4{o[0], o[1], o[2], o[3]}); stg4(d + 16, u32x4{o[4], o[5], o[6], o[7]}); }
      continue;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (j >= n) break;
      if constexpr (BYTES == 2) stg(reinterpret_cast<uint16_t*>(d) + j, (uint16_t)o[j]);
      else stg(reinterpret_cast<uint32_t*>(d) + j, o[j]);
    }
  }
}

void launch_residual_planes(const ResidArgs& a, hipStream_t s) {
  const int cols = ((a.x0 + a.w + 63) >> 6) - (a.x0 >> 6);                     // (the chroma window needs no more 64-sample columns than the luma one)
  const int lb = (a.comps & 1) && a.dst[0] ? ((a.y0 + a.h + 31) >> 5) - (a.y0 >> 5) : 0;
  const int cy0 = a.y0 >> 1, ch = a.h >> 1;
  const int cb = ((a.comps & 6) && (a.dst[1] || a.dst[2])) ? ((cy0 + ch + 31) >> 5) - (cy0 >> 5) : 0;
  if (lb + cb == 0) return;
  const dim3 grid((unsigned)cols, (unsigned)(lb + cb), (unsigned)a.n), block(256);
  hipLaunchKernelGGL(k_residual_planes, grid, block, 0, s, a, lb);
}

void launch_residual_dense(const ResidArgs& a, int elem, hipStream_t s) {
  const dim3 grid((unsigned)((a.W + 255) / 256), (unsigned)((a.H + 7) / 8), (unsigned)a.n), block(256);
  if (elem == kElemU16) hipLaunchKernelGGL((k_residual_dense<kElemU16>), grid, block, 0, s, a);
  else if (elem == kElemF16) hipLaunchKernelGGL((k_residual_dense<kElemF16>), grid, block, 0, s, a);
  else if (elem == kElemBF16) hipLaunchKernelGGL((k_residual_dense<kElemBF16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_residual_dense<kElemF32>), grid, block, 0, s, a);
}

}  // namespace hmgpu
