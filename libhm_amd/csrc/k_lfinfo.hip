// k_lfinfo.hip -- the loop-filter decisions of finished pictures written into caller-owned device memory
// (hmgpu_pictures_export_loopfilter, include/hmgpu.h "loop-filter export").
//   source: the edge-unit records k_prep left for the deblocking kernels (PicDev::edges: Bs, mean QP and exemptions of the four units of
//           every 8x8 luma area), the slice table (tc / beta offsets, PPS chroma offsets) and the SAO parameters of the last filter call
//   GRIDS:  the edge grid, thirteen int16 channels per 4x4 luma block, and the SAO grid, six int8 channels per CTB and component
//   DENSE:  Bs of the vertical / horizontal edge that can reach a sample and the luma SAO type, per output sample of a window export
// Pure gathers with a table lookup; no LDS, no atomics, no zeroing launch: every destination element is written exactly once.
//   GRIDS  edge part: one lane per 8x8 area, one 8-byte load of its EdgeRec; a wave is the 8 x 8 areas of one 64 x 64 luma square, a
//          workgroup four squares side by side.  With 64-sample CTUs (U) the square is a CTU: its slice index and the slice's constants
//          are the same in every lane and come through scalar loads.  A lane stores one dword (two adjacent int16) per channel and
//          block row, the eight lanes of an area row 32 contiguous bytes.  SAO part: the workgroups behind the edge part's, one lane
//          per CTB and component, component-major so that a wave stores runs of consecutive bytes.
//   DENSE  one lane per eight output samples of a row; a record is loaded once per run of samples that share it.
// The tc / beta tables and chroma_tc are filter_core.h's own: the values are what the filter kernels compute from the same record.
#include "hmgpu_dev.h"
#include "filter_core.h"
#include "quant_core.h"                            // resid_elem: the float output element of the side-information exports

namespace hmgpu {

namespace {

// a value that is the same in every lane of the wave (U): a scalar load through the constant address space, as in k_prep.hip
template <bool U, typename T> __device__ inline T ldu(const T* p) {
  if constexpr (U) return *(const T __attribute__((address_space(4)))*)p;
  else return ldg(p);
}

struct SliceLf { int tc_off, beta_off, cb_off, cr_off; };

// what the filters derive from one edge unit `rec` (EdgeRec, hmgpu_dev.h): v[0] Bs, 1 mean QP, 2 luma tc, 3 beta, 4 / 5 chroma tc of
// Cb / Cr (on_chroma: the unit lies on the chroma plane's own 8-sample grid), 6 the P / Q exemption bits.  All 0 where Bs is 0.
__device__ inline void unit_values(uint32_t rec, bool on_chroma, const SliceLf& sl, const LfArgs& a, int (&v)[7]) {
#pragma unroll
  for (int k = 0; k < 7; k++) v[k] = 0;
  const int bs = rec & 3;
  if (bs == 0) return;
  const int qp = (int)((rec >> 2) & 127) - 32;
  v[0] = bs; v[1] = qp;
  v[2] = c_tc_table[clip3(0, 53, qp + 2 * (bs - 1) + (sl.tc_off << 1))] << (a.bd[0] - 8);        // filter_luma_unit
  v[3] = c_beta_table[clip3(0, 51, qp + (sl.beta_off << 1))] << (a.bd[0] - 8);
  if (bs == 2 && on_chroma && !a.mono) {
    v[4] = chroma_tc(qp, sl.cb_off, sl.tc_off, a.bd[1], a.fmt);
    v[5] = chroma_tc(qp, sl.cr_off, sl.tc_off, a.bd[1], a.fmt);
  }
  v[6] = (rec >> 9) & 3;
}

// two adjacent int16 of one row
__device__ inline void store_pair(uint8_t* d, int lo, int hi, bool vec) {
  if (vec) { stg(reinterpret_cast<uint32_t*>(d), ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16)); return; }
  stg(reinterpret_cast<int16_t*>(d), (int16_t)lo);
  stg(reinterpret_cast<int16_t*>(d) + 1, (int16_t)hi);
}

// n (<= 4) consecutive elements of a dense row from the integers v
template <int ELEM>
__device__ inline void store_dense4(uint8_t* d, const int v[4], int n, bool vec, float sc) {
  constexpr int B = elem_bytes<ELEM>();
  uint32_t o[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if constexpr (ELEM == kElemU8) o[i] = (uint32_t)v[i] & 0xffu;
    else o[i] = resid_elem<ELEM>(v[i], sc);
  }
  if (vec && n == 4) {
    if constexpr (B == 1) stg(reinterpret_cast<uint32_t*>(d), o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24);
    else if constexpr (B == 2) { u32x2 w; w.x = o[0] | o[1] << 16; w.y = o[2] | o[3] << 16; stg2(d, w); }
    else { u32x4 w; w.x = o[0]; w.y = o[1]; w.z = o[2]; w.w = o[3]; stg4(d, w); }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (i >= n) break;
    if constexpr (B == 1) stg(d + i, (uint8_t)o[i]);
    else if constexpr (B == 2) stg(reinterpret_cast<uint16_t*>(d) + i, (uint16_t)o[i]);
    else stg(reinterpret_cast<uint32_t*>(d) + i, o[i]);
  }
}

}  // namespace

// edge_bx: workgroups per row of them; edge_blocks: workgroups of the edge part (0: no edge grid), the SAO part's follow
template <bool U>
__global__ void __launch_bounds__(256) k_lfinfo_grids(const LfArgs a, int edge_bx, int edge_blocks) {
  const int pic = blockIdx.y;
  const LfSrc& s = a.src[pic];
  if ((int)blockIdx.x >= edge_blocks) {
    // ---- SAO grid: one lane per CTB and component
    const int nct = a.ctus_w * a.ctus_h;
    const int item = ((int)blockIdx.x - edge_blocks) * 256 + (int)threadIdx.x;
    if (item >= 3 * nct) return;
    const int comp = item / nct, ctu = item - comp * nct;
    if (comp && a.mono) return;                                  // (4:0:0: the chroma components are left untouched)
    int ch[6] = {-1, 0, 0, 0, 0, 0};
    if (s.gate & kLfSao) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(s.saoprm + (size_t)ctu * 3 + comp);
      const uint32_t w0 = ldg(p), w1 = ldg(p + 1), w2 = ldg(p + 2);
      const int type = (int8_t)(w0 & 0xffu);
      if (type == HMGPU_SAO_BO) {
        ch[0] = type; ch[1] = (int)((w0 >> 8) & 0xffu);
#pragma unroll
        for (int i = 0; i < 4; i++) ch[2 + i] = (int8_t)((w1 >> (8 * i)) & 0xffu);
      } else if (type >= 0) {                                    // edge offset: SaoDev::off by edge class, class 2 is "none"
        ch[0] = type;
        ch[2] = (int8_t)(w1 & 0xffu); ch[3] = (int8_t)((w1 >> 8) & 0xffu); ch[4] = (int8_t)((w1 >> 24) & 0xffu); ch[5] = (int8_t)(w2 & 0xffu);
      }
    }
    const int cx = ctu % a.ctus_w, cy = ctu / a.ctus_w;
    int8_t* d = reinterpret_cast<int8_t*>(a.dst[1] + pic * a.bstride[1] + (int64_t)(comp * 6) * a.pstride[1] + cy * a.pitch[1]) + cx;
#pragma unroll
    for (int k = 0; k < 6; k++) stg(d + k * a.pstride[1], (int8_t)ch[k]);
    return;
  }
  // ---- edge grid: one lane per 8x8 area; a wave = the 8 x 8 areas of one 64 x 64 square aligned in the picture
  const int lane = threadIdx.x & 63;
  const int wave = U ? __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) : (int)threadIdx.x >> 6;
  const int sqx = (a.x8 >> 3) + ((int)blockIdx.x % edge_bx) * 4 + wave, sqy = (a.y8 >> 3) + (int)blockIdx.x / edge_bx;
  const int ax = sqx * 8 + (lane & 7), ay = sqy * 8 + (lane >> 3);
  if (ax < a.x8 || ax >= a.x8 + a.w8 || ay < a.y8 || ay >= a.y8 + a.h8) return;
  // the slice constants are those of the CTU the Q side -- the area itself -- lies in
  const int ctu = U ? sqy * a.ctus_w + sqx : ((ay * 8) >> a.log2ctu) * a.ctus_w + ((ax * 8) >> a.log2ctu);
  const int sidx = s.slice_idx ? min((int)ldu<U>(s.slice_idx + ctu), HMGPU_MAX_SLICES - 1) : 0;
  const SliceDev* sp = s.slices + sidx;
  SliceLf sl;
  sl.tc_off = ldu<U>(&sp->tc_offset_div2); sl.beta_off = ldu<U>(&sp->beta_offset_div2);
  sl.cb_off = ldu<U>(&sp->pps_cb_qp_offset); sl.cr_off = ldu<U>(&sp->pps_cr_qp_offset);
  const u32x2 er = ldg2(s.edges + (size_t)ay * a.ew + ax);
  // chroma filters the units on the chroma plane's own 8-sample grid: every second area across a subsampled direction
  const bool cv = !(a.csx && (ax & 1)), chh = !(a.csy && (ay & 1));
  int v0[7], v1[7], h0[7], h1[7];
  unit_values(er.x & 0xffffu, cv, sl, a, v0);
  unit_values(er.x >> 16, cv, sl, a, v1);
  unit_values(er.y & 0xffffu, chh, sl, a, h0);
  unit_values(er.y >> 16, chh, sl, a, h1);
  const bool vec = a.vec & 1;
  uint8_t* d = a.dst[0] + pic * a.bstride[0] + (int64_t)(2 * (ay - a.y8)) * a.pitch[0] + (ptrdiff_t)(2 * (ax - a.x8)) * 2;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    uint8_t* dv = d + (int64_t)(2 * q) * a.pstride[0];
    uint8_t* dh = dv + a.pstride[0];
    // vertical units: the left block of either row; horizontal units: both blocks of the upper row
    store_pair(dv, v0[q], 0, vec); store_pair(dv + a.pitch[0], v1[q], 0, vec);
    store_pair(dh, h0[q], h1[q], vec); store_pair(dh + a.pitch[0], 0, 0, vec);
  }
  uint8_t* df = d + (int64_t)HMGPU_LF_FLAGS * a.pstride[0];
  store_pair(df, v0[6] | (h0[6] << 2), h1[6] << 2, vec);
  store_pair(df + a.pitch[0], v1[6], 0, vec);
}

template <int ELEM>
__global__ void __launch_bounds__(256) k_lfinfo_dense(const LfArgs a) {
  constexpr int BYTES = elem_bytes<ELEM>();
  const int pic = blockIdx.z;
  const int c0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * 8;                       // destination columns c0 .. c0 + 7 of row oy
  const int oy = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (c0 >= a.W || oy >= a.H) return;
  const LfSrc& s = a.src[pic];
  const SideWin w = a.win[pic];
  const bool flip = (a.flip >> pic) & 1;
  const int y = w.top + nearest_src(oy, w.h, a.H);
  const int n = min(8, a.W - c0);
  // the horizontal edge that can reach row y, and the rows of the record grid the two directions read
  const int ey = (y + 4) & ~7;
  const bool hor_on = ey != 0 && ey < a.height;
  const uint16_t* row_v = reinterpret_cast<const uint16_t*>(s.edges + (size_t)(y >> 3) * a.ew) + ((y >> 2) & 1);
  const uint16_t* row_h = reinterpret_cast<const uint16_t*>(s.edges + (size_t)(hor_on ? ey >> 3 : 0) * a.ew) + 2;
  const int8_t* row_s = reinterpret_cast<const int8_t*>(s.saoprm + (size_t)(y >> a.log2ctu) * a.ctus_w * 3);
  int val[3][8];
  int bv = 0, bh = 0, st = 0, last_v = -1, last_h = -1, last_c = -1;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    if (j < n) {
      const int ox = flip ? a.W - 1 - (c0 + j) : c0 + j;                           // the mirror acts on the output: column c shows sample W - 1 - c
      const int x = w.left + nearest_src(ox, w.w, a.W);
      const int ex = (x + 4) & ~7;
      const int kv = (ex == 0 || ex >= a.width) ? 0 : ex >> 3;                     // (area 0 has no vertical edge to export: 0 stands for "none")
      if (kv != last_v) { bv = kv ? (int)(ldg(row_v + 4 * kv) & 3u) : 0; last_v = kv; }
      const int kh = x >> 2;
      if (kh != last_h) { bh = hor_on ? (int)(ldg(row_h + 4 * (x >> 3) + (kh & 1)) & 3u) : 0; last_h = kh; }
      const int kc = x >> a.log2ctu;
      if (kc != last_c) { st = (s.gate & kLfSao) ? (int)ldg(row_s + (size_t)kc * 3 * sizeof(SaoDev)) + 1 : 0; last_c = kc; }
    }
    val[0][j] = bv; val[1][j] = bh; val[2][j] = st;
  }
  const bool vec = (a.vec >> 2) & 1;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    uint8_t* d = a.dst[2] + pic * a.bstride[2] + c * a.pstride[2] + oy * a.pitch[2] + (ptrdiff_t)c0 * BYTES;
    store_dense4<ELEM>(d, val[c], min(4, n), vec, a.scale[c]);
    if (n > 4) store_dense4<ELEM>(d + 4 * BYTES, val[c] + 4, n - 4, vec, a.scale[c]);
  }
}

void launch_lfinfo_grids(const LfArgs& a, hipStream_t s) {
  int edge_bx = 1, edge_blocks = 0, sao_blocks = 0;
  if (a.dst[0]) {
    const int sq_x = ((a.x8 + a.w8 + 7) >> 3) - (a.x8 >> 3), sq_y = ((a.y8 + a.h8 + 7) >> 3) - (a.y8 >> 3);
    edge_bx = (sq_x + 3) / 4;
    edge_blocks = edge_bx * sq_y;
  }
  if (a.dst[1]) sao_blocks = (3 * a.ctus_w * a.ctus_h + 255) / 256;
  const dim3 grid((unsigned)(edge_blocks + sao_blocks), (unsigned)a.n), block(256);
  if (a.log2ctu == 6) hipLaunchKernelGGL(k_lfinfo_grids<true>, grid, block, 0, s, a, edge_bx, edge_blocks);
  else hipLaunchKernelGGL(k_lfinfo_grids<false>, grid, block, 0, s, a, edge_bx, edge_blocks);
}

void launch_lfinfo_dense(const LfArgs& a, int elem, hipStream_t s) {
  const dim3 grid((unsigned)((a.W + 255) / 256), (unsigned)((a.H + 7) / 8), (unsigned)a.n), block(256);
  if (elem == kElemU8) hipLaunchKernelGGL((k_lfinfo_dense<kElemU8>), grid, block, 0, s, a);
  else if (elem == kElemF16) hipLaunchKernelGGL((k_lfinfo_dense<kElemF16>), grid, block, 0, s, a);
  else if (elem == kElemBF16) hipLaunchKernelGGL((k_lfinfo_dense<kElemBF16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_lfinfo_dense<kElemF32>), grid, block, 0, s, a);
}

}  // namespace hmgpu
