// k_motion.hip -- motion vectors, reference POCs and block information of finished pictures written into caller-owned device memory
// (hmgpu_pictures_export_motion, include/hmgpu.h "motion and block export").
//   source: HM's per-partition arrays as the decompress calls staged them (CTU raster, z-scan inside a CTU) and the slice table
//   BLOCKS: the grid of 4x4 luma blocks as int16 / int32 / int8 planes          DENSE: one value per output sample of a window export
// Pure gathers, bound by HBM and by how the z-scan lines up with raster rows; no LDS, no arithmetic beyond the index maps.
//   BLOCKS  one lane per four blocks of a row, aligned to four in the picture: inside any CTU these are partitions z, z + 1, z + 4,
//           z + 5, so every byte array is two 2-byte loads and a list's vectors two 8-byte loads; a workgroup covers 64 x 16 blocks
//           (256 x 64 luma samples: whole 64-sample CTUs, every loaded line is used up inside the workgroup), and the 16 lanes of a
//           row store 128 contiguous bytes of an int16 plane, 256 of ref_poc, 64 of a block plane.
//   DENSE   one lane per eight output samples of a row; the block record is looked up once per run of samples that share a block.
// The slice type of the block's CTU gates every read of the list arrays: list 1 of a picture without B slices is never loaded
// (it may hold an earlier picture's values), list 0 of an I slice neither.
#include "hmgpu_dev.h"

namespace hmgpu {

namespace {

struct MotionRec {
  int32_t mvx[2], mvy[2];   // quarter luma samples; 0 where the list is unused
  int32_t poc[2];           // HMGPU_MOTION_NO_REF where the list is unused
  int32_t info[4];          // mode, log2 CU size, part_size, QP
};

template <int N> __device__ inline uint32_t ld_bytes(const void* p) {
  if constexpr (N == 1) return ldg(static_cast<const uint8_t*>(p));
  else return ldg(static_cast<const uint16_t*>(p));                       // (z is even: 2-byte aligned)
}

// N (1 or 2) z-consecutive partitions of CTU `ctu`, first z-index z (even when N = 2)
template <int N>
__device__ inline void load_recs(const MotionSrc& s, const MotionArgs& a, int ctu, int z, bool want_motion, bool want_block, MotionRec* r) {
  const size_t p = (size_t)ctu * a.parts + z;
  const uint32_t ps = ld_bytes<N>(s.part_size + p), pm = ld_bytes<N>(s.pred_mode + p);
  uint32_t dp = 0, qp = 0;
  if (want_block) { dp = ld_bytes<N>(s.depth + p); qp = ld_bytes<N>(s.qp + p); }
  const SliceDev* sl = s.slices + min((int)ldg(s.slice_idx + ctu), HMGPU_MAX_SLICES - 1);
  uint32_t ri[2] = {0xffffffffu, 0xffffffffu}, mv[2][N] = {};
  bool on[2] = {false, false};
  if (want_motion) {
    const int st = ldg(&sl->slice_type);
#pragma unroll
    for (int l = 0; l < 2; l++) {
      on[l] = ((a.lists >> l) & 1) && (st == HMGPU_B_SLICE || (l == 0 && st == HMGPU_P_SLICE));
      if (!on[l]) continue;
      ri[l] = ld_bytes<N>(s.ref_idx[l] + p);
      if constexpr (N == 1) {
        mv[l][0] = ldg(reinterpret_cast<const uint32_t*>(s.mv[l] + 2 * p));
      } else {
        const u32x2 w = ldg2(s.mv[l] + 2 * p);
        mv[l][0] = w.x; mv[l][1] = w.y;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    const int psi = (int8_t)(ps >> (8 * i)), pmi = (int8_t)(pm >> (8 * i));
    const bool decoded = psi != HMGPU_SIZE_NONE, inter = decoded && pmi == HMGPU_MODE_INTER;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      const int ref = (int8_t)(ri[l] >> (8 * i));
      const bool used = on[l] && inter && ref >= 0;
      r[i].mvx[l] = used ? (int16_t)(mv[l][i] & 0xffff) : 0;
      r[i].mvy[l] = used ? (int16_t)(mv[l][i] >> 16) : 0;
      r[i].poc[l] = used ? ldg(&sl->ref_poc[l][ref & (HMGPU_MAX_REF - 1)]) : HMGPU_MOTION_NO_REF;
    }
    r[i].info[0] = !decoded ? -1 : pmi == HMGPU_MODE_INTER ? 0 : pmi == HMGPU_MODE_INTRA ? 1 : -1;
    r[i].info[1] = a.log2ctu - (int)((dp >> (8 * i)) & 0xff);
    r[i].info[2] = decoded ? psi : -1;
    r[i].info[3] = (int8_t)(qp >> (8 * i));
  }
}

// four consecutive elements of one row, the first at d: element i is stored where bit i of `mask` is set; all four as one store where
// `vec` says the position is aligned
__device__ inline void store_i16(uint8_t* d, const int32_t v[4], uint32_t mask, bool vec) {
  if (vec && mask == 15u) { u32x2 w; w.x = (v[0] & 0xffff) | ((uint32_t)v[1] << 16); w.y = (v[2] & 0xffff) | ((uint32_t)v[3] << 16); stg2(d, w); return; }
#pragma unroll
  for (int i = 0; i < 4; i++) if ((mask >> i) & 1) stg(reinterpret_cast<int16_t*>(d) + i, (int16_t)v[i]);
}
__device__ inline void store_i32(uint8_t* d, const int32_t v[4], uint32_t mask, bool vec) {
  if (vec && mask == 15u) { u32x4 w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3]; stg4(d, w); return; }
#pragma unroll
  for (int i = 0; i < 4; i++) if ((mask >> i) & 1) stg(reinterpret_cast<int32_t*>(d) + i, v[i]);
}
__device__ inline void store_i8(uint8_t* d, const int32_t v[4], uint32_t mask, bool vec) {
  if (vec && mask == 15u) { stg(reinterpret_cast<uint32_t*>(d), (v[0] & 0xffu) | ((v[1] & 0xffu) << 8) | ((v[2] & 0xffu) << 16) | ((uint32_t)v[3] << 24)); return; }
#pragma unroll
  for (int i = 0; i < 4; i++) if ((mask >> i) & 1) stg(reinterpret_cast<int8_t*>(d) + i, (int8_t)v[i]);
}

}  // namespace

__global__ void __launch_bounds__(256) k_motion_blocks(const MotionArgs a) {
  const int pic = blockIdx.z;
  const int by = a.y4 + blockIdx.y * 16 + (threadIdx.x >> 4);
  const int bx0 = (a.x4 & ~3) + (blockIdx.x * 16 + (threadIdx.x & 15)) * 4;       // four blocks, aligned to four in the picture
  if (by >= a.y4 + a.h4 || bx0 >= a.x4 + a.w4) return;
  const MotionSrc& s = a.src[pic];
  const bool want_motion = a.dst[0] || a.dst[2], want_block = a.dst[3] != nullptr;
  const Part p = part_of(bx0, by, a.log2ctu, a.ctus_w);                            // (a CTU is at least four blocks wide: one CTU per lane)
  MotionRec r[4];
  load_recs<2>(s, a, p.ctu, p.z, want_motion, want_block, r);
  load_recs<2>(s, a, p.ctu, p.z + 4, want_motion, want_block, r + 2);
  // the lane's columns of the cropped grid: c0 .. c0 + 3, those inside [0, w4) are written (d may point in front of the row: masked)
  const int row = by - a.y4, c0 = bx0 - a.x4;
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) mask |= (c0 + i >= 0 && c0 + i < a.w4 ? 1u : 0u) << i;
  int32_t v[4];
  if (a.dst[0]) {
    uint8_t* d = a.dst[0] + pic * a.bstride[0] + row * a.pitch[0] + (ptrdiff_t)c0 * 2;
    int plane = 0;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      if (!((a.lists >> l) & 1)) continue;
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = r[i].mvx[l];
      store_i16(d + plane * a.pstride[0], v, mask, a.vec & 1);
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = r[i].mvy[l];
      store_i16(d + (plane + 1) * a.pstride[0], v, mask, a.vec & 1);
      plane += 2;
    }
  }
  if (a.dst[2]) {
    uint8_t* d = a.dst[2] + pic * a.bstride[2] + row * a.pitch[2] + (ptrdiff_t)c0 * 4;
    int plane = 0;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      if (!((a.lists >> l) & 1)) continue;
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = r[i].poc[l];
      store_i32(d + plane * a.pstride[2], v, mask, a.vec & 4);
      plane++;
    }
  }
  if (a.dst[3]) {
    uint8_t* d = a.dst[3] + pic * a.bstride[3] + row * a.pitch[3] + c0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] = r[i].info[k];
      store_i8(d + k * a.pstride[3], v, mask, a.vec & 8);
    }
  }
}

template <int ELEM>
__global__ void __launch_bounds__(256) k_motion_dense(const MotionArgs a) {
  constexpr int BYTES = elem_bytes<ELEM>();
  const int pic = blockIdx.z;
  const int c0 = (blockIdx.x * 32 + (threadIdx.x & 31)) * 8;                       // destination columns c0 .. c0 + 7 of row oy
  const int oy = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (c0 >= a.W || oy >= a.H) return;
  const MotionSrc& s = a.src[pic];
  const MotionWin w = a.win[pic];
  const bool flip = (a.flip >> pic) & 1;
  const bool want_motion = a.dst[0] || a.dst[1] || a.dst[2], want_block = a.dst[3] != nullptr;
  const int sh = a.log2ctu - 2, m = (1 << sh) - 1;
  const int by = (w.top + nearest_src(oy, w.h, a.H)) >> 2;
  const int n = min(8, a.W - c0);
  int32_t dx[2][8], dy[2][8], poc[2][8], info[4][8];
  MotionRec r = {};
  int last = -1;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int ox = flip ? a.W - 1 - (c0 + j) : c0 + j;                             // the mirror acts on the output: column c shows sample W - 1 - c
    if (j < n) {
      const int bx = (w.left + nearest_src(ox, w.w, a.W)) >> 2;
      if (bx != last) {
        const int ctu = (by >> sh) * a.ctus_w + (bx >> sh);                        // (part_of written out: sh and m stay outside the unrolled loop)
        load_recs<1>(s, a, ctu, spread4(bx & m) | (spread4(by & m) << 1), want_motion, want_block, &r);
        last = bx;
      }
    }
    for (int l = 0; l < 2; l++) { dx[l][j] = flip ? -r.mvx[l] : r.mvx[l]; dy[l][j] = r.mvy[l]; poc[l][j] = r.poc[l]; }
    for (int k = 0; k < 4; k++) info[k][j] = r.info[k];
  }
#pragma unroll
  for (int l = 0; l < 2; l++) {
    if (!a.dst[l]) continue;
    uint8_t* d = a.dst[l] + pic * a.bstride[l] + oy * a.pitch[l] + (ptrdiff_t)c0 * BYTES;
    const bool vec = (a.vec >> l) & 1;
#pragma unroll
    for (int g = 0; g < 2; g++) {
      const int ng = min(4, n - 4 * g);
      if (ng <= 0) continue;
      uint32_t ux[4], uy[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { ux[i] = (uint32_t)dx[l][4 * g + i]; uy[i] = (uint32_t)dy[l][4 * g + i]; }
      export_store4<ELEM>(d + 4 * g * BYTES, ux, ng, vec, 0, w.kx, 0.f);
      export_store4<ELEM>(d + a.pstride[l] + 4 * g * BYTES, uy, ng, vec, 0, w.ky, 0.f);
    }
  }
  int32_t v[4];
  if (a.dst[2]) {
    uint8_t* d = a.dst[2] + pic * a.bstride[2] + oy * a.pitch[2] + (ptrdiff_t)c0 * 4;
    int plane = 0;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      if (!((a.lists >> l) & 1)) continue;
#pragma unroll
      for (int g = 0; g < 2; g++) {
        const int ng = min(4, n - 4 * g);
        if (ng <= 0) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = poc[l][4 * g + i];
        store_i32(d + plane * a.pstride[2] + 16 * g, v, (1u << ng) - 1u, (a.vec >> 2) & 1);
      }
      plane++;
    }
  }
  if (a.dst[3]) {
    uint8_t* d = a.dst[3] + pic * a.bstride[3] + oy * a.pitch[3] + c0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int g = 0; g < 2; g++) {
        const int ng = min(4, n - 4 * g);
        if (ng <= 0) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = info[k][4 * g + i];
        store_i8(d + k * a.pstride[3] + 4 * g, v, (1u << ng) - 1u, (a.vec >> 3) & 1);
      }
  }
}

void launch_motion_blocks(const MotionArgs& a, hipStream_t s) {
  const int groups = ((a.x4 + a.w4 + 3) >> 2) - (a.x4 >> 2);
  const dim3 grid((unsigned)((groups + 15) / 16), (unsigned)((a.h4 + 15) / 16), (unsigned)a.n), block(256);
  hipLaunchKernelGGL(k_motion_blocks, grid, block, 0, s, a);
}

void launch_motion_dense(const MotionArgs& a, int elem, hipStream_t s) {
  const dim3 grid((unsigned)((a.W + 255) / 256), (unsigned)((a.H + 7) / 8), (unsigned)a.n), block(256);
  if (elem == kElemF16) hipLaunchKernelGGL((k_motion_dense<kElemF16>), grid, block, 0, s, a);
  else if (elem == kElemBF16) hipLaunchKernelGGL((k_motion_dense<kElemBF16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_motion_dense<kElemF32>), grid, block, 0, s, a);
}

}  // namespace hmgpu
