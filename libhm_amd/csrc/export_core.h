// export_core.h -- what the unscaled YUV export kernels share (k_export.hip, k_export_fmt.hip): the bit-depth rule, the loads of a
// lane's group, a luma row, and the way four CbCr pairs at the output depth leave a lane.  k_export.hip takes depth_conv and load4
// from here, which leaves its instances' instructions as they were; its luma and chroma rows keep their own few lines of the two row
// functions below, because calling them reorders a handful of its byte-packing instructions.
#pragma once
#include "hmgpu_dev.h"

namespace hmgpu {

__device__ inline int depth_conv(int v, int sh, int maxv) {
  return sh >= 0 ? v << sh : min(maxv, max(0, (v + (1 << (-sh - 1))) >> -sh));
}

// 4 consecutive int16 samples: one 8-byte load, or four 2-byte ones where the group is not 8-byte aligned
__device__ inline void load4(const int16_t* p, bool vec, int v[4]) {
  if (vec) {
    const u32x2 w = ldg2(p);
    v[0] = (int16_t)(w.x & 0xffff); v[1] = (int16_t)(w.x >> 16); v[2] = (int16_t)(w.y & 0xffff); v[3] = (int16_t)(w.y >> 16);
  } else {
    for (int i = 0; i < 4; i++) v[i] = ldg(p + i);
  }
}

// 8 consecutive int16 samples (four CbCr pairs): one 16-byte load where load4 would use 8-byte ones (the group is 8-byte aligned, and
// 16-byte aligned wherever the window starts on a multiple of 4 pairs), else eight 2-byte ones.  One instruction for the lane's 16
// contiguous bytes, so that a wave's load touches every cache line once
__device__ inline void load8(const int16_t* p, bool vec, int v[8]) {
  if (vec) {
    const u32x4 w = ldg4_a8(p);
    v[0] = (int16_t)(w.x & 0xffff); v[1] = (int16_t)(w.x >> 16); v[2] = (int16_t)(w.y & 0xffff); v[3] = (int16_t)(w.y >> 16);
    v[4] = (int16_t)(w.z & 0xffff); v[5] = (int16_t)(w.z >> 16); v[6] = (int16_t)(w.w & 0xffff); v[7] = (int16_t)(w.w >> 16);
  } else {
    for (int i = 0; i < 8; i++) v[i] = ldg(p + i);
  }
}

// the group of n luma samples yv at column x of row r of a YUV layout: the depth rule, then the store
template <int ELEM>
__device__ inline void export_luma_row(const ExportArgs& a, uint8_t* d0, int r, int x, int n, const int yv[4], bool vec, bool flip) {
  uint32_t o[4];
  for (int i = 0; i < 4; i++) o[i] = (uint32_t)depth_conv(yv[i], a.sh[0], a.maxv[0]);
  export_store_row<ELEM>(d0 + r * a.pitch[0], x, a.w, o, n, vec, flip, a.msb[0], a.scale[0], a.bias[0]);
}

// n CbCr pairs o[2j], o[2j + 1], already at the output depth, at pair x of chroma row rc: two planes, or the pairs as they lie
template <int LAYOUT, int ELEM>
__device__ inline void export_chroma_out(const ExportArgs& a, uint8_t* d1, uint8_t* d2, int rc, int x, int n, const uint32_t o[8], bool vec, bool flip) {
  if (LAYOUT == HMGPU_EXPORT_PLANAR) {
    const uint32_t cb[4] = {o[0], o[2], o[4], o[6]}, cr[4] = {o[1], o[3], o[5], o[7]};
    export_store_row<ELEM>(d1 + rc * a.pitch[1], x, a.cw, cb, n, vec, flip, a.msb[1], a.scale[1], a.bias[1]);
    export_store_row<ELEM>(d2 + rc * a.pitch[2], x, a.cw, cr, n, vec, flip, a.msb[1], a.scale[2], a.bias[2]);
  } else {                                // the pairs as they lie: two groups of four samples
    export_store_pairs<ELEM>(d1 + rc * a.pitch[1], x, a.cw, o, n, vec, flip, a.msb[1]);
  }
}

}  // namespace hmgpu
