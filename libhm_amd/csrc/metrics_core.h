// metrics_core.h -- what the two picture-metrics kernels share (k_metrics.hip: sums per picture; k_metrics_map.hip: sums per block):
// the loads of a group of 4 samples from a picture or from a caller's plane, the lane exchange, the sums of a 4x4 block and the value of
// an SSIM window from four of them -- one piece of code, so a window counts the same bits in a record and in a map
// (include/hmgpu.h "picture metrics").
#pragma once
#include "hmgpu_dev.h"

namespace hmgpu {

namespace {

typedef unsigned long long u64;

struct BlockSum { u64 ss, s12; uint32_t s1, s2; };   // of one 4x4 block: sum (a^2 + b^2), sum ab, sum a, sum b

// a 24-bit by 24-bit product, low 32 bits, unsigned (the intrinsic's result type is not relied on)
__device__ inline uint32_t mul24(uint32_t a, uint32_t b) { return (uint32_t)__umul24(a, b); }
__device__ inline uint32_t xor32(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m, 64); }
__device__ inline u64 xor64(u64 v, int m) { return ((u64)xor32((uint32_t)(v >> 32), m) << 32) | xor32((uint32_t)v, m); }

// 4 samples of one component (NC 1) or 4 Cb / Cr pairs (NC 2) at p: one load where the group is whole and aligned, else sample by
// sample up to nv; the rest stays 0
template <int NC>
__device__ inline void load_pic(const int16_t* p, bool vec, int nv, int v[NC][4]) {
  if (vec) {
    if (NC == 1) {
      const u32x2 q = ldg2(p);
      v[0][0] = (int16_t)(q.x & 0xffff); v[0][1] = (int16_t)(q.x >> 16); v[0][2] = (int16_t)(q.y & 0xffff); v[0][3] = (int16_t)(q.y >> 16);
    } else {
      const u32x4 q = ldg4(p);
      const uint32_t d[4] = {q.x, q.y, q.z, q.w};
      for (int j = 0; j < 4; j++) { v[0][j] = (int16_t)(d[j] & 0xffff); v[NC - 1][j] = (int16_t)(d[j] >> 16); }
    }
  } else {
    for (int j = 0; j < 4; j++)
      if (j < nv)
        for (int k = 0; k < NC; k++) v[k][j] = ldg(p + NC * j + k);
  }
}

// 4 elements of a caller's plane: uint8 (ES 1) or uint16 (ES 2)
template <int ES>
__device__ inline void load_plane(const uint8_t* p, bool vec, int nv, int v[4]) {
  if (vec) {
    if (ES == 1) {
      const uint32_t q = ldg(reinterpret_cast<const uint32_t*>(p));
      for (int j = 0; j < 4; j++) v[j] = (int)((q >> (8 * j)) & 0xff);
    } else {
      const u32x2 q = ldg2(p);
      v[0] = (int)(q.x & 0xffff); v[1] = (int)(q.x >> 16); v[2] = (int)(q.y & 0xffff); v[3] = (int)(q.y >> 16);
    }
  } else {
    for (int j = 0; j < 4; j++)
      if (j < nv) v[j] = ES == 1 ? (int)ldg(p + j) : (int)ldg(reinterpret_cast<const uint16_t*>(p) + j);
  }
}

// the SSIM terms of a lane's 4 samples of a and b, summed over the four rows of its 4x4 block: lanes 4k .. 4k + 3 hold the rows of
// block k, two __shfl_xor steps leave the block's sums in every one of them
__device__ inline BlockSum block_sums(const int va[4], const int vb[4]) {
  uint32_t s1 = 0, s2 = 0;
  u64 ss = 0, s12 = 0;
  for (int j = 0; j < 4; j++) {
    const uint32_t p = (uint32_t)va[j], q = (uint32_t)vb[j];
    s1 += p; s2 += q;
    ss += (u64)mul24(p, p) + (u64)mul24(q, q);
    s12 += (u64)mul24(p, q);
  }
  for (int m = 1; m <= 2; m <<= 1) { s1 += xor32(s1, m); s2 += xor32(s2, m); ss += xor64(ss, m); s12 += xor64(s12, m); }
  BlockSum o;
  o.ss = ss; o.s12 = s12; o.s1 = s1; o.s2 = s2;
  return o;
}

// llrint(ssim * 2^32) of the 8x8 window made of the 2x2 group of 4x4 blocks whose top-left one is b[0]; `right` / `below`: the
// distance to the block right of it and to the one below it
__device__ inline long long window_q32(const BlockSum* b, int right, int below, long long c1, long long c2) {
  long long s1 = 0, s2 = 0, ss = 0, s12 = 0;
  for (int q = 0; q < 4; q++) {
    const BlockSum& v = b[(q >> 1) * below + (q & 1) * right];
    s1 += v.s1; s2 += v.s2; ss += (long long)v.ss; s12 += (long long)v.s12;
  }
  const long long vars = 64 * ss - s1 * s1 - s2 * s2, covar = 64 * s12 - s1 * s2;
  const double num = (double)(2 * s1 * s2 + c1) * (double)(2 * covar + c2);
  const double den = (double)(s1 * s1 + s2 * s2 + c1) * (double)(vars + c2);
  return __double2ll_rn((num / den) * 4294967296.0);
}

}  // namespace

}  // namespace hmgpu
