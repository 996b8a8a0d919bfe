// k_export.hip -- a finished picture converted into caller-owned device memory (hmgpu_picture_export, include/hmgpu.h "device export").
//   PLANAR / SEMIPLANAR: TVideoIOYuv::write's bit-depth rule (TVideoIOYuv.cpp:70-87, 743-763; CLIP_TO_709_RANGE 0), per channel type
//   RGB: chroma replicated to the luma grid (writePlane's 4:2:2 -> 4:4:4, TVideoIOYuv.cpp:425-443), an integer Y'CbCr -> R'G'B' matrix
//        whose coefficients the host derives (hmgpu_export_plan.coef), or the identity (RGBtoGBR, TVideoIOYuv.cpp:962-978)
// Memory-bound, no reuse beyond chroma: one lane per 4 samples of a row (8-byte loads per plane, 4- or 8-byte stores), rows along
// the grid's y, no LDS.  One instance per layout and container size, so nothing per sample branches on either.  The source planes
// keep at least 128 samples of margin right of the picture, so the loads of the last group of a row never leave the allocation;
// only its stores are cut to the row.
#include "hmgpu_dev.h"

namespace hmgpu {

namespace {

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

// n (<= 4) samples of one plane; full groups of an aligned export as one 4-byte (1 byte per sample) or 8-byte store
template <int BYTES>
__device__ inline void store4(uint8_t* d, const uint32_t o[4], int n, bool vec) {
  if (vec && n == 4) {
    if (BYTES == 1) stg(reinterpret_cast<uint32_t*>(d), o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24);
    else { u32x2 w; w.x = o[0] | o[1] << 16; w.y = o[2] | o[3] << 16; stg2(d, w); }
    return;
  }
  for (int i = 0; i < n; i++) {
    if (BYTES == 1) stg(d + i, (uint8_t)o[i]);
    else stg(reinterpret_cast<uint16_t*>(d) + i, (uint16_t)o[i]);
  }
}

}  // namespace

template <int LAYOUT, int BYTES>
__global__ void __launch_bounds__(256) k_export(const ExportArgs a) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int r = blockIdx.y;
  const bool vec = a.vec != 0;
  if (LAYOUT == HMGPU_EXPORT_RGB || r < a.h) {
    if (x >= a.w) return;
    const int n = min(4, a.w - x);
    int yv[4];
    load4(a.y + (ptrdiff_t)r * a.pitch_y + x, vec, yv);
    if (LAYOUT != HMGPU_EXPORT_RGB) {
      uint32_t o[4];
      for (int i = 0; i < 4; i++) o[i] = (uint32_t)depth_conv(yv[i], a.sh[0], a.maxv[0]) << a.msb[0];
      store4<BYTES>(a.dst[0] + r * a.pitch[0] + (ptrdiff_t)x * BYTES, o, n, vec);
      return;
    }
    // RGB: the chroma of the group's four luma samples (one pair for two of them when csx = 1)
    int u[4], v[4];
    if (a.mono) {
      for (int i = 0; i < 4; i++) u[i] = v[i] = a.coef[3];
    } else {
      const int16_t* cp = a.c + (ptrdiff_t)(r >> a.csy) * a.pitch_c + kCStep * (x >> a.csx);
      int p[8];
      load4(cp, vec, p);
      if (a.csx) {
        u[0] = u[1] = p[0]; v[0] = v[1] = p[1]; u[2] = u[3] = p[2]; v[2] = v[3] = p[3];
      } else {
        load4(cp + 4, vec, p + 4);
        for (int i = 0; i < 4; i++) { u[i] = p[2 * i]; v[i] = p[2 * i + 1]; }
      }
    }
    uint32_t R[4], G[4], B[4];
    if (a.coef[10]) {                     // identity (GBR): the YUV bit-depth rule per channel type
      for (int i = 0; i < 4; i++) {
        G[i] = (uint32_t)depth_conv(yv[i], a.sh[0], a.maxv[0]) << a.msb[0];
        B[i] = (uint32_t)depth_conv(u[i], a.sh[1], a.maxv[1]) << a.msb[1];
        R[i] = (uint32_t)depth_conv(v[i], a.sh[1], a.maxv[1]) << a.msb[1];
      }
    } else {
      const int S = a.coef[0], M = a.coef[9];
      for (int i = 0; i < 4; i++) {
        const int t = a.coef[4] * (yv[i] - a.coef[2]) + a.coef[1];
        const int cu = u[i] - a.coef[3], cv = v[i] - a.coef[3];
        R[i] = (uint32_t)min(M, max(0, (t + a.coef[5] * cv) >> S)) << a.msb[0];
        G[i] = (uint32_t)min(M, max(0, (t + a.coef[6] * cu + a.coef[7] * cv) >> S)) << a.msb[0];
        B[i] = (uint32_t)min(M, max(0, (t + a.coef[8] * cu) >> S)) << a.msb[0];
      }
    }
    const ptrdiff_t off = (ptrdiff_t)x * BYTES;
    store4<BYTES>(a.dst[0] + r * a.pitch[0] + off, R, n, vec);
    store4<BYTES>(a.dst[1] + r * a.pitch[1] + off, G, n, vec);
    store4<BYTES>(a.dst[2] + r * a.pitch[2] + off, B, n, vec);
    return;
  }
  // chroma rows of the YUV layouts: four CbCr pairs per lane
  const int rc = r - a.h;
  if (x >= a.cw) return;
  const int n = min(4, a.cw - x);
  int p[8];
  const int16_t* cp = a.c + (ptrdiff_t)rc * a.pitch_c + kCStep * x;
  load4(cp, vec, p);
  load4(cp + 4, vec, p + 4);
  uint32_t o[8];
  for (int i = 0; i < 8; i++) o[i] = (uint32_t)depth_conv(p[i], a.sh[1], a.maxv[1]) << a.msb[1];
  if (LAYOUT == HMGPU_EXPORT_PLANAR) {
    const uint32_t cb[4] = {o[0], o[2], o[4], o[6]}, cr[4] = {o[1], o[3], o[5], o[7]};
    const ptrdiff_t off = (ptrdiff_t)x * BYTES;
    store4<BYTES>(a.dst[1] + rc * a.pitch[1] + off, cb, n, vec);
    store4<BYTES>(a.dst[2] + rc * a.pitch[2] + off, cr, n, vec);
  } else {                                // the pairs as they lie: two groups of four samples
    uint8_t* d = a.dst[1] + rc * a.pitch[1] + (ptrdiff_t)x * 2 * BYTES;
    store4<BYTES>(d, o, min(4, 2 * n), vec);
    if (n > 2) store4<BYTES>(d + 4 * BYTES, o + 4, 2 * n - 4, vec);
  }
}

void launch_export(const ExportArgs& a, hipStream_t s) {
  const int groups = (std::max(a.w, a.layout == HMGPU_EXPORT_RGB ? 0 : a.cw) + 3) / 4;
  const int rows = a.h + (a.layout == HMGPU_EXPORT_RGB || a.mono ? 0 : a.ch);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)rows), block(256);
#define HMGPU_EXPORT_CASE(L)                                                              \
  if (a.layout == L) {                                                                    \
    if (a.bytes == 1) hipLaunchKernelGGL((k_export<L, 1>), grid, block, 0, s, a);         \
    else hipLaunchKernelGGL((k_export<L, 2>), grid, block, 0, s, a);                      \
  }
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_SEMIPLANAR)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB)
#undef HMGPU_EXPORT_CASE
}

}  // namespace hmgpu
