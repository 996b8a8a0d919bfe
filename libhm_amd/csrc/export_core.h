// export_core.h -- the one device core of the picture exports (k_export.hip, k_export_fmt.hip; k_export_scale.hip and k_export_warp.hip in part)
// and of k_histogram.hip's maxRGB.  Each rule stands here once:
//   - the bit-depth rule (depth_conv) and the loads of a lane's group (load4, load8, unpack8; export_load by group size);
//   - the chroma of a group of N luma samples: replicated to the luma grid (export_chroma_replicated; callers at N = 4) or interpolated at
//     the signalled sample location (export_chroma_sited; callers at N = 4: the six loads, then chroma_core.h's arithmetic);
//   - the conversion to R'G'B', the integer matrix or the identity (export_rgb), for the 1- and 4-sample callers;
//   - the container shift of the R and B channels (export_mc);
//   - the RGB store step: the optional colour stage (colour_core.h), then three planes or packed pixels (export_store_rgb);
//   - the YUV store steps: a luma row, and four CbCr pairs as two planes or as they lie;
//   - on the host, the one dispatch from the runtime element / pixel size / stages to the compile-time instance (export_rgb_instance,
//     export_yuv_instance), which every launch function of the four kernel files goes through.
// The helpers take the kernel's argument record as a template parameter: ExportArgs, ScaleArgs, WarpArgs and HistogramArgs name the
// fields they read (coef, sh, maxv, msb, mono, csx, csy, pitch_c) alike.
// Two habits keep these helpers free of scratch memory and of repeated scalar loads once they are inlined, and are to be kept:
//   - where two branches of a helper fill the same output arrays, both write them in the same order (u before v; G, B, R).  The
//     compiler merges the branches' stores while the arrays are still pointer arguments; stores in differing order merge into a store
//     through a chosen pointer, which then keeps the caller's arrays in memory (12 to 20 bytes of scratch per lane, measured);
//   - launch-uniform fields are read into locals before a loop over the samples, not inside it.
// What stays outside, because sharing it would make this file branch on its caller:
//   - k_export.hip's luma and chroma rows of the YUV layouts keep their own few lines of export_luma_row / export_chroma_out:
//     calling them reorders a handful of that kernel's byte-packing instructions;
// And what could be shared but is not, for speed: k_export_scale.hip's stage step and epilogue keep their own 8-sample text of the
// chroma fetches, the conversion and the store choice, and k_export_warp.hip's tap and epilogue their own 1-sample text of the
// replicated chroma, the conversion and the store choice (their headers have the measurements).  Both take the depth rule, the
// unpack and the dispatch from here.  The helpers below stay templates on the group size; only N = 4 (and export_rgb<1>, from
// k_histogram.hip) has callers at present.
#pragma once
#include "hmgpu_dev.h"
#include "colour_core.h"
#include "chroma_core.h"

#include <type_traits>

namespace hmgpu {

// the kernels' optional stages travel as a parameter pack behind their first argument (PxOrder, ChromaSite, ColourLut, in that
// order): whether the pack holds a T, and that T
template <class T, class... X> constexpr bool pack_has = (std::is_same_v<T, X> || ...);
template <class T, class U, class... X>
__device__ inline const T& pack_get(const U& u, const X&... x) {
  if constexpr (std::is_same_v<T, U>) return u;
  else return pack_get<T>(x...);
}

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

// the 8 int16 samples of one 16-byte load
__device__ inline void unpack8(const u32x4 w, int v[8]) {
  for (int i = 0; i < 4; i++) { v[2 * i] = (int16_t)(w[i] & 0xffff); v[2 * i + 1] = (int16_t)(w[i] >> 16); }
}

// 8 consecutive int16 samples (four CbCr pairs): one 16-byte load where load4 would use 8-byte ones (the group is 8-byte aligned, and
// 16-byte aligned wherever the window starts on a multiple of 4 pairs), else eight 2-byte ones.  One instruction for the lane's 16
// contiguous bytes, so that a wave's load touches every cache line once
__device__ inline void load8(const int16_t* p, bool vec, int v[8]) {
  if (vec) unpack8(ldg4_a8(p), v);
  else for (int i = 0; i < 8; i++) v[i] = ldg(p + i);
}

// N consecutive int16 samples of a lane's group: N = 4 by load4; N = 8 a 16-byte group of the scaled export's staged span, which is
// 16-byte aligned by construction (vec is not read)
template <int N>
__device__ inline void export_load(const int16_t* p, bool vec, int v[N]) {
  static_assert(N == 4 || N == 8, "group size");
  if constexpr (N == 4) load4(p, vec, v);
  else unpack8(ldg4(p), v);
}

// Chroma of the N luma samples at column x (a multiple of N) of row y, replicated to the luma grid: the 4:0:0 constant, one pair for
// two samples (csx = 1) or a pair each.  c: the pair plane at the origin that x and y count from
template <int N, class A>
__device__ inline void export_chroma_replicated(const A& a, const int16_t* c, int y, int x, bool vec, int u[N], int v[N]) {
  if (a.mono) {
    for (int i = 0; i < N; i++) { u[i] = a.coef[3]; v[i] = a.coef[3]; }
  } else {
    const int16_t* cp = c + (ptrdiff_t)(y >> a.csy) * a.pitch_c + kCStep * (x >> a.csx);
    if constexpr (N == 1) {
      chroma_pair(cp, u, v);
    } else {
      int p[2 * N];
      export_load<N>(cp, vec, p);
      if (a.csx) {
        for (int i = 0; i < N; i++) { u[i] = p[2 * (i >> 1)]; v[i] = p[2 * (i >> 1) + 1]; }
      } else {
        export_load<N>(cp + N, vec, p + N);
        for (int i = 0; i < N; i++) { u[i] = p[2 * i]; v[i] = p[2 * i + 1]; }
      }
    }
  }
}

// The same chroma through the chroma stage (chroma_core.h; csx = 1): pairs J - 1 .. J + N / 2 of the two rows ia and ib that
// chroma_rows chose, row ia with weight w -- six loads none of which waits for another.  pa / pb: pair J of those rows, J in plane
// coordinates
template <int N>
__device__ inline void export_chroma_sited(const ChromaSite& cs, const int16_t* pa, const int16_t* pb, int J, int w, bool vec, int u[N], int v[N]) {
  constexpr int H = N / 2;
  int ma[N], mb[N], ua[H + 2], ub[H + 2], va[H + 2], vb[H + 2];
  export_load<N>(pa, vec, ma);
  export_load<N>(pb, vec, mb);
  chroma_pair(pa - kCStep, &ua[0], &va[0]);
  chroma_pair(pb - kCStep, &ub[0], &vb[0]);
  chroma_pair(pa + H * kCStep, &ua[H + 1], &va[H + 1]);
  chroma_pair(pb + H * kCStep, &ub[H + 1], &vb[H + 1]);
  for (int i = 0; i < H; i++) { ua[1 + i] = ma[2 * i]; va[1 + i] = ma[2 * i + 1]; ub[1 + i] = mb[2 * i]; vb[1 + i] = mb[2 * i + 1]; }
  chroma_line<H>(cs, J, w, ua, ub, u);
  chroma_line<H>(cs, J, w, va, vb, v);
}

// N samples' R'G'B': the integer matrix of hmgpu_export_plan.coef, or (coef[10]) the identity (GBR), which is the YUV bit-depth rule
// per channel type
template <int N, class A>
__device__ inline void export_rgb(const A& a, const int y[N], const int u[N], const int v[N], uint32_t R[N], uint32_t G[N], uint32_t B[N]) {
  if (a.coef[10]) {
    const int sl = a.sh[0], ml = a.maxv[0], sc = a.sh[1], mc = a.maxv[1];
    for (int i = 0; i < N; i++) {
      G[i] = (uint32_t)depth_conv(y[i], sl, ml);
      B[i] = (uint32_t)depth_conv(u[i], sc, mc);
      R[i] = (uint32_t)depth_conv(v[i], sc, mc);
    }
  } else {
    const int S = a.coef[0], M = a.coef[9], rnd = a.coef[1], yoff = a.coef[2], coff = a.coef[3];
    const int ky = a.coef[4], krv = a.coef[5], kgu = a.coef[6], kgv = a.coef[7], kbu = a.coef[8];
    for (int i = 0; i < N; i++) {
      const int t = ky * (y[i] - yoff) + rnd;
      const int cu = u[i] - coff, cv = v[i] - coff;
      G[i] = (uint32_t)min(M, max(0, (t + kgu * cu + kgv * cv) >> S));
      B[i] = (uint32_t)min(M, max(0, (t + kbu * cu) >> S));
      R[i] = (uint32_t)min(M, max(0, (t + krv * cv) >> S));
    }
  }
}

// the container shift of R and B (G always carries the luma one): under the identity they are chroma channels
template <class A>
__device__ inline int export_mc(const A& a) { return a.coef[10] ? a.msb[1] : a.msb[0]; }

// The store step of every RGB export: the group of n (<= 4) pixels at column x of row y of picture pic, w pixels a row, through the
// colour stage where the pack st holds a ColourLut, then as three planes (NCH 0) or as packed pixels of NCH elements in the order po.
// mrb / mg: the container shifts of R and B / of G
template <int ELEM, int NCH, class A, class... X>
__device__ inline void export_store_rgb(const A& a, const PxOrder& po, int pic, int y, int x, int w, uint32_t R[4], uint32_t G[4], uint32_t B[4],
                                        int n, bool vec, bool flip, int mrb, int mg, const X&... st) {
  if constexpr (pack_has<ColourLut, X...>) colour_map4(pack_get<ColourLut>(st...), R, G, B);
  if constexpr (NCH != 0) {
    export_store_px<ELEM, NCH>(a.dst[0] + pic * a.bstride[0] + y * a.pitch[0], x, w, R, G, B, n, vec, flip, mrb, mg, a.scale, a.bias, po);
  } else {
    export_store_row<ELEM>(a.dst[0] + pic * a.bstride[0] + y * a.pitch[0], x, w, R, n, vec, flip, mrb, a.scale[0], a.bias[0]);
    export_store_row<ELEM>(a.dst[1] + pic * a.bstride[1] + y * a.pitch[1], x, w, G, n, vec, flip, mg, a.scale[1], a.bias[1]);
    export_store_row<ELEM>(a.dst[2] + pic * a.bstride[2] + y * a.pitch[2], x, w, B, n, vec, flip, mrb, a.scale[2], a.bias[2]);
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

// ---- host: from the runtime choice to the compile-time instance ------------------------------------------------------
// f(std::integral_constant<int, V>) for the V that v equals; false where it equals none
template <int... V, class F>
inline bool export_pick(int v, F&& f) {
  return ((v == V && (f(std::integral_constant<int, V>()), true)) || ...);
}

// The instance of an RGB kernel family: f(element, nch, stages...) with the element and the pixel size (0: planes, 3, 4) as
// integral constants and the stages that are present, a ChromaSite before a ColourLut, by reference.  5 x 3 x 4 instances
template <class F>
inline void export_rgb_instance(int elem, int nch, const ChromaSite* cs, const ColourLut* lut, F&& f) {
  export_pick<kElemU8, kElemU16, kElemF16, kElemBF16, kElemF32>(elem, [&](auto e) {
    export_pick<0, 3, 4>(nch, [&](auto n) {
      if (cs && lut) f(e, n, *cs, *lut);
      else if (cs) f(e, n, *cs);
      else if (lut) f(e, n, *lut);
      else f(e, n);
    });
  });
}

// The instance of a YUV kernel family: f(layout, element).  The planar layout has every element, the semi-planar one the integer
// elements only (the host refuses semi-planar float); no stages.  7 instances
template <class F>
inline void export_yuv_instance(int layout, int elem, F&& f) {
  export_pick<kElemU8, kElemU16, kElemF16, kElemBF16, kElemF32>(elem, [&](auto e) {
    if (layout == HMGPU_EXPORT_PLANAR) f(std::integral_constant<int, HMGPU_EXPORT_PLANAR>(), e);
    else if constexpr (decltype(e)::value <= kElemU16) {
      if (layout == HMGPU_EXPORT_SEMIPLANAR) f(std::integral_constant<int, HMGPU_EXPORT_SEMIPLANAR>(), e);
    }
  });
}

}  // namespace hmgpu
