// k_export.hip -- finished pictures converted into caller-owned device memory (hmgpu_picture_export / hmgpu_pictures_export,
// include/hmgpu.h "device export", "batched tensor export").
//   PLANAR / SEMIPLANAR: TVideoIOYuv::write's bit-depth rule (TVideoIOYuv.cpp:70-87, 743-763; CLIP_TO_709_RANGE 0), per channel type
//   RGB: chroma replicated to the luma grid (writePlane's 4:2:2 -> 4:4:4, TVideoIOYuv.cpp:425-443), an integer Y'CbCr -> R'G'B' matrix
//        whose coefficients the host derives (hmgpu_export_plan.coef), or the identity (RGBtoGBR, TVideoIOYuv.cpp:962-978)
// Memory-bound, no reuse beyond chroma: one lane per 4 samples of a row (8-byte loads per plane, 4- or 8-byte stores), rows along
// the grid's y, the pictures of a batch along z (each with its own origin, alignment and mirror flag: hmgpu_pictures_export_windows), no LDS.  One instance per layout and output element (1- or 2-byte unsigned, float16,
// bfloat16, float32: hmgpu_dev.h export_store4), so nothing per sample branches on either.  The source planes
// keep at least 128 samples of margin right of the picture, so the loads of the last group of a row never leave the allocation;
// only its stores are cut to the row.  The RGB layout has a second instance family with the colour stage of colour_core.h between the clip
// and the store (hmgpu_pictures_export_colour), and a third with the chroma stage of chroma_core.h in place of the replicated chroma
// (hmgpu_pictures_export_chroma), with or without the colour stage.
#include "hmgpu_dev.h"
#include "export_core.h"
#include "colour_core.h"
#include "chroma_core.h"

namespace hmgpu {

// X: nothing, or the stages of the RGB layout, each an instance family of its own -- a ColourLut: the colour stage (colour_core.h)
// between the clip and the store (launch_export_colour); a ChromaSite, before it: the chroma stage (chroma_core.h) in place of the
// replicated chroma (launch_export_chroma).  The instances without them have the one argument and hold no trace of either
template <int LAYOUT, int ELEM, class... X>
__global__ void __launch_bounds__(256) k_export(const ExportArgs a, const X... st) {
  constexpr int BYTES = elem_bytes<ELEM>();
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int r = blockIdx.y, pic = blockIdx.z;
  const bool vec = (a.vec >> pic) & 1, flip = (a.flip >> pic) & 1;
  const int16_t* const ay = a.y[pic];
  const int16_t* const ac = a.c[pic];
  uint8_t* const d0 = a.dst[0] + pic * a.bstride[0];
  uint8_t* const d1 = a.dst[1] + pic * a.bstride[1];
  uint8_t* const d2 = a.dst[2] + pic * a.bstride[2];
  if (LAYOUT == HMGPU_EXPORT_RGB || r < a.h) {
    if (x >= a.w) return;
    const int n = min(4, a.w - x);
    int yv[4];
    load4(ay + (ptrdiff_t)r * a.pitch_y + x, vec, yv);
    if (LAYOUT != HMGPU_EXPORT_RGB) {
      uint32_t o[4];
      for (int i = 0; i < 4; i++) o[i] = (uint32_t)depth_conv(yv[i], a.sh[0], a.maxv[0]);
      export_store_row<ELEM>(d0 + r * a.pitch[0], x, a.w, o, n, vec, flip, a.msb[0], a.scale[0], a.bias[0]);
      return;
    }
    // RGB: the chroma of the group's four luma samples (one pair for two of them when csx = 1)
    int u[4], v[4];
    if constexpr (pack_has<ChromaSite, X...>) {
      // the chroma stage (csx = 1): pairs J - 1 .. J + 2 of two rows, six loads none of which waits for another
      const ChromaSite& cs = pack_get<ChromaSite>(st...);
      const int x0 = cs.x0[pic], y0 = cs.y0[pic];
      int ia, ib, wv;
      chroma_rows(cs, (y0 << a.csy) + r, a.csy, &ia, &ib, &wv);
      const int16_t* pa = ac + (ptrdiff_t)(ia - y0) * a.pitch_c + kCStep * (x >> 1);
      const int16_t* pb = ac + (ptrdiff_t)(ib - y0) * a.pitch_c + kCStep * (x >> 1);
      int ma[4], mb[4], ua[4], ub[4], va[4], vb[4];
      load4(pa, vec, ma);
      load4(pb, vec, mb);
      chroma_pair(pa - kCStep, &ua[0], &va[0]);
      chroma_pair(pb - kCStep, &ub[0], &vb[0]);
      chroma_pair(pa + 2 * kCStep, &ua[3], &va[3]);
      chroma_pair(pb + 2 * kCStep, &ub[3], &vb[3]);
      ua[1] = ma[0]; va[1] = ma[1]; ua[2] = ma[2]; va[2] = ma[3];
      ub[1] = mb[0]; vb[1] = mb[1]; ub[2] = mb[2]; vb[2] = mb[3];
      chroma_line<2>(cs, x0 + (x >> 1), wv, ua, ub, u);
      chroma_line<2>(cs, x0 + (x >> 1), wv, va, vb, v);
    } else if (a.mono) {
      for (int i = 0; i < 4; i++) u[i] = v[i] = a.coef[3];
    } else {
      const int16_t* cp = ac + (ptrdiff_t)(r >> a.csy) * a.pitch_c + kCStep * (x >> a.csx);
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
        G[i] = (uint32_t)depth_conv(yv[i], a.sh[0], a.maxv[0]);
        B[i] = (uint32_t)depth_conv(u[i], a.sh[1], a.maxv[1]);
        R[i] = (uint32_t)depth_conv(v[i], a.sh[1], a.maxv[1]);
      }
    } else {
      const int S = a.coef[0], M = a.coef[9];
      for (int i = 0; i < 4; i++) {
        const int t = a.coef[4] * (yv[i] - a.coef[2]) + a.coef[1];
        const int cu = u[i] - a.coef[3], cv = v[i] - a.coef[3];
        R[i] = (uint32_t)min(M, max(0, (t + a.coef[5] * cv) >> S));
        G[i] = (uint32_t)min(M, max(0, (t + a.coef[6] * cu + a.coef[7] * cv) >> S));
        B[i] = (uint32_t)min(M, max(0, (t + a.coef[8] * cu) >> S));
      }
    }
    if constexpr (pack_has<ColourLut, X...>) colour_map4(pack_get<ColourLut>(st...), R, G, B);
    // (identity: G carries the luma container shift, B and R the chroma one; the matrix: all three the luma one)
    const int mc = a.coef[10] ? a.msb[1] : a.msb[0];
    export_store_row<ELEM>(d0 + r * a.pitch[0], x, a.w, R, n, vec, flip, mc, a.scale[0], a.bias[0]);
    export_store_row<ELEM>(d1 + r * a.pitch[1], x, a.w, G, n, vec, flip, a.msb[0], a.scale[1], a.bias[1]);
    export_store_row<ELEM>(d2 + r * a.pitch[2], x, a.w, B, n, vec, flip, mc, a.scale[2], a.bias[2]);
    return;
  }
  // chroma rows of the YUV layouts: four CbCr pairs per lane
  const int rc = r - a.h;
  if (x >= a.cw) return;
  const int n = min(4, a.cw - x);
  int p[8];
  const int16_t* cp = ac + (ptrdiff_t)rc * a.pitch_c + kCStep * x;
  load4(cp, vec, p);
  load4(cp + 4, vec, p + 4);
  uint32_t o[8];
  for (int i = 0; i < 8; i++) o[i] = (uint32_t)depth_conv(p[i], a.sh[1], a.maxv[1]);
  if (LAYOUT == HMGPU_EXPORT_PLANAR) {
    const uint32_t cb[4] = {o[0], o[2], o[4], o[6]}, cr[4] = {o[1], o[3], o[5], o[7]};
    export_store_row<ELEM>(d1 + rc * a.pitch[1], x, a.cw, cb, n, vec, flip, a.msb[1], a.scale[1], a.bias[1]);
    export_store_row<ELEM>(d2 + rc * a.pitch[2], x, a.cw, cr, n, vec, flip, a.msb[1], a.scale[2], a.bias[2]);
  } else {                                // the pairs as they lie: two groups of four samples
    export_store_pairs<ELEM>(d1 + rc * a.pitch[1], x, a.cw, o, n, vec, flip, a.msb[1]);
  }
}

void launch_export_chroma(const ExportArgs& a, const ChromaSite& cs, const ColourLut* lut, hipStream_t s) {
  const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_CHROMA_CASE(E) \
  if (a.elem == E && !lut) hipLaunchKernelGGL((k_export<HMGPU_EXPORT_RGB, E, ChromaSite>), grid, block, 0, s, a, cs); \
  if (a.elem == E && lut) hipLaunchKernelGGL((k_export<HMGPU_EXPORT_RGB, E, ChromaSite, ColourLut>), grid, block, 0, s, a, cs, *lut);
  HMGPU_EXPORT_CHROMA_CASE(kElemU8)
  HMGPU_EXPORT_CHROMA_CASE(kElemU16)
  HMGPU_EXPORT_CHROMA_CASE(kElemF16)
  HMGPU_EXPORT_CHROMA_CASE(kElemBF16)
  HMGPU_EXPORT_CHROMA_CASE(kElemF32)
#undef HMGPU_EXPORT_CHROMA_CASE
}

void launch_export_colour(const ExportArgs& a, const ColourLut& lut, hipStream_t s) {
  const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_COLOUR_CASE(E) \
  if (a.elem == E) hipLaunchKernelGGL((k_export<HMGPU_EXPORT_RGB, E, ColourLut>), grid, block, 0, s, a, lut);
  HMGPU_EXPORT_COLOUR_CASE(kElemU8)
  HMGPU_EXPORT_COLOUR_CASE(kElemU16)
  HMGPU_EXPORT_COLOUR_CASE(kElemF16)
  HMGPU_EXPORT_COLOUR_CASE(kElemBF16)
  HMGPU_EXPORT_COLOUR_CASE(kElemF32)
#undef HMGPU_EXPORT_COLOUR_CASE
}

void launch_export(const ExportArgs& a, hipStream_t s) {
  const int groups = (std::max(a.w, a.layout == HMGPU_EXPORT_RGB ? 0 : a.cw) + 3) / 4;
  const int rows = a.h + (a.layout == HMGPU_EXPORT_RGB || a.mono ? 0 : a.ch);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)rows, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_CASE(L, E) \
  if (a.layout == L && a.elem == E) hipLaunchKernelGGL((k_export<L, E>), grid, block, 0, s, a);
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR, kElemU8)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR, kElemU16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_SEMIPLANAR, kElemU8)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_SEMIPLANAR, kElemU16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB, kElemU8)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB, kElemU16)
  // float elements: the planar and RGB layouts (the host refuses semi-planar)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR, kElemF16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR, kElemBF16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_PLANAR, kElemF32)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB, kElemF16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB, kElemBF16)
  HMGPU_EXPORT_CASE(HMGPU_EXPORT_RGB, kElemF32)
#undef HMGPU_EXPORT_CASE
}

}  // namespace hmgpu
