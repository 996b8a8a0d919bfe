// k_export_px.hip -- finished pictures converted into packed pixels in caller-owned device memory (hmgpu_pictures_export_pixels,
// include/hmgpu.h "packed pixel export"): RGB / BGR (3 elements per pixel) and RGBA / BGRA / ARGB / ABGR (4), the elements those of
// the RGB layout of k_export.hip bit for bit.
// The load and convert side is k_export<HMGPU_EXPORT_RGB, ELEM>'s, restated here so that k_export.hip stays as it is: one lane per 4
// pixels of a row (8-byte loads per plane), rows along the grid's y, the pictures of a batch along z, no LDS.  The store side differs:
// the lane's 4 pixels are 12 .. 64 contiguous bytes, written as dword stores (hmgpu_dev.h export_store_px) where the group's first byte
// is dword aligned, so the lanes of a wave write one contiguous run (768 bytes for 1-byte RGB).  The alignment of the loads (the crop's left edge: ExportArgs::vec) and of the
// stores (the destination: PxOrder::vst, and the group's byte offset) are separate conditions.  One instance per output element and
// pixel size; the channel order is two launch-uniform flags applied with selects.  A second instance family runs the colour stage of
// colour_core.h between the clip and the store (hmgpu_pictures_export_colour), a third the chroma stage of chroma_core.h in place of
// the replicated chroma (hmgpu_pictures_export_chroma), with or without the colour stage.
#include "hmgpu_dev.h"
#include "colour_core.h"
#include "chroma_core.h"

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

}  // namespace

// X: nothing, or the stages as k_export takes them, each an instance family of its own -- a ColourLut: the colour stage
// (colour_core.h) between the clip and the store (launch_export_px_colour); a ChromaSite, before it: the chroma stage (chroma_core.h)
// in place of the replicated chroma (launch_export_px_chroma)
template <int ELEM, int NCH, class... X>
__global__ void __launch_bounds__(256) k_export_px(const ExportArgs a, const PxOrder po, const X... st) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int r = blockIdx.y, pic = blockIdx.z;
  if (x >= a.w) return;
  const bool vld = (a.vec >> pic) & 1, flip = (a.flip >> pic) & 1;
  const int n = min(4, a.w - x);
  int yv[4], u[4], v[4];
  load4(a.y[pic] + (ptrdiff_t)r * a.pitch_y + x, vld, yv);
  if constexpr (pack_has<ChromaSite, X...>) {
    // the chroma stage (csx = 1): pairs J - 1 .. J + 2 of two rows, six loads none of which waits for another
    const ChromaSite& cs = pack_get<ChromaSite>(st...);
    const int x0 = cs.x0[pic], y0 = cs.y0[pic];
    int ia, ib, wv;
    chroma_rows(cs, (y0 << a.csy) + r, a.csy, &ia, &ib, &wv);
    const int16_t* pa = a.c[pic] + (ptrdiff_t)(ia - y0) * a.pitch_c + kCStep * (x >> 1);
    const int16_t* pb = a.c[pic] + (ptrdiff_t)(ib - y0) * a.pitch_c + kCStep * (x >> 1);
    int ma[4], mb[4], ua[4], ub[4], va[4], vb[4];
    load4(pa, vld, ma);
    load4(pb, vld, mb);
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
    const int16_t* cp = a.c[pic] + (ptrdiff_t)(r >> a.csy) * a.pitch_c + kCStep * (x >> a.csx);
    int p[8];
    load4(cp, vld, p);
    if (a.csx) {
      u[0] = u[1] = p[0]; v[0] = v[1] = p[1]; u[2] = u[3] = p[2]; v[2] = v[3] = p[3];
    } else {
      load4(cp + 4, vld, p + 4);
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
  export_store_px<ELEM, NCH>(a.dst[0] + pic * a.bstride[0] + r * a.pitch[0], x, a.w, R, G, B, n, po.vst != 0, flip, mc, a.msb[0],
                             a.scale, a.bias, po);
}

void launch_export_px_chroma(const ExportArgs& a, const PxOrder& po, const ChromaSite& cs, const ColourLut* lut, int nch, hipStream_t s) {
  const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_PX_CHROMA_CASE(E, N) \
  if (a.elem == E && nch == N && !lut) hipLaunchKernelGGL((k_export_px<E, N, ChromaSite>), grid, block, 0, s, a, po, cs); \
  if (a.elem == E && nch == N && lut) hipLaunchKernelGGL((k_export_px<E, N, ChromaSite, ColourLut>), grid, block, 0, s, a, po, cs, *lut);
#define HMGPU_EXPORT_PX_CHROMA_ELEM(E) HMGPU_EXPORT_PX_CHROMA_CASE(E, 3) HMGPU_EXPORT_PX_CHROMA_CASE(E, 4)
  HMGPU_EXPORT_PX_CHROMA_ELEM(kElemU8)
  HMGPU_EXPORT_PX_CHROMA_ELEM(kElemU16)
  HMGPU_EXPORT_PX_CHROMA_ELEM(kElemF16)
  HMGPU_EXPORT_PX_CHROMA_ELEM(kElemBF16)
  HMGPU_EXPORT_PX_CHROMA_ELEM(kElemF32)
#undef HMGPU_EXPORT_PX_CHROMA_ELEM
#undef HMGPU_EXPORT_PX_CHROMA_CASE
}

void launch_export_px_colour(const ExportArgs& a, const PxOrder& po, const ColourLut& lut, int nch, hipStream_t s) {
  const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_PX_COLOUR_CASE(E) \
  if (a.elem == E && nch == 3) hipLaunchKernelGGL((k_export_px<E, 3, ColourLut>), grid, block, 0, s, a, po, lut); \
  if (a.elem == E && nch == 4) hipLaunchKernelGGL((k_export_px<E, 4, ColourLut>), grid, block, 0, s, a, po, lut);
  HMGPU_EXPORT_PX_COLOUR_CASE(kElemU8)
  HMGPU_EXPORT_PX_COLOUR_CASE(kElemU16)
  HMGPU_EXPORT_PX_COLOUR_CASE(kElemF16)
  HMGPU_EXPORT_PX_COLOUR_CASE(kElemBF16)
  HMGPU_EXPORT_PX_COLOUR_CASE(kElemF32)
#undef HMGPU_EXPORT_PX_COLOUR_CASE
}

void launch_export_px(const ExportArgs& a, const PxOrder& po, int nch, hipStream_t s) {
  const dim3 grid((unsigned)(((a.w + 3) / 4 + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
#define HMGPU_EXPORT_PX_CASE(E) \
  if (a.elem == E && nch == 3) hipLaunchKernelGGL((k_export_px<E, 3>), grid, block, 0, s, a, po); \
  if (a.elem == E && nch == 4) hipLaunchKernelGGL((k_export_px<E, 4>), grid, block, 0, s, a, po);
  HMGPU_EXPORT_PX_CASE(kElemU8)
  HMGPU_EXPORT_PX_CASE(kElemU16)
  HMGPU_EXPORT_PX_CASE(kElemF16)
  HMGPU_EXPORT_PX_CASE(kElemBF16)
  HMGPU_EXPORT_PX_CASE(kElemF32)
#undef HMGPU_EXPORT_PX_CASE
}

}  // namespace hmgpu
