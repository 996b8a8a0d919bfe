// k_export.hip -- finished pictures converted into caller-owned device memory (hmgpu_picture_export / hmgpu_pictures_export,
// include/hmgpu.h "device export", "batched tensor export", "packed pixel export").
//   PLANAR / SEMIPLANAR: TVideoIOYuv::write's bit-depth rule (TVideoIOYuv.cpp:70-87, 743-763; CLIP_TO_709_RANGE 0), per channel type
//   RGB: chroma replicated to the luma grid (writePlane's 4:2:2 -> 4:4:4, TVideoIOYuv.cpp:425-443), an integer Y'CbCr -> R'G'B' matrix
//        whose coefficients the host derives (hmgpu_export_plan.coef), or the identity (RGBtoGBR, TVideoIOYuv.cpp:962-978); as three
//        planes, or as packed pixels RGB / BGR (3 elements per pixel) and RGBA / BGRA / ARGB / ABGR (4), the same elements bit for bit
// Memory-bound, no reuse beyond chroma: one lane per 4 samples of a row (8-byte loads per plane, 4- or 8-byte stores), rows along
// the grid's y, the pictures of a batch along z (each with its own origin, alignment and mirror flag: hmgpu_pictures_export_windows),
// no LDS.  One instance per layout, output element (1- or 2-byte unsigned, float16, bfloat16, float32: hmgpu_dev.h export_store4)
// and, for RGB, pixel size and stages, so nothing per sample branches on any of them.  The source planes keep at least 128 samples of
// margin right of the picture, so the loads of the last group of a row never leave the allocation; only its stores are cut to the row.
// Packed pixels: a lane's 4 pixels are 12 .. 64 contiguous bytes, written as dword stores (hmgpu_dev.h export_store_px) where the
// group's first byte is dword aligned, so the lanes of a wave write one contiguous run (768 bytes for 1-byte RGB).  The alignment of
// the loads (the crop's left edge: ExportArgs::vec) and of the stores (the destination: PxOrder::vst, and the group's byte offset) are
// separate conditions; the channel order is two launch-uniform flags applied with selects.
// The chroma fetch, the conversion and the store step of the RGB layout are export_core.h's, shared with the scaled and warp kernels.
#include "hmgpu_dev.h"
#include "export_core.h"

namespace hmgpu {

// NCH (RGB): 0 = three planes, else the elements of a packed pixel.  X: nothing, or the stages of the RGB layout, each an instance
// family of its own -- a PxOrder where NCH is not 0; a ChromaSite: the chroma stage (chroma_core.h) in place of the replicated
// chroma; a ColourLut: the colour stage (colour_core.h) between the clip and the store.  The instances without them have the one
// argument and hold no trace of any
template <int LAYOUT, int ELEM, int NCH, class... X>
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
    // RGB: the chroma of the group's four luma samples, the conversion, the store
    int u[4], v[4];
    if constexpr (pack_has<ChromaSite, X...>) {
      const ChromaSite& cs = pack_get<ChromaSite>(st...);
      const int x0 = cs.x0[pic], y0 = cs.y0[pic];
      int ia, ib, wv;
      chroma_rows(cs, (y0 << a.csy) + r, a.csy, &ia, &ib, &wv);
      export_chroma_sited<4>(cs, ac + (ptrdiff_t)(ia - y0) * a.pitch_c + kCStep * (x >> 1), ac + (ptrdiff_t)(ib - y0) * a.pitch_c + kCStep * (x >> 1),
                             x0 + (x >> 1), wv, vec, u, v);
    } else {
      export_chroma_replicated<4>(a, ac, r, x, vec, u, v);
    }
    uint32_t R[4], G[4], B[4];
    export_rgb<4>(a, yv, u, v, R, G, B);
    if constexpr (NCH != 0) {
      const PxOrder& po = pack_get<PxOrder>(st...);
      export_store_rgb<ELEM, NCH>(a, po, pic, r, x, a.w, R, G, B, n, po.vst != 0, flip, export_mc(a), a.msb[0], st...);
    } else {
      export_store_rgb<ELEM, 0>(a, PxOrder{}, pic, r, x, a.w, R, G, B, n, vec, flip, export_mc(a), a.msb[0], st...);
    }
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

// po: null (planes; nch 0), or the channel order of packed pixels of nch elements; cs / lut: null, or the stage (RGB only)
void launch_export(const ExportArgs& a, const PxOrder* po, int nch, const ChromaSite* cs, const ColourLut* lut, hipStream_t s) {
  const bool rgb = a.layout == HMGPU_EXPORT_RGB;
  const int groups = (std::max(a.w, rgb ? 0 : a.cw) + 3) / 4;
  const int rows = a.h + (rgb || a.mono ? 0 : a.ch);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)rows, (unsigned)a.n), block(256);
  if (!rgb) {
    export_yuv_instance(a.layout, a.elem, [&](auto l, auto e) { hipLaunchKernelGGL((k_export<l(), e(), 0>), grid, block, 0, s, a); });
    return;
  }
  export_rgb_instance(a.elem, po ? nch : 0, cs, lut, [&](auto e, auto n, const auto&... st) {
    if constexpr (n() != 0) hipLaunchKernelGGL((k_export<HMGPU_EXPORT_RGB, e(), n(), PxOrder, std::decay_t<decltype(st)>...>), grid, block, 0, s, a, *po, st...);
    else hipLaunchKernelGGL((k_export<HMGPU_EXPORT_RGB, e(), 0, std::decay_t<decltype(st)>...>), grid, block, 0, s, a, st...);
  });
}

}  // namespace hmgpu
