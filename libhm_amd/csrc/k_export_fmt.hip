// k_export_fmt.hip -- the planar and semi-planar exports with Cb / Cr at a chroma format other than the picture's
// (hmgpu_pictures_export_format, include/hmgpu.h "format export"; TVideoIOYuv::writePlane with fileFormat != srcFormat,
// TVideoIOYuv.cpp:362-483, and its siting-aware linear forms).
// k_export's shape: memory-bound, one lane per 4 output samples of a row (luma) or 4 output CbCr pairs (chroma), rows along the
// grid's y -- the luma rows, then the chroma rows of the OUTPUT format --, the pictures of a batch along z with their own origin,
// alignment and mirror flag, no LDS.  Luma rows are k_export's, and kFmtUp's fetch is the RGB exports' sited chroma (export_core.h).  A chroma row reads the pair plane of the source
// format: its one to three source rows are chosen and clamped to the decoded plane before the loads (uniform per workgroup; a row
// without weight is not loaded), every load's address is known before the first load is consumed, and columns are clamped as selects
// behind whole-group loads (chroma_core.h's argument: a column outside the plane is read from the plane's margin, whatever it holds,
// and replaced by the edge sample before use).  The rows and the arithmetic of the classes are fmt_core.h's, shared with
// k_export_yuvpack.hip.  The furthest a lane reaches: one pair left of pair 0 (kFmtUp, kFmtDown) and, the
// last lane of a row, 5 pairs beyond the last source pair of the window (kFmtDown: pairs 2x .. 2x + 7 for x <= cw - 1) or 2 (the
// others); the pair planes keep 128 >> csx pairs of margin on both sides, 128 for the 4:4:4 planes kFmtDown reads.
// One instance per layout, output element and class (FmtConv), so nothing per sample branches on the format or the filter: REPLICATE
// and DROP are the same instances with a single weight 4 per axis, which the rounding returns exactly.
#include "hmgpu_dev.h"
#include "export_core.h"
#include "fmt_core.h"

namespace hmgpu {

template <int LAYOUT, int ELEM, int CLS>
__global__ void __launch_bounds__(256) k_export_fmt(const ExportArgs a, const FmtConv f) {
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int r = blockIdx.y, pic = blockIdx.z;
  const bool vec = (a.vec >> pic) & 1, flip = (a.flip >> pic) & 1;
  uint8_t* const d0 = a.dst[0] + pic * a.bstride[0];
  uint8_t* const d1 = a.dst[1] + pic * a.bstride[1];
  uint8_t* const d2 = a.dst[2] + pic * a.bstride[2];
  if (r < a.h) {
    if (x >= a.w) return;
    int yv[4];
    load4(a.y[pic] + (ptrdiff_t)r * a.pitch_y + x, vec, yv);
    export_luma_row<ELEM>(a, d0, r, x, min(4, a.w - x), yv, vec, flip);
    return;
  }
  // a chroma row of the output format: four CbCr pairs per lane
  const int rc = r - a.h;
  if (x >= a.cw) return;
  const int n = min(4, a.cw - x);
  uint32_t o[8];
  if constexpr (CLS == kFmtConst) {
    for (int i = 0; i < 8; i++) o[i] = (uint32_t)f.constant;
  } else {
    const int16_t* const ac = a.c[pic];
    const int x0 = f.cs.x0[pic], y0 = f.cs.y0[pic];
    int ri[3], rw[3];
    fmt_rows_at(f, y0, rc, ri, rw);
    int c[8];
    if constexpr (CLS == kFmtUp) {
      // source pairs J - 1 .. J + 2 (J = the pair of output pair x) of two rows: the sited fetch of four luma samples
      int u[4], v[4];
      export_chroma_sited<4>(f.cs, ac + (ptrdiff_t)(ri[0] - y0) * a.pitch_c + kCStep * (x >> 1), ac + (ptrdiff_t)(ri[1] - y0) * a.pitch_c + kCStep * (x >> 1),
                             x0 + (x >> 1), rw[0], vec, u, v);
      for (int i = 0; i < 4; i++) { c[2 * i] = u[i]; c[2 * i + 1] = v[i]; }
    } else if constexpr (CLS == kFmtVert) {
      // the group's own four pairs on every row that has a weight
      int p[3][8];
      for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 8; i++) p[k][i] = 0;
        if (rw[k]) {
          const int16_t* cp = ac + (ptrdiff_t)(ri[k] - y0) * a.pitch_c + kCStep * x;
          load8(cp, vec, p[k]);
        }
      }
      fmt_vert<4>(rw, p, c);
    } else {
      // kFmtDown: source pairs 2x - 1 .. 2x + 7 on every row that has a weight
      int p[3][18];
      for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 18; i++) p[k][i] = 0;
        if (rw[k]) {
          const int16_t* cp = ac + (ptrdiff_t)(ri[k] - y0) * a.pitch_c + kCStep * 2 * x;
          load8(cp, vec, p[k] + 2);
          load8(cp + 8, vec, p[k] + 10);
          chroma_pair(cp - kCStep, &p[k][0], &p[k][1]);
        }
      }
      fmt_down<4>(f, rw, p, x0 + 2 * x, c);
    }
    for (int i = 0; i < 8; i++) o[i] = (uint32_t)depth_conv(c[i], a.sh[1], a.maxv[1]);
  }
  export_chroma_out<LAYOUT, ELEM>(a, d1, d2, rc, x, n, o, vec, flip);
}

void launch_export_fmt(const ExportArgs& a, const FmtConv& f, hipStream_t s) {
  const int groups = (std::max(a.w, a.cw) + 3) / 4;
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)(a.h + a.ch), (unsigned)a.n), block(256);
  export_yuv_instance(a.layout, a.elem, [&](auto l, auto e) {
    export_pick<kFmtConst, kFmtUp, kFmtVert, kFmtDown>(f.cls, [&](auto k) { hipLaunchKernelGGL((k_export_fmt<l(), e(), k()>), grid, block, 0, s, a, f); });
  });
}

}  // namespace hmgpu
