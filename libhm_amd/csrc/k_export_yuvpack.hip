// k_export_yuvpack.hip -- YUV interleaved into words: UYVY, YUY2, Y210, Y216, v210, AYUV, Y410, Y416 (hmgpu_pictures_export_yuvpack,
// include/hmgpu.h "packed YUV").  The values are those of the planar format export at the words' chroma format (4:2:2 or 4:4:4) and
// depth; this kernel adds no arithmetic to them, it places them.  k_export_fmt's shape: memory-bound, rows along the grid's y, the
// pictures of a batch along z with their own origin and mirror flag, no LDS.  One lane owns the source samples of one 16-byte unit
// of an output row -- eight pixels of UYVY / YUY2, four of Y210 / Y216 / AYUV / Y410, two of Y416, one group of six of v210 (eight
// lanes write one 128-byte line of 48 pixels) -- and forms
//   Y      by the depth rule of export_core.h from the luma of its pixels,
//   Cb, Cr for its own output row by the class of the conversion, whose rows and arithmetic are fmt_core.h's and chroma_core.h's, the
//          ones k_export_fmt.hip runs: kFmtConst, kFmtVert (also the words' own format: one row of weight 4), kFmtUp, kFmtDown.
// A unit starts on an even pixel but on no multiple of four pairs (v210: pair 3g), and under a mirror it starts where the row's width
// puts it, so the loads are the 4-byte ones that need no more than that: two luma samples, or a CbCr pair (chroma_pair).  A wave's
// lanes read adjacent addresses, every address is known before the first load is consumed, rows are clamped before the loads
// (uniform per workgroup) and columns behind them, as selects (chroma_line, fmt_down; the plane's first column, which a mirrored
// ragged unit can hold in its middle, by a clamp of the tap's column).  The mirror reverses pixels: the lane of output
// pixels X .. X + n - 1 reads source pixels w - X - n .. w - X - 1 and reverses them, so that the pair (Y0, Y1) of a 4:2:2 unit
// swaps with the unit and a v210 group is built from the mirrored row.  The furthest a lane reaches beyond its window: 7 luma samples
// or pairs to either side (the ragged last unit; under a mirror it is the row's first source samples that have no pixel), kFmtDown 15
// pairs to the right; the planes keep 128 samples of margin (128 >> csx pairs) on both sides.
// The store: one 16-byte store where the unit is whole and its address 16-byte aligned; else dwords, 2-byte or single elements under
// the unit's byte count, by the alignment of the address.  A v210 group is always whole: values at or beyond the width are 0.
#include "hmgpu_dev.h"
#include "export_core.h"
#include "fmt_core.h"

namespace hmgpu {

namespace {

template <int FAM> constexpr int pack_pixels() { return FAM == kPack422x8 ? 8 : FAM == kPackV210 ? 6 : FAM == kPackY416 ? 2 : 4; }
template <int FAM> constexpr bool pack_422() { return FAM <= kPackV210; }
// the classes a family is reached by: the horizontal axis gains towards 4:4:4 only and loses towards 4:2:2 only
template <int FAM, int CLS> constexpr bool pack_reached() { return CLS == kFmtConst || CLS == kFmtVert || (CLS == kFmtUp) != pack_422<FAM>(); }

// NP output CbCr pairs j0 .. j0 + NP - 1 (window coordinates of the output format, source order) of output row r, at the coding depth
template <int CLS, int NP>
__device__ inline void pack_chroma(const ExportArgs& a, const FmtConv& f, int pic, int r, int j0, int c[2 * NP]) {
  const int16_t* const ac = a.c[pic];
  const int x0 = f.cs.x0[pic], y0 = f.cs.y0[pic];
  int ri[3], rw[3];
  fmt_rows_at(f, y0, r, ri, rw);
  // A mirrored ragged unit starts left of its window, and of the plane where the window starts there: the plane's first column is
  // then inside the unit, not at its start where chroma_line and fmt_down replace the missing neighbour.  The taps' columns are
  // therefore clamped to the plane's first one behind the address arithmetic (lo: that column in window coordinates).
  const int lo = -x0;
  if constexpr (CLS == kFmtUp) {
    // source pairs J - 1 .. J + H of two rows (J = the pair of output pair j0, which is even): export_chroma_sited's fetch, pair by pair
    constexpr int H = NP / 2;
    const int16_t* const pa = ac + (ptrdiff_t)(ri[0] - y0) * a.pitch_c + kCStep * (j0 >> 1);
    const int16_t* const pb = ac + (ptrdiff_t)(ri[1] - y0) * a.pitch_c + kCStep * (j0 >> 1);
    int ua[H + 2], ub[H + 2], va[H + 2], vb[H + 2], u[NP], v[NP];
    for (int i = 0; i < H + 2; i++) {
      const int col = max((j0 >> 1) + i - 1, lo) - (j0 >> 1);
      chroma_pair(pa + col * kCStep, &ua[i], &va[i]);
      chroma_pair(pb + col * kCStep, &ub[i], &vb[i]);
    }
    chroma_line<H>(f.cs, x0 + (j0 >> 1), rw[0], ua, ub, u);
    chroma_line<H>(f.cs, x0 + (j0 >> 1), rw[0], va, vb, v);
    for (int i = 0; i < NP; i++) { c[2 * i] = u[i]; c[2 * i + 1] = v[i]; }
  } else if constexpr (CLS == kFmtVert) {
    int p[3][2 * NP];
    for (int k = 0; k < 3; k++) {
      for (int i = 0; i < 2 * NP; i++) p[k][i] = 0;
      if (rw[k]) {
        const int16_t* cp = ac + (ptrdiff_t)(ri[k] - y0) * a.pitch_c + kCStep * j0;
        for (int i = 0; i < NP; i++) chroma_pair(cp + i * kCStep, &p[k][2 * i], &p[k][2 * i + 1]);
      }
    }
    fmt_vert<NP>(rw, p, c);
  } else {
    // kFmtDown: source pairs 2 j0 - 1 .. 2 j0 + 2 NP - 1 on every row that has a weight
    constexpr int M = 4 * NP + 2;
    int p[3][M];
    for (int k = 0; k < 3; k++) {
      for (int i = 0; i < M; i++) p[k][i] = 0;
      if (rw[k]) {
        const int16_t* cp = ac + (ptrdiff_t)(ri[k] - y0) * a.pitch_c;
        for (int i = 0; i < M / 2; i++) chroma_pair(cp + max(2 * j0 - 1 + i, lo) * kCStep, &p[k][2 * i], &p[k][2 * i + 1]);
      }
    }
    fmt_down<NP>(f, rw, p, x0 + 2 * j0, c);
  }
}

// the unit's four dwords q, `bytes` of them (a multiple of 4) to be written at d
template <int ES>
__device__ inline void pack_store(uint8_t* d, const uint32_t q[4], int bytes) {
  const uintptr_t ad = (uintptr_t)d;
  if (bytes == 16 && !(ad & 15)) {
    u32x4 w; w.x = q[0]; w.y = q[1]; w.z = q[2]; w.w = q[3];
    stg4(d, w);
  } else if (ES == 4 || !(ad & 3)) {
    for (int k = 0; k < 4; k++) if (4 * k < bytes) stg(reinterpret_cast<uint32_t*>(d) + k, q[k]);
  } else if (ES == 2 || !(ad & 1)) {
    for (int k = 0; k < 8; k++) if (2 * k < bytes) stg(reinterpret_cast<uint16_t*>(d) + k, (uint16_t)(q[k >> 1] >> (16 * (k & 1))));
  } else {
    for (int k = 0; k < 16; k++) if (k < bytes) stg(d + k, (uint8_t)(q[k >> 2] >> (8 * (k & 3))));
  }
}

}  // namespace

template <int FAM, int CLS>
__global__ void __launch_bounds__(256) k_export_yuvpack(const ExportArgs a, const FmtConv f, const YuvPackArgs pk) {
  constexpr int NPX = pack_pixels<FAM>(), NP = pack_422<FAM>() ? NPX / 2 : NPX;
  const int unit = blockIdx.x * 256 + threadIdx.x, X = unit * NPX;
  const int r = blockIdx.y, pic = blockIdx.z;
  if (X >= a.w) return;
  const bool flip = (a.flip >> pic) & 1;
  const int n = min(NPX, a.w - X);                             // the unit's pixels inside the row
  const int xs = flip ? a.w - X - NPX : X;                     // its first source pixel; a ragged mirrored unit starts left of the window
  // ---- loads: luma, then the chroma of the class
  int yv[NPX], c[2 * NP];
  const int16_t* const yp = a.y[pic] + (ptrdiff_t)r * a.pitch_y + xs;
  if constexpr (pack_422<FAM>()) {                             // (xs is even, and so is the window's left edge: whole 4:2:2 samples)
    for (int i = 0; i < NPX / 2; i++) chroma_pair(yp + 2 * i, &yv[2 * i], &yv[2 * i + 1]);
  } else {
    for (int i = 0; i < NPX; i++) yv[i] = ldg(yp + i);
  }
  if constexpr (CLS == kFmtConst) {
    for (int i = 0; i < 2 * NP; i++) c[i] = f.constant;
  } else {
    pack_chroma<CLS, NP>(a, f, pic, r, pack_422<FAM>() ? xs >> 1 : xs, c);
    const int sc = a.sh[1], mc = a.maxv[1];
    for (int i = 0; i < 2 * NP; i++) c[i] = depth_conv(c[i], sc, mc);
  }
  // ---- output order: the mirror reverses the unit's pixels and pairs; v210's values beyond the width are 0
  uint32_t Y[NPX], Cb[NP], Cr[NP];
  const int sl = a.sh[0], ml = a.maxv[0];
  for (int i = 0; i < NPX; i++) Y[i] = (uint32_t)depth_conv(flip ? yv[NPX - 1 - i] : yv[i], sl, ml);
  for (int i = 0; i < NP; i++) { Cb[i] = (uint32_t)(flip ? c[2 * (NP - 1 - i)] : c[2 * i]); Cr[i] = (uint32_t)(flip ? c[2 * (NP - 1 - i) + 1] : c[2 * i + 1]); }
  // ---- the words
  uint32_t q[4];
  int bytes;
  if constexpr (FAM == kPack422x8) {
    const int sy = pk.yfirst ? 0 : 8, scx = pk.yfirst ? 8 : 0;
    for (int i = 0; i < 4; i++) q[i] = (Y[2 * i] | Y[2 * i + 1] << 16) << sy | (Cb[i] | Cr[i] << 16) << scx;
    bytes = 2 * n;
  } else if constexpr (FAM == kPack422x16) {
    const int s = pk.shift;
    for (int i = 0; i < 2; i++) { q[2 * i] = (Y[2 * i] | Cb[i] << 16) << s; q[2 * i + 1] = (Y[2 * i + 1] | Cr[i] << 16) << s; }
    bytes = 4 * n;
  } else if constexpr (FAM == kPackV210) {
    for (int i = 0; i < NPX; i++) if (i >= n) Y[i] = 0;
    for (int i = 0; i < NP; i++) if (2 * i >= n) Cb[i] = Cr[i] = 0;
    q[0] = Cb[0] | Y[0] << 10 | Cr[0] << 20;
    q[1] = Y[1] | Cb[1] << 10 | Y[2] << 20;
    q[2] = Cr[1] | Y[3] << 10 | Cb[2] << 20;
    q[3] = Y[4] | Cr[2] << 10 | Y[5] << 20;
    bytes = 16;
  } else if constexpr (FAM == kPackAYUV) {
    for (int i = 0; i < 4; i++) q[i] = Cr[i] | Cb[i] << 8 | Y[i] << 16 | pk.alpha << 24;
    bytes = 4 * n;
  } else if constexpr (FAM == kPackY410) {
    for (int i = 0; i < 4; i++) q[i] = Cb[i] | Y[i] << 10 | Cr[i] << 20 | pk.alpha << 30;
    bytes = 4 * n;
  } else {
    for (int i = 0; i < 2; i++) { q[2 * i] = Cb[i] | Y[i] << 16; q[2 * i + 1] = Cr[i] | pk.alpha << 16; }
    bytes = 8 * n;
  }
  uint8_t* const d = a.dst[0] + pic * a.bstride[0] + r * a.pitch[0] + (ptrdiff_t)unit * 16;
  pack_store<(FAM == kPack422x8 || FAM == kPackAYUV) ? 1 : (FAM == kPack422x16 || FAM == kPackY416) ? 2 : 4>(d, q, bytes);
}

void launch_export_yuvpack(const ExportArgs& a, const FmtConv& f, const YuvPackArgs& p, hipStream_t s) {
  export_pick<kPack422x8, kPack422x16, kPackV210, kPackAYUV, kPackY410, kPackY416>(p.fam, [&](auto fam) {
    constexpr int NPX = pack_pixels<fam()>();
    const int units = (a.w + NPX - 1) / NPX;
    const dim3 grid((unsigned)((units + 255) / 256), (unsigned)a.h, (unsigned)a.n), block(256);
    export_pick<kFmtConst, kFmtUp, kFmtVert, kFmtDown>(f.cls, [&](auto k) {
      if constexpr (pack_reached<fam(), k()>()) hipLaunchKernelGGL((k_export_yuvpack<fam(), k()>), grid, block, 0, s, a, f, p);
    });
  });
}

}  // namespace hmgpu
