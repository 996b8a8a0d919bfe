// fmt_core.h -- the chroma arithmetic of a conversion between chroma formats (include/hmgpu.h "format export"), once, for the two
// kernels that convert: k_export_fmt.hip, which writes Cb / Cr as planes or pairs, and k_export_yuvpack.hip, which interleaves them
// with the luma into words.  What stands here: the source rows of an output chroma row with their weights (fmt_rows), the combination
// of the rows of kFmtVert (fmt_vert) and the rows and columns of kFmtDown (fmt_down).  kFmtUp's arithmetic is chroma_core.h's
// chroma_line.  The loads stay with the kernels: k_export_fmt.hip fetches groups of four output pairs with whole-group loads, the
// packed kernel the pairs of one word unit.  All templates on the number of output pairs N.
#pragma once
#include "hmgpu_dev.h"
#include "chroma_core.h"

namespace hmgpu {

// the source rows (plane coordinates, clamped) of output chroma row Y (plane coordinates of the output format) and their weights in
// quarters, which sum to 4; a row without weight repeats the one before it
__device__ inline void fmt_rows(const FmtConv& f, int Y, int ri[3], int rw[3]) {
  if (f.vgain) {
    chroma_rows(f.cs, Y, 1, &ri[0], &ri[1], &rw[0]);
    rw[1] = 4 - rw[0]; rw[2] = 0;
  } else if (f.vloss) {
    for (int k = 0; k < 3; k++) { ri[k] = min(f.cs.hc - 1, max(0, 2 * Y + f.dv0 + k)); rw[k] = f.dv[k]; }
  } else {
    ri[0] = Y; rw[0] = 4; rw[1] = rw[2] = 0;
  }
  if (!rw[1]) ri[1] = ri[0];
  if (!rw[2]) ri[2] = ri[1];
}

// the row of output chroma row rc of a picture whose window starts at source chroma row y0: fmt_rows in plane coordinates
__device__ inline void fmt_rows_at(const FmtConv& f, int y0, int rc, int ri[3], int rw[3]) {
  fmt_rows(f, (f.vgain ? y0 << 1 : f.vloss ? y0 >> 1 : y0) + rc, ri, rw);
}

// kFmtVert: the N pairs of a group on the up to three rows that have a weight (p[k]: row k, 2N samples; a row without weight: zeros)
template <int N>
__device__ inline void fmt_vert(const int rw[3], const int (*p)[2 * N], int c[2 * N]) {
  for (int i = 0; i < 2 * N; i++) c[i] = (4 * (rw[0] * p[0][i] + rw[1] * p[1][i] + rw[2] * p[2][i]) + 8) >> 4;
}

// kFmtDown: N output pairs x .. x + N - 1 from the source pairs 2x - 1 .. 2x + 2N - 1 (p[k][0 ..]: row k; entries behind them are
// not read).  col0: the plane column of source pair 2x; the plane's first column has no left neighbour
template <int N, int M>
__device__ inline void fmt_down(const FmtConv& f, const int rw[3], const int (*p)[M], int col0, int c[2 * N]) {
  static_assert(M >= 4 * N + 2, "source pairs of the group");
  int v[M];
  for (int i = 0; i < M; i++) v[i] = rw[0] * p[0][i] + rw[1] * p[1][i] + rw[2] * p[2][i];
  if (col0 == 0) { v[0] = v[2]; v[1] = v[3]; }
  for (int j = 0; j < N; j++)
    for (int e = 0; e < 2; e++)
      c[2 * j + e] = (f.dh[0] * v[4 * j + e] + f.dh[1] * v[4 * j + 2 + e] + f.dh[2] * v[4 * j + 4 + e] + 8) >> 4;
}

}  // namespace hmgpu
