// chroma_core.h -- the chroma stage of the RGB exports (hmgpu_pictures_export_chroma, include/hmgpu.h "chroma export"): Cb and Cr
// linearly interpolated to the luma grid at the signalled chroma sample location, before the matrix: the arithmetic of the stage.  The fetch
// that feeds it is export_core.h's export_chroma_sited (k_export.hip, k_export_fmt.hip's kFmtUp); k_export_scale.hip keeps its own 8-sample
// text of that fetch, and k_export_warp.hip's tap gathers its 2 x 2 pairs itself with these rows and weights.  Integer arithmetic, exact: two taps per axis with weights in quarters,
//   c' = (sum over the 2x2 taps of wx * wy * C[iy][ix] + 8) >> 4
// The two rows are combined first (a lane's rows are the same for all its columns), then the columns; the sum is the same integer.
// Tap indices are clamped to the decoded plane: the rows as indices before the loads (a row index is uniform per workgroup in the
// unscaled kernels), the columns as selects behind them, so that the loads stay whole groups: a column left of sample 0 or right of
// the last one is read from the plane's margin (memory of the plane, of any content) and replaced by the edge sample before it is
// used.  Only subsampled-horizontally formats come here (4:2:0, 4:2:2): the host runs the instances without the stage for 4:4:4 and
// 4:0:0, where it is the identity.
#pragma once
#include "hmgpu_dev.h"

namespace hmgpu {

// the two chroma rows of luma row y (plane coordinates) and the weight of the first; the second has 4 - w
__device__ inline void chroma_rows(const ChromaSite& s, int y, int csy, int* ia, int* ib, int* w) {
  const int par = y & csy, j = (y >> csy) + s.vy[par][0];
  *ia = min(s.hc - 1, max(0, j));
  *ib = min(s.hc - 1, max(0, j + 1));
  *w = s.vy[par][1];
}

// One component of the N + 2 chroma columns J - 1 .. J + N (plane coordinates), rows a and b already loaded with row a's weight w:
// the rows combined, the columns clamped to 0 .. wc - 1, then the 2N luma columns 2J .. 2J + 2N - 1 into out.
template <int N>
__device__ inline void chroma_line(const ChromaSite& s, int J, int w, const int a[N + 2], const int b[N + 2], int out[2 * N]) {
  int v[N + 2];
  for (int k = 0; k < N + 2; k++) v[k] = w * a[k] + (4 - w) * b[k];
  if (J == 0) v[0] = v[1];
  const int last = s.wc - 1 - J;                           // v[1 + last] is the plane's last column
  for (int k = 1; k <= N; k++) if (k > last) v[1 + k] = v[k];
  for (int k = 0; k < N; k++) {
    out[2 * k] = (s.hx[0][0] * v[k] + s.hx[0][1] * v[k + 1] + s.hx[0][2] * v[k + 2] + 8) >> 4;
    out[2 * k + 1] = (s.hx[1][0] * v[k] + s.hx[1][1] * v[k + 1] + s.hx[1][2] * v[k + 2] + 8) >> 4;
  }
}

// a CbCr pair as one 4-byte load
__device__ inline void chroma_pair(const int16_t* p, int* u, int* v) {
  const uint32_t w = ldg(reinterpret_cast<const uint32_t*>(p));
  *u = (int16_t)(w & 0xffff); *v = (int16_t)(w >> 16);
}

}  // namespace hmgpu
