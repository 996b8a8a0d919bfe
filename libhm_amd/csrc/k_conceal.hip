// k_conceal.hip -- error concealment: the CTUs a damaged stream did not deliver are filled from another picture of the context, or with
// a constant (hmgpu_pictures_conceal, include/hmgpu.h "error concealment").
//   work item   (picture, CTU, plane): blockIdx.z / .x / .y; plane 0 is luma, plane 1 the one chroma plane in which Cb and Cr alternate
//               (kCStep).  A workgroup whose CTU is not in the picture's mask leaves at once -- the test is one scalar load.
//   a lane      16 bytes of one row at a time: 8 luma samples, or 4 (Cb, Cr) pairs.  Either way the piece lies inside ONE 8x8 luma
//               block (4:2:0 and 4:2:2: 4 pairs = 8 luma columns; 4:4:4: 4 pairs = 4 luma columns, aligned to 4), so it has one
//               displacement.
//   COPY        the co-located piece: one 16-byte load, one 16-byte store.
//   MOTION      the vector of the 4x4 block at the 8x8 block's top-left corner, list 0 before list 1, by the `used` rule of the motion
//               export (slice-type term included: list 1 of a picture without B slices is never loaded), scaled by POC distance with
//               the integers of H.265 8.5.3.2.7 and rounded to whole luma samples.  A displaced piece that lies inside the plane is one
//               16-byte load (at 2- or 4-byte alignment); one that crosses a border is gathered element by element with clamped
//               coordinates.  Margins are never read.
//   fill        no source: a constant per component.
// Only samples inside width x height are written: partial CTUs at the right and bottom end at the picture.  No LDS, no scratch.
#include "hmgpu_dev.h"

namespace hmgpu {

namespace {

typedef uint32_t u32x4_a2 __attribute__((ext_vector_type(4), aligned(2)));

// the displacement of the 8x8 luma block whose top-left 4x4 block is partition z of CTU `ctu`, in whole luma samples
__device__ inline void block_disp(const ConcealPic& j, const ConcealArgs& a, int ctu, int z, int* dx, int* dy) {
  *dx = 0; *dy = 0;
  if (!j.side) return;
  const size_t p = (size_t)ctu * a.parts + z;
  if (ldg(j.part_size + p) == HMGPU_SIZE_NONE || ldg(j.pred_mode + p) != HMGPU_MODE_INTER) return;
  const SliceDev* sl = j.slices + min((int)ldg(j.slice_idx + ctu), HMGPU_MAX_SLICES - 1);
  const int st = ldg(&sl->slice_type);
  uint32_t mv = 0;
  int poc = 0;
  bool have = false;
#pragma unroll
  for (int l = 0; l < 2; l++) {
    const bool on = st == HMGPU_B_SLICE || (l == 0 && st == HMGPU_P_SLICE);
    if (have || !on) continue;
    const int ref = ldg(j.ref_idx[l] + p);
    if (ref < 0) continue;
    mv = ldg(reinterpret_cast<const uint32_t*>(j.mv[l] + 2 * p));
    poc = ldg(&sl->ref_poc[l][ref & (HMGPU_MAX_REF - 1)]);
    have = true;
  }
  if (!have) return;
  const long long dd = (long long)j.src_poc - poc, db = (long long)j.dst_poc - j.src_poc;
  const int td = (int)min(127ll, max(-128ll, dd)), tb = (int)min(127ll, max(-128ll, db));
  if (td == 0) return;
  const int tx = (16384 + (abs(td) >> 1)) / td;
  const int ds = clip3(-4096, 4095, (tb * tx + 32) >> 6);
  int v[2];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int m = ds * (int)(int16_t)(mv >> (16 * k));
    const int r = (abs(m) + 127) >> 8;
    v[k] = clip3(-32768, 32767, m < 0 ? -r : r);
  }
  *dx = (v[0] + 2) >> 2; *dy = (v[1] + 2) >> 2;
}

// one plane of one CTU; E = int16 elements per position (1 luma sample, kCStep: the Cb, Cr pair), sx / sy: the plane's subsampling
template <int E>
__device__ inline void conceal_plane(const ConcealPic& j, const ConcealArgs& a, int ctu, int16_t* dpl, const int16_t* spl, int pitch,
                                     int sx, int sy, uint32_t fill) {
  constexpr int VP = 8 / E;                                    // positions per 16 bytes
  const int Wp = a.width >> sx, Hp = a.height >> sy;
  const int cx = ctu % a.ctus_w, cy = ctu / a.ctus_w;
  const int px_lo = (cx << a.log2ctu) >> sx, py_lo = (cy << a.log2ctu) >> sy;
  const int ph = min((1 << a.log2ctu) >> sy, Hp - py_lo);      // rows of the CTU inside the picture
  const int lv = a.log2ctu - sx - (E == 1 ? 3 : 2);            // log2 pieces per row of the CTU
  const int nvec = ph << lv;
  const bool motion = j.mode == HMGPU_CONCEAL_MOTION;
  for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
    const int y = py_lo + (v >> lv), px = px_lo + (v & ((1 << lv) - 1)) * VP;
    if (px >= Wp) continue;
    const int n = min(VP, Wp - px);
    u32x4 o;
    if (!spl) {
      o = (u32x4){fill, fill, fill, fill};
    } else {
      int dx = 0, dy = 0;
      if (motion) {
        const int m = (1 << (a.log2ctu - 2)) - 1;
        const int bx = (((px << sx) >> 3) << 1) & m, by = (((y << sy) >> 3) << 1) & m;
        block_disp(j, a, ctu, spread4(bx) | (spread4(by) << 1), &dx, &dy);
        dx >>= sx; dy >>= sy;
      }
      // (a vector of 32767 quarter samples is 8192 samples: the sums stay far inside an int)
      const int16_t* row = spl + (ptrdiff_t)clip3(0, Hp - 1, y + dy) * pitch;
      const int x0 = px + dx;
      if (x0 >= 0 && x0 + VP <= Wp) {
        if ((x0 & (VP - 1)) == 0) o = ldg4(row + E * x0);
        else if constexpr (E == 1) o = *(const u32x4_a2 HMGPU_AS1*)(row + x0);
        else o = *(const u32x4_a4 HMGPU_AS1*)(row + E * x0);
      } else {
        uint32_t t[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
          if constexpr (E == 1) {
            const uint32_t lo = ldg(reinterpret_cast<const uint16_t*>(row) + clip3(0, Wp - 1, x0 + 2 * i));
            const uint32_t hi = ldg(reinterpret_cast<const uint16_t*>(row) + clip3(0, Wp - 1, x0 + 2 * i + 1));
            t[i] = lo | (hi << 16);
          } else {
            t[i] = ldg(reinterpret_cast<const uint32_t*>(row + E * clip3(0, Wp - 1, x0 + i)));
          }
        }
        o = (u32x4){t[0], t[1], t[2], t[3]};
      }
    }
    int16_t* d = dpl + (ptrdiff_t)y * pitch + E * px;
    if (n == VP) { stg4(d, o); continue; }
    const uint32_t t[4] = {o.x, o.y, o.z, o.w};                // the picture ends inside the piece
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if constexpr (E == 1) {
        if (2 * i < n) stg(reinterpret_cast<uint16_t*>(d) + 2 * i, (uint16_t)t[i]);
        if (2 * i + 1 < n) stg(reinterpret_cast<uint16_t*>(d) + 2 * i + 1, (uint16_t)(t[i] >> 16));
      } else if (i < n) {
        stg(reinterpret_cast<uint32_t*>(d) + i, t[i]);
      }
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_conceal(const ConcealArgs a) {
  const int ctu = blockIdx.x;
  const ConcealPic& j = a.pic[blockIdx.z];
  if (!((ldg(j.mask + (ctu >> 3)) >> (ctu & 7)) & 1)) return;
  if (blockIdx.y == 0) conceal_plane<1>(j, a, ctu, j.dst_y, j.src_y, a.pitch_y, 0, 0, j.fill_y);
  else conceal_plane<kCStep>(j, a, ctu, j.dst_c, j.src_c, a.pitch_c, a.csx, a.csy, j.fill_c);
}

void launch_conceal(const ConcealArgs& a, hipStream_t s) {
  const int pieces = (1 << (2 * a.log2ctu)) / 8;               // of a whole luma CTU: 32 .. 512
  const dim3 grid((unsigned)a.num_ctus, a.mono ? 1u : 2u, (unsigned)a.n), block((unsigned)min(256, max(64, pieces)));
  hipLaunchKernelGGL(k_conceal, grid, block, 0, s, a);
}

}  // namespace hmgpu
