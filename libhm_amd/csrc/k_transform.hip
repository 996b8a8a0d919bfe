// k_transform.hip -- the frequency-domain side of finished pictures written into caller-owned device memory
// (hmgpu_pictures_export_transform, include/hmgpu.h "transform export").
//   source: the levels as staged for the picture (PicDev::coef: HM's dense layout, or compact behind coef_start) and HM's per-partition
//           arrays, which say where a coded transform block lies, how large it is and with which QpParam it is de-quantised
//   planes: one element per component sample, element v * size + u of a block at (y0 + v, x0 + u): the level, or xDeQuant of it
//   info:   six int8 channels per 4x4 luma block (transform size, tr_idx, coded mask, flags, intra modes)
// Nothing here reads PicDev::tu[]: those lists belong to the last k_prep call, hold neither PCM CUs nor intra CUs without modes, and a
// picture built slice by slice keeps only its last call's.  Codedness comes from the arrays alone -- a dense level array holds stale
// values outside the current picture's coded blocks -- by the rule of hmgpu_pack_levels (hmgpu_input.hip), whose set the compact
// offsets have to reproduce exactly: both test the cbf chain through cbf_coded (hmgpu_dev.h).
//
// One 256-lane workgroup per CTU and component class (grid y: 0 luma and the info grid, 1 Cb + Cr), grid z the picture.
//   phase 1  lane z = partition z.  Its bytes go to LDS so that every lane can read the flags at the FIRST partition of the block that
//            covers it (a chroma block's flags sit there; 4:2:2: the lower square's half the block further on); from them the lane derives,
//            per component of the class, the covering block's origin, size, QpParam, flags and level offset and leaves them as an 8-byte
//            record.  Compact levels: the offset is the CTU's start plus the exclusive prefix sum, in z order, of the element counts of the
//            coded blocks that originate at a partition -- a wave scan joined through LDS.
//   phase 2  the lanes walk the CTU's rows in segments of eight samples (16 bytes of levels): eight lanes store 128 contiguous bytes of a
//            row.  A segment is two halves of four samples, each with the record of the partition above it; a half of a coded block loads
//            its 8 bytes of levels (both halves of a block of 8 or more: one 16-byte load), de-quantises in registers and the segment goes
//            out as one 16-byte store (two for float32), or element by element under a mask at the picture's right edge and for
//            destinations that are not aligned.
// Every element inside the picture is written exactly once: no atomics, no scratch, no zeroing launch.
#include "hmgpu_dev.h"
#include "quant_core.h"

namespace hmgpu {

namespace {

// the block of component c that covers partition z of a unit of 2^log2tu luma samples: zo its first partition, zf the partition its
// own flags are stored at (4:2:2: the lower square's are half the block on), log2n its size
struct Cover { int zo, zf, log2n, lower; };
__device__ inline Cover cover(int c, int z, int log2tu, int fmt) {
  const int tup = 1 << (2 * max(log2tu - 2, 0));
  Cover r;
  r.lower = 0;
  if (c == 0 || fmt == 3) { r.zo = z & ~(tup - 1); r.zf = r.zo; r.log2n = log2tu; return r; }
  const int bp = max(tup, 4);                       // the 4x4 chroma block under four 4x4 luma units belongs to the 8x8 node
  r.zo = z & ~(bp - 1); r.zf = r.zo; r.log2n = max(log2tu, 3) - 1;
  if (fmt == 2) { r.lower = (z - r.zo) >= (bp >> 1) ? 1 : 0; r.zf = r.zo + (r.lower ? bp >> 1 : 0); }
  return r;
}

// record word 1: bit 0 coded, 1-3 log2 size, 4-7 / 8-11 the block's origin in the CTU (x, y) in units of four component samples,
// 12-16 per, 17-19 rem, 20 transform skip, 21 cu_transquant_bypass, 22 intra CU
__device__ inline uint32_t rec_pack(bool coded, int log2n, int ox4, int oy4, int per, int rem, int ts, int byp, bool intra) {
  return (coded ? 1u : 0u) | ((uint32_t)log2n << 1) | ((uint32_t)ox4 << 4) | ((uint32_t)oy4 << 8) | ((uint32_t)per << 12) | ((uint32_t)rem << 17) |
         ((uint32_t)(ts & 1) << 20) | ((uint32_t)(byp ? 1 : 0) << 21) | ((intra ? 1u : 0u) << 22);
}

// TComTrQuant::xDeQuant of one level (TComTrQuant.cpp:1203-1311): m the list's factor at the position (lists), else flat scaling
__device__ inline int dequant1(int q, int f, int rs, int in_min, int in_max) {
  q = clip3(in_min, in_max, q);
  const int p = q * f;
  const int c = rs > 0 ? (p + (1 << (rs - 1))) >> rs : (int)((unsigned)p << (-rs));
  return clip3(-32768, 32767, c);
}

}  // namespace

template <int ELEM, bool COEFFS>
__global__ void __launch_bounds__(256) k_transform(const TransformArgs a) {
  __shared__ uint32_t s_flag[256];                  // partition z: cbf[0] | cbf[1] << 8 | cbf[2] << 16 | (transform_skip[c] & 1) << (24 + c)
  __shared__ u32x2 s_rec[2][256];                   // per component of the class: the record of the block that covers partition z
  __shared__ uint32_t s_start[2][256];              // compact levels: elements of the CTU's coded blocks before partition z
  __shared__ uint32_t s_wave[2][4];
  const int pic = blockIdx.z, ctu = blockIdx.x, cls = blockIdx.y;
  const TransformSrc& s = a.src[pic];
  const bool want_info = cls == 0 && a.dst[3] != nullptr;
  const int c_lo = cls ? 1 : 0, nk = cls ? 2 : 1;
  bool sel[2];
#pragma unroll
  for (int k = 0; k < 2; k++) sel[k] = k < nk && ((a.comps >> (c_lo + k)) & 1) && a.dst[c_lo + k] != nullptr;
  if (!want_info && !sel[0] && !sel[1]) return;
  const int z = threadIdx.x, parts = a.parts, log2ctu = a.log2ctu, pw = 1 << (log2ctu - 2);
  const bool active = z < parts;
  const bool flags = (s.gate & kTransFlags) != 0;
  const int ctu_x = ctu % a.ctus_w, ctu_y = ctu / a.ctus_w;
  // ---- phase 1a: the partition's bytes
  int ps = HMGPU_SIZE_NONE, pm = 0, dp = 0, tr = 0, byp = 0, pcm = 0;
  const size_t i0 = (size_t)ctu * parts + z;
  if (active) {
    ps = ldg(s.part_size + i0); pm = ldg(s.pred_mode + i0); dp = ldg(s.depth + i0); tr = ldg(s.tr_idx + i0);
    uint32_t f = (uint32_t)ldg(s.cbf[0] + i0) | ((uint32_t)ldg(s.cbf[1] + i0) << 8) | ((uint32_t)ldg(s.cbf[2] + i0) << 16);
    if (flags) {
#pragma unroll
      for (int c = 0; c < 3; c++) if (s.tskip[c]) f |= (uint32_t)(ldg(s.tskip[c] + i0) & 1) << (24 + c);
      byp = ldg(s.bypass + i0); pcm = ldg(s.ipcm + i0);
    }
    s_flag[z] = f;
  }
  __syncthreads();
  // ---- phase 1b: the covering block of every component
  const bool compact = s.coef_start[0] != nullptr;  // (4:2:0 / 4:0:0 only: stage_inputs)
  const int zx = zscan_x(z), zy = zscan_y(z);
  const int bx = ctu_x * pw + zx, by = ctu_y * pw + zy;            // the partition in the picture's grid of 4x4 luma blocks
  const bool inpic = active && bx * 4 < a.width && by * 4 < a.height;
  const bool decoded = active && ps != HMGPU_SIZE_NONE && dp <= log2ctu - 3;
  const int log2tu = decoded ? log2ctu - dp - (tr & 7) : 6;
  const bool sized = decoded && log2tu >= 2 && log2tu <= 5;
  const bool intra = pm == HMGPU_MODE_INTRA;
  uint32_t coded_mask = 0, ts_mask = 0;
  uint32_t cnt[2] = {0, 0};
  Cover cv[2] = {{0, 0, 2, 0}, {0, 0, 2, 0}};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c && a.mono) break;
    const Cover v = cover(c, z, clip3(2, 6, log2tu), a.fmt);
    const uint32_t fo = s_flag[v.zo], ff = s_flag[v.zf];
    bool coded = sized && cbf_coded((fo >> (8 * c)) & 0xffu, tr & 7);
    if (c && a.fmt == 2) coded = coded && ((ff >> (8 * c + (tr & 7) + 1)) & 1u);
    if (decoded) ts_mask |= ((ff >> (24 + c)) & 1u) << c;
    const int k = c - c_lo;
    if (k >= 0 && k < nk) {
      cv[k] = v;
      // the elements hmgpu_pack_levels emits for the block that starts here (PCM and intra CUs included)
      if (coded && inpic && z == v.zo) cnt[k] = 1u << (2 * v.log2n);
    }
    if (coded && !pcm) coded_mask |= 1u << c;
  }
  if (compact) {
    const int lane = z & 63, wave = z >> 6;
    uint32_t incl[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      incl[k] = cnt[k];
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(incl[k], d); if (lane >= d) incl[k] += o; }
      if (lane == 63) s_wave[k][wave] = incl[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; k++) {
      uint32_t before = 0;
#pragma unroll
      for (int w = 0; w < 3; w++) if (w < wave) before += s_wave[k][w];
      s_start[k][z] = before + incl[k] - cnt[k];
    }
    __syncthreads();
  }
  if (active) {
    const int cu_z = decoded ? z & ~((parts >> (2 * dp)) - 1) : z;
    int cqo[2] = {0, 0};
    int qp_cu = 0;
    if (COEFFS && decoded) {
      qp_cu = ldg(s.qp + (size_t)ctu * parts + cu_z);            // cu.getQP(0): the CU's first partition
      if (cls) {
        const SliceDev* sl = s.slices + (s.slice_idx ? (int)ldg(s.slice_idx + ctu) : 0);
        cqo[0] = ldg(&sl->cb_qp_offset); cqo[1] = ldg(&sl->cr_qp_offset);
      }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (k >= nk) break;
      const int c = c_lo + k;
      const Cover v = cv[k];
      const int sx = c ? a.csx : 0, sy = c ? a.csy : 0, n = 1 << v.log2n;
      uint32_t off;
      if (compact) off = ldg(s.coef_start[c] + ctu) + s_start[k][v.zo];
      else off = (uint32_t)ctu * ((1u << (2 * log2ctu)) >> (sx + sy)) + ((16u * v.zo) >> (sx + sy)) + (v.lower ? (uint32_t)(n * n) : 0u);
      int8_t per = 0, rem = 0;
      if (COEFFS && decoded) qp_param(qp_cu, c, a.bd[c], c ? cqo[c - 1] : 0, a.fmt, per, rem);
      const int ox4 = (zscan_x(v.zo) * 4 >> sx) >> 2, oy4 = ((zscan_y(v.zo) * 4 >> sy) + (v.lower ? n : 0)) >> 2;
      u32x2 r;
      r.x = off;
      r.y = rec_pack(((coded_mask >> c) & 1u) != 0, v.log2n & 7, ox4, oy4, per, rem, (ts_mask >> c) & 1, byp, intra);
      s_rec[k][z] = r;
    }
    // ---- the info grid, a side product (luma workgroups)
    if (want_info && inpic) {
      int8_t ch[6] = {-1, -1, -1, -1, -1, -1};
      if (ps != HMGPU_SIZE_NONE) {
        ch[0] = (int8_t)(log2ctu - dp - tr); ch[1] = (int8_t)tr; ch[2] = (int8_t)coded_mask;
        ch[3] = (int8_t)(ts_mask | (byp ? 8u : 0u) | (pcm ? 16u : 0u));
        if (intra && (s.gate & kTransDir)) {
          ch[4] = (int8_t)ldg(s.intra_dir[0] + i0);
          if (!a.mono) ch[5] = (int8_t)ldg(s.intra_dir[1] + i0);
        }
      }
      int8_t* d = reinterpret_cast<int8_t*>(a.dst[3] + pic * a.bstride[3] + by * a.pitch[3]) + bx;
#pragma unroll
      for (int k = 0; k < 6; k++) stg(d + k * a.pstride[3], ch[k]);
    }
  }
  if (!sel[0] && !sel[1]) return;
  __syncthreads();
  // ---- phase 2: the CTU's rows in segments of eight samples
  const int sx = cls ? a.csx : 0, sy = cls ? a.csy : 0;
  const int cw = (1 << log2ctu) >> sx, chh = (1 << log2ctu) >> sy;  // the CTU in component samples
  const int pw_c = a.width >> sx, ph_c = a.height >> sy;            // the plane
  const int log2spr = log2ctu - sx - 3, total = chh << log2spr;     // segments per row, segments of the CTU
  const int x00 = ctu_x * cw, y00 = ctu_y * chh;
  constexpr int BYTES = elem_bytes<ELEM>();
  for (int i = threadIdx.x; i < total; i += 256) {
    const int yl = i >> log2spr, xl = (i & ((1 << log2spr) - 1)) * 8;
    const int x = x00 + xl, y = y00 + yl;
    if (x >= pw_c || y >= ph_c) continue;
    const int prow = (yl << sy) >> 2;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (!sel[k]) continue;
      const int c = c_lo + k;
      int val[8];
      u32x2 rc[2];
#pragma unroll
      for (int h = 0; h < 2; h++) rc[h] = s_rec[k][spread4(((xl + 4 * h) << sx) >> 2) | (spread4(prow) << 1)];
      // both halves in one block of eight or more: one 16-byte load
      const bool one = (rc[0].y & 1u) && ((rc[0].y >> 1) & 7u) >= 3;
      u32x2 lv[2] = {{0u, 0u}, {0u, 0u}};
      int idx[2];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int log2n = (rc[h].y >> 1) & 7, ox = ((rc[h].y >> 4) & 15) * 4, oy = ((rc[h].y >> 8) & 15) * 4;
        idx[h] = ((yl - oy) << log2n) + (xl + 4 * h - ox);
      }
      if (one) {
        const u32x4 w = ldg4(s.coef[c] + rc[0].x + idx[0]);
        lv[0].x = w.x; lv[0].y = w.y; lv[1].x = w.z; lv[1].y = w.w;
      } else {
#pragma unroll
        for (int h = 0; h < 2; h++) if (rc[h].y & 1u) lv[h] = ldg2(s.coef[c] + rc[h].x + idx[h]);
      }
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t w1 = rc[h].y;
        int q[4] = {(int16_t)(lv[h].x & 0xffffu), (int16_t)(lv[h].x >> 16), (int16_t)(lv[h].y & 0xffffu), (int16_t)(lv[h].y >> 16)};
        if (COEFFS && (w1 & 1u) && !((w1 >> 21) & 1u)) {
          const int log2n = (w1 >> 1) & 7, per = (w1 >> 12) & 31, rem = (w1 >> 17) & 7, ts = (w1 >> 20) & 1;
          // getUseScalingList (TComTrQuant.h:180): a transform-skip block takes the list only when it is 4x4
          const bool lists = s.sl_m != nullptr && (!ts || log2n == 2);
          const int rs = 6 - (15 - a.bd[c] - log2n + per) + (lists ? 4 : 0);
          const int tb = min(16, (lists ? 17 : 25) + rs), in_max = (1 << (tb - 1)) - 1, in_min = -in_max - 1;
          const int scale = rem == 0 ? 40 : rem == 1 ? 45 : rem == 2 ? 51 : rem == 3 ? 57 : rem == 4 ? 64 : 72;
          uint32_t mw = 0x01010101u;
          if (lists) mw = ldg(reinterpret_cast<const uint32_t*>(s.sl_m + (((log2n - 2) * 6 + (((w1 >> 22) & 1u) ? 0 : 3) + c) << 10) + idx[h]));
#pragma unroll
          for (int j = 0; j < 4; j++) q[j] = dequant1(q[j], scale * (int)((mw >> (8 * j)) & 0xffu), rs, in_min, in_max);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) val[4 * h + j] = q[j];
      }
      const float sc = k == 0 ? (cls ? a.scale[1] : a.scale[0]) : a.scale[2];
      uint32_t o[8];
#pragma unroll
      for (int j = 0; j < 8; j++) o[j] = resid_elem<ELEM>(val[j], sc);
      uint8_t* d = a.dst[c] + pic * a.bstride[c] + y * a.pitch[c] + (ptrdiff_t)x * BYTES;
      if (((a.vec >> c) & 1) && x + 8 <= pw_c) {
        if constexpr (BYTES == 2) stg4(d, u32x4{o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16});
        else { stg4(d, u32x4{o[0], o[1], o[2], o[3]}); stg4(d + 16, u32x4{o[4], o[5], o[6], o[7]}); }
        continue;
      }
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (x + j >= pw_c) break;
        if constexpr (BYTES == 2) stg(reinterpret_cast<uint16_t*>(d) + j, (uint16_t)o[j]);
        else stg(reinterpret_cast<uint32_t*>(d) + j, o[j]);
      }
    }
  }
}

template <bool COEFFS>
static void launch_transform_v(const TransformArgs& a, int elem, const dim3& grid, hipStream_t s) {
  const dim3 block(256);
  if (elem == kElemU16) hipLaunchKernelGGL((k_transform<kElemU16, COEFFS>), grid, block, 0, s, a);
  else if (elem == kElemF16) hipLaunchKernelGGL((k_transform<kElemF16, COEFFS>), grid, block, 0, s, a);
  else if (elem == kElemBF16) hipLaunchKernelGGL((k_transform<kElemBF16, COEFFS>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((k_transform<kElemF32, COEFFS>), grid, block, 0, s, a);
}

void launch_transform(const TransformArgs& a, bool coeffs, int elem, int num_ctus, hipStream_t s) {
  const dim3 grid((unsigned)num_ctus, a.mono ? 1u : 2u, (unsigned)a.n);
  if (coeffs) launch_transform_v<true>(a, elem, grid, s);
  else launch_transform_v<false>(a, elem, grid, s);
}

}  // namespace hmgpu
