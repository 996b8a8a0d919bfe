// k_unpack.hip -- device expansion of the packed picture input (include/hmgpu.h "packed input", layout: packed_format.h).
//
// One workgroup per CTU and picture.  It writes exactly what the staging path copies: the picture's metadata arrays (carve_meta
// layout, hmgpu_api.hip), the per-CTU slice / tile index, the compact levels and their CTU starts.  Every blob was validated on the
// host (packed::validate) before the launch: run ends are strictly ascending up to parts_per_ctu, every section and every level piece
// lies inside the blob, level positions are strictly ascending inside their piece -- the kernel trusts those facts (a position is still
// bounded by its piece before it indexes LDS: a cheap guard against a blob changed after the check).
//
// Metadata: the run ends of the CTU's runs of one group go to LDS; a lane owns four consecutive partitions, finds the run of the first
// by binary search and steps on for the other three, and writes each byte array with one dword store (motion vectors: one dwordx4).
// Levels: a raw piece is copied through; a sparse piece is zeroed in LDS (<= 4096 elements = 8 KB), the pairs are scattered into it,
// and the piece leaves coalesced.
#include "hmgpu_dev.h"
#include "packed_format.h"

namespace hmgpu {

namespace {

constexpr int kThreads = 256;

__device__ inline uint32_t hdr(const char* base, int word) { return ldg(reinterpret_cast<const uint32_t*>(base) + word); }
__device__ inline const char* section(const char* base, int s) { return base + hdr(base, 8 + 2 * s); }

// byte b of the four tuples as one dword (partition z0 + j in byte j)
__device__ inline uint32_t bytes4(const u32x2 t[4], int b) {
  uint32_t v = 0;
  for (int j = 0; j < 4; j++) v |= (((b < 4 ? t[j].x >> (8 * b) : t[j].y >> (8 * (b - 4))) & 0xffu) << (8 * j));
  return v;
}
template <typename T> __device__ inline void st_u32(const T* p, size_t i, uint32_t v) { stg(reinterpret_cast<uint32_t*>(const_cast<T*>(p) + i), v); }

__global__ void __launch_bounds__(kThreads) k_unpack_input(const PicDev* __restrict__ pics, UnpackArgs ua) {
  __shared__ uint16_t s_end[256];
  __shared__ int16_t s_piece[4096];
  const int a = blockIdx.x, t = threadIdx.x;
  const PicDev& P = pics[ua.pic[blockIdx.z]];
  const char* base = ua.blob[blockIdx.z];
  const int parts = P.parts, n = P.num_ctus;
  const uint32_t groups = hdr(base, 4);
  const int z0 = 4 * t;
  const bool active = z0 < parts;
  const size_t i0 = (size_t)a * parts + z0;
  if (t == 0) {
    const uint32_t v = ldg(reinterpret_cast<const uint32_t*>(section(base, packed::S_CTU)) + a);
    stg(const_cast<uint16_t*>(P.slice_idx) + a, (uint16_t)(v & 0xffff));
    stg(const_cast<uint16_t*>(P.tile_idx) + a, (uint16_t)(v >> 16));
  }
  // ---- metadata, group by group
  for (int g = 0; g < packed::kGroups; g++) {
    const bool present = (groups >> g) & 1;
    if (!present && g == packed::G_INTRA) continue;              // (no modes: intra CUs are left untouched, has_intra_dir = 0)
    u32x2 tup[4];
    if (present) {
      const uint32_t* starts = reinterpret_cast<const uint32_t*>(section(base, packed::sec_starts(g)));
      const uint16_t* ends = reinterpret_cast<const uint16_t*>(section(base, packed::sec_ends(g)));
      const u32x2* tuples = reinterpret_cast<const u32x2*>(section(base, packed::sec_tuples(g)));
      const uint32_t r0 = ldg(starts + a), nr = ldg(starts + a + 1) - r0;
      __syncthreads();                                           // (the previous group's searches are done with s_end)
      if ((uint32_t)t < nr) s_end[t] = ldg(ends + r0 + t);
      __syncthreads();
      if (active) {
        uint32_t lo = 0, hi = nr - 1;                            // the first run whose end lies beyond z0
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s_end[mid] > (uint32_t)z0) hi = mid; else lo = mid + 1; }
        for (int j = 0; j < 4; j++) {
          while (s_end[lo] <= (uint32_t)(z0 + j)) lo++;
          tup[j] = ldg2(tuples + r0 + lo);
        }
      }
    } else {
      for (int j = 0; j < 4; j++) tup[j] = u32x2{0u, g == packed::G_L1 ? 0xffu : 0u};   // list 1 left out: mv 0, ref_idx -1
    }
    if (!active) continue;
    switch (g) {
      case packed::G_CU:
        st_u32(P.depth, i0, bytes4(tup, 0)); st_u32(P.part_size, i0, bytes4(tup, 1)); st_u32(P.pred_mode, i0, bytes4(tup, 2));
        st_u32(P.qp, i0, bytes4(tup, 3)); st_u32(P.bypass, i0, bytes4(tup, 4)); st_u32(P.ipcm, i0, bytes4(tup, 5));
        break;
      case packed::G_TU:
        st_u32(P.tr_idx, i0, bytes4(tup, 0));
        for (int k = 0; k < 3; k++) { st_u32(P.cbf[k], i0, bytes4(tup, 1 + k)); st_u32(P.tskip[k], i0, bytes4(tup, 4 + k)); }
        break;
      case packed::G_L0: case packed::G_L1: {
        const int l = g - packed::G_L0;
        u32x4 mv;
        mv.x = tup[0].x; mv.y = tup[1].x; mv.z = tup[2].x; mv.w = tup[3].x;
        stg4(const_cast<int16_t*>(P.mv[l]) + 2 * i0, mv);
        st_u32(P.ref_idx[l], i0, bytes4(tup, 4));
        break;
      }
      default:
        st_u32(P.intra_dir[0], i0, bytes4(tup, 0)); st_u32(P.intra_dir[1], i0, bytes4(tup, 1));
    }
  }
  // ---- levels: one piece per component
  const uint32_t* lstart = reinterpret_cast<const uint32_t*>(section(base, packed::S_LSTART));
  const uint32_t* ltab = reinterpret_cast<const uint32_t*>(section(base, packed::S_LTAB));
  const char* data = section(base, packed::S_LDATA);
  for (int k = 0; k < 3; k++) {
    const uint32_t* ls = lstart + (size_t)k * (n + 1);
    const uint32_t s0 = ldg(ls + a), len = ldg(ls + a + 1) - s0;
    uint32_t* cs = const_cast<uint32_t*>(P.coef_start[k]);
    if (t == 0) { stg(cs + a, s0); if (a == n - 1) stg(cs + n, s0 + len); }
    if (len == 0) continue;                                      // (uniform over the workgroup)
    const uint32_t off = ldg(ltab + (size_t)a * 6 + 2 * k), mode = ldg(ltab + (size_t)a * 6 + 2 * k + 1);
    const char* src = data + 4 * (size_t)off;
    int16_t* dst = const_cast<int16_t*>(P.coef[k]) + s0;
    if (mode == packed::kRaw) {
      const int16_t* v = reinterpret_cast<const int16_t*>(src);
      for (uint32_t i = t; i < len; i += kThreads) stg(dst + i, ldg(v + i));
      continue;
    }
    __syncthreads();                                             // (the previous piece has left LDS)
    for (uint32_t i = t; i < len; i += kThreads) s_piece[i] = 0;
    __syncthreads();
    const uint16_t* pos = reinterpret_cast<const uint16_t*>(src);
    const int16_t* val = reinterpret_cast<const int16_t*>(src + ((2 * mode + 3) & ~3u));
    for (uint32_t j = t; j < mode; j += kThreads) {
      const uint32_t q = ldg(pos + j);
      if (q < len) s_piece[q] = ldg(val + j);
    }
    __syncthreads();
    for (uint32_t i = t; i < len; i += kThreads) stg(dst + i, s_piece[i]);
  }
}

}  // namespace

void launch_unpack_input(const PicDev* pics, const UnpackArgs& ua, int num_ctus, hipStream_t s) {
  hipLaunchKernelGGL(k_unpack_input, dim3((unsigned)num_ctus, 1, (unsigned)ua.n), dim3(kThreads), 0, s, pics, ua);
}

}  // namespace hmgpu
