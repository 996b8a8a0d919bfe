// hmgpu_packed.hip -- the packed picture input on the host: packer (HM's arrays -> one blob), validator and reference expansion
// (blob -> HM's arrays).  Plain host C++; the device expansion is k_unpack.hip.  Layout: packed_format.h, contract: include/hmgpu.h.
#include "hmgpu_dev.h"
#include "packed_format.h"

#include <cstring>
#include <type_traits>
#include <vector>

using namespace hmgpu;
using namespace hmgpu::packed;

namespace {

struct Geo {
  int n = 0, parts = 0, ctu = 0, log2ctu = 0;
  uint32_t per[3] = {0, 0, 0};   // level elements of one CTU and component (the longest piece)
};

bool geometry(const hmgpu_seq_params* seq, Geo* g) {
  if (!seq || seq->log2_ctu_size < 4 || seq->log2_ctu_size > 6 || seq->width <= 0 || seq->height <= 0) return false;
  g->n = hmgpu_num_ctus(seq); g->parts = hmgpu_parts_per_ctu(seq); g->log2ctu = seq->log2_ctu_size; g->ctu = 1 << g->log2ctu;
  for (int k = 0; k < 3; k++) g->per[k] = (uint32_t)(g->ctu * g->ctu) >> (k ? 2 : 0);
  return true;
}

inline size_t pad4(size_t v) { return (v + 3) & ~(size_t)3; }

// the 8-byte tuple of group g at partition i (packed_format.h); absent optional arrays read as their default
inline uint64_t tuple_of(const hmgpu_ctu_meta* m, int g, size_t i) {
  uint8_t b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  switch (g) {
    case G_CU:
      b[0] = m->depth[i]; b[1] = (uint8_t)m->part_size[i]; b[2] = (uint8_t)m->pred_mode[i]; b[3] = (uint8_t)m->qp[i];
      b[4] = m->transquant_bypass ? m->transquant_bypass[i] : 0; b[5] = m->ipcm ? m->ipcm[i] : 0;
      break;
    case G_TU:
      b[0] = m->tr_idx[i];
      for (int k = 0; k < 3; k++) { b[1 + k] = m->cbf[k][i]; b[4 + k] = m->transform_skip[k] ? m->transform_skip[k][i] : 0; }
      break;
    case G_L0: case G_L1: {
      const int l = g - G_L0;
      if (m->mv[l]) memcpy(b, m->mv[l] + 2 * i, 4);
      b[4] = m->ref_idx[l] ? (uint8_t)m->ref_idx[l][i] : 0xff;
      break;
    }
    default:
      b[0] = m->intra_dir[0][i]; b[1] = m->intra_dir[1][i];
  }
  uint64_t t;
  memcpy(&t, b, 8);
  return t;
}
constexpr uint64_t kDefaultL1 = 0xffull << 32;   // mv 0, ref_idx -1

struct Runs { std::vector<uint32_t> start; std::vector<uint16_t> end; std::vector<uint64_t> tuple; };

// the parts of one level piece as the blob stores them
inline size_t piece_bytes(uint32_t len, uint32_t nnz, bool* raw) {
  const size_t r = pad4(2 * (size_t)len), p = 2 * pad4(2 * (size_t)nnz);
  *raw = r <= p;
  return *raw ? r : p;
}

template <typename T> const T* at(const char* base, const Header& h, int s) { return reinterpret_cast<const T*>(base + h.sec[s][0]); }

}  // namespace

namespace hmgpu {
namespace packed {

hmgpu_status validate(const hmgpu_seq_params* seq, const void* blob, size_t bytes, Summary* out, bool positions) {
  Geo g;
  if (!geometry(seq, &g) || !blob || !out) return HMGPU_EINVAL;
  if (seq->chroma_format > 1) return HMGPU_EUNSUPPORTED;
  // (never larger than the worst case: the runtime's device copy of a blob is allocated at that size)
  if (((uintptr_t)blob & 3) || bytes < kHeaderBytes || bytes > hmgpu_packed_max_bytes(seq)) return HMGPU_EINVAL;
  const char* base = (const char*)blob;
  Header h;
  memcpy(&h, base, sizeof(h));
  if (h.magic != kMagic || h.version != kVersion || h.num_ctus != (uint32_t)g.n || h.parts != (uint32_t)g.parts || h.bytes != bytes) return HMGPU_EINVAL;
  if ((h.groups & 7) != 7 || (h.groups >> kGroups)) return HMGPU_EINVAL;
  const uint64_t n = (uint64_t)g.n;
  for (int s = 0; s < kSections; s++) {
    const uint64_t off = h.sec[s][0], sz = h.sec[s][1];
    if (off % kAlign || off < kHeaderBytes || off + sz > bytes) return HMGPU_EINVAL;
  }
  if (h.sec[S_CTU][1] != 4 * n || h.sec[S_LSTART][1] != 12 * (n + 1) || h.sec[S_LTAB][1] != 24 * n) return HMGPU_EINVAL;
  Summary sm;
  sm.groups = h.groups;
  sm.ctu = at<uint32_t>(base, h, S_CTU);
  for (int a = 0; a < g.n; a++) sm.max_slice = std::max(sm.max_slice, sm.ctu[a] & 0xffff);
  // ---- runs: per CTU at least one, ends strictly ascending, the last one = parts
  for (int gr = 0; gr < kGroups; gr++) {
    if (!(h.groups >> gr & 1)) {
      if (h.sec[sec_starts(gr)][1] || h.sec[sec_ends(gr)][1] || h.sec[sec_tuples(gr)][1]) return HMGPU_EINVAL;
      continue;
    }
    if (h.sec[sec_starts(gr)][1] != 4 * (n + 1)) return HMGPU_EINVAL;
    const uint32_t* st = at<uint32_t>(base, h, sec_starts(gr));
    const uint64_t nruns = st[g.n];
    if (st[0] != 0 || h.sec[sec_ends(gr)][1] != 2 * nruns || h.sec[sec_tuples(gr)][1] != 8 * nruns) return HMGPU_EINVAL;
    const uint16_t* en = at<uint16_t>(base, h, sec_ends(gr));
    const uint8_t* tu = at<uint8_t>(base, h, sec_tuples(gr));
    const uint8_t d8 = (uint8_t)(g.log2ctu - 3), d8m = (uint8_t)(d8 - 1);
    // (branch-free per CTU: the checks of a blob that passes cost ~0.1 ms of the calling thread per 2160p picture)
    unsigned bad = 0;
    for (int a = 0; a < g.n; a++) {
      const uint32_t r0 = st[a], r1 = st[a + 1];
      if (r1 <= r0 || r1 - r0 > (uint32_t)g.parts || r1 > nruns) return HMGPU_EINVAL;
      bad |= (en[r0] == 0) | (en[r1 - 1] != (uint16_t)g.parts);
      for (uint32_t r = r0 + 1; r < r1; r++) bad |= en[r] <= en[r - 1];
    }
    if (bad) return HMGPU_EINVAL;
    if (gr == G_CU) {
      // what stage_inputs' scan of the arrays derives, once per run (the fields are constant over it)
      for (int a = 0; a < g.n; a++)
        for (uint32_t r = st[a], prev = 0; r < st[a + 1]; prev = en[r], r++) {
          const uint8_t* t = tu + 8 * (size_t)r;
          const uint8_t ptn = t[1], d = t[0];
          const bool intra = (int8_t)t[2] == HMGPU_MODE_INTRA;
          sm.n_intra += intra ? en[r] - prev : 0;
          const bool part = ptn != HMGPU_SIZE_2Nx2N && ptn != HMGPU_SIZE_NONE;
          const bool small = d >= d8 || (d == d8m && ptn >= HMGPU_SIZE_2NxnU);
          sm.cells |= part && !intra && small;
          sm.any_bypass |= t[4] == 1; sm.any_pcm |= t[5] == 1;
          sm.flags_used |= t[4] != 0 || t[5] != 0;
        }
    } else if (gr == G_TU) {
      const uint64_t* t = reinterpret_cast<const uint64_t*>(tu);
      uint64_t any = 0;
      for (uint64_t r = 0; r < nruns; r++) any |= t[r];
      sm.flags_used |= (any & 0x00ffffff00000000ull) != 0;        // transform_skip[0..2]
    }
  }
  // ---- levels: CTU starts as the compact form has them, every piece inside the data section, positions strictly ascending inside the piece
  const uint32_t* ls = at<uint32_t>(base, h, S_LSTART);
  const uint32_t* lt = at<uint32_t>(base, h, S_LTAB);
  const uint64_t data_bytes = h.sec[S_LDATA][1];
  const char* data = base + h.sec[S_LDATA][0];
  for (int k = 0; k < 3; k++) {
    const uint32_t* s = ls + (size_t)k * (n + 1);
    if (s[0] != 0) return HMGPU_EINVAL;
    for (int a = 0; a < g.n; a++) {
      if (s[a + 1] < s[a] || s[a + 1] - s[a] > g.per[k]) return HMGPU_EINVAL;
      const uint32_t len = s[a + 1] - s[a];
      const uint64_t off = 4 * (uint64_t)lt[(size_t)a * 6 + 2 * k], w1 = lt[(size_t)a * 6 + 2 * k + 1];
      if (w1 == kRaw) {
        if (off + pad4(2 * (size_t)len) > data_bytes) return HMGPU_EINVAL;
        continue;
      }
      if (w1 > len || off + 2 * pad4(2 * w1) > data_bytes) return HMGPU_EINVAL;
      if (!w1 || !positions) continue;
      // (as int16: a vectorised compare; positions >= 32768 are caught by the OR of all of them)
      const int16_t* pos = (const int16_t*)(data + off);
      unsigned bad = (uint16_t)pos[w1 - 1] >= len;
      uint16_t all = 0;
      for (uint32_t i = 0; i + 1 < (uint32_t)w1; i++) { bad |= pos[i] >= pos[i + 1]; all |= (uint16_t)pos[i]; }
      if (bad || (all & 0x8000)) return HMGPU_EINVAL;
    }
  }
  *out = sm;
  return HMGPU_OK;
}

}  // namespace packed
}  // namespace hmgpu

extern "C" {

size_t hmgpu_packed_max_bytes(const hmgpu_seq_params* seq) {
  Geo g;
  if (!geometry(seq, &g)) return 0;
  const size_t n = (size_t)g.n, np = n * g.parts;
  size_t b = kHeaderBytes + align(4 * n) + align(12 * (n + 1)) + align(24 * n);
  b += kGroups * (align(4 * (n + 1)) + align(2 * np) + align(8 * np));
  for (int k = 0; k < 3; k++) b += n * pad4(2 * (size_t)g.per[k]);     // every piece full length, raw
  return align(b);
}

hmgpu_status hmgpu_pack_input(const hmgpu_seq_params* seq, const hmgpu_ctu_meta* m, const hmgpu_coeffs* co, void* out, size_t capacity,
                              size_t* bytes_out) {
  Geo g;
  if (!geometry(seq, &g) || !m || !co || !out || !bytes_out || ((uintptr_t)out & 3)) return HMGPU_EINVAL;
  if (seq->chroma_format < 0 || seq->chroma_format > 3) return HMGPU_EINVAL;
  if (seq->chroma_format > 1) return HMGPU_EUNSUPPORTED;          // (the compact form's envelope: 4:0:0 / 4:2:0)
  if (!m->depth || !m->part_size || !m->pred_mode || !m->qp || !m->tr_idx || !m->cbf[0] || !m->cbf[1] || !m->cbf[2] || !m->mv[0] ||
      !m->ref_idx[0] || !co->level[0] || !co->level[1] || !co->level[2]) return HMGPU_EINVAL;
  const size_t n = (size_t)g.n, np = n * g.parts;
  // ---- levels in the compact form: the caller's, or packed here from HM's dense arrays
  const bool compact = co->ctu_level_start[0] && co->ctu_level_start[1] && co->ctu_level_start[2];
  if (!compact && (co->ctu_level_start[0] || co->ctu_level_start[1] || co->ctu_level_start[2])) return HMGPU_EINVAL;
  std::vector<int16_t> lv_own[3];
  std::vector<uint32_t> st_own[3];
  const int16_t* lv[3];
  const uint32_t* st[3];
  if (compact) {
    for (int k = 0; k < 3; k++) {
      lv[k] = co->level[k]; st[k] = co->ctu_level_start[k];
      if (st[k][0] != 0) return HMGPU_EINVAL;
      for (size_t a = 0; a < n; a++) if (st[k][a + 1] < st[k][a] || st[k][a + 1] - st[k][a] > g.per[k]) return HMGPU_EINVAL;
    }
  } else {
    int16_t* ol[3];
    uint32_t* os[3];
    for (int k = 0; k < 3; k++) {
      lv_own[k].resize(n * g.per[k]); st_own[k].resize(n + 1);
      ol[k] = lv_own[k].data(); os[k] = st_own[k].data(); lv[k] = ol[k]; st[k] = os[k];
    }
    const hmgpu_status s = hmgpu_pack_levels(seq, m, co, ol, os);
    if (s != HMGPU_OK) return s;
  }
  // ---- runs of every group, CTU by CTU
  uint32_t groups = (1u << G_CU) | (1u << G_TU) | (1u << G_L0);
  if (m->mv[1] && m->ref_idx[1])
    for (size_t i = 0; i < np; i++) if (tuple_of(m, G_L1, i) != kDefaultL1) { groups |= 1u << G_L1; break; }
  if (m->intra_dir[0] && m->intra_dir[1]) groups |= 1u << G_INTRA;
  Runs runs[kGroups];
  for (int gr = 0; gr < kGroups; gr++) {
    if (!(groups >> gr & 1)) continue;
    Runs& r = runs[gr];
    r.start.resize(n + 1);
    for (size_t a = 0; a < n; a++) {
      r.start[a] = (uint32_t)r.end.size();
      const size_t i0 = a * g.parts;
      uint64_t cur = tuple_of(m, gr, i0);
      for (int z = 1; z < g.parts; z++) {
        const uint64_t t = tuple_of(m, gr, i0 + z);
        if (t != cur) { r.end.push_back((uint16_t)z); r.tuple.push_back(cur); cur = t; }
      }
      r.end.push_back((uint16_t)g.parts); r.tuple.push_back(cur);
    }
    r.start[n] = (uint32_t)r.end.size();
  }
  // ---- the level pieces: raw or (position, value) pairs, whichever is smaller
  std::vector<uint32_t> nnz(3 * n);
  size_t data_bytes = 0;
  for (size_t a = 0; a < n; a++)
    for (int k = 0; k < 3; k++) {
      const int16_t* p = lv[k] + st[k][a];
      const uint32_t len = st[k][a + 1] - st[k][a];
      uint32_t c = 0;
      for (uint32_t i = 0; i < len; i++) c += p[i] != 0;
      nnz[a * 3 + k] = c;
      bool raw;
      data_bytes += piece_bytes(len, c, &raw);
    }
  // ---- layout
  Header h;
  memset(&h, 0, sizeof(h));
  h.magic = kMagic; h.version = kVersion; h.num_ctus = (uint32_t)n; h.parts = (uint32_t)g.parts; h.groups = groups;
  size_t off = kHeaderBytes;
  auto place = [&](int s, size_t sz) { h.sec[s][0] = (uint32_t)off; h.sec[s][1] = (uint32_t)sz; off = align(off + sz); };
  place(S_CTU, 4 * n);
  for (int gr = 0; gr < kGroups; gr++) {
    const size_t nr = runs[gr].end.size();
    place(sec_starts(gr), (groups >> gr & 1) ? 4 * (n + 1) : 0);
    place(sec_ends(gr), 2 * nr);
    place(sec_tuples(gr), 8 * nr);
  }
  place(S_LSTART, 12 * (n + 1));
  place(S_LTAB, 24 * n);
  place(S_LDATA, data_bytes);
  if (off > capacity || off > 0xffffffffu) return HMGPU_EINVAL;
  h.bytes = (uint32_t)off;
  char* base = (char*)out;
  memset(base, 0, off);                                          // (padding included: the blob is a function of the input alone)
  memcpy(base, &h, sizeof(h));
  uint32_t* ctu = (uint32_t*)(base + h.sec[S_CTU][0]);
  for (size_t a = 0; a < n; a++)
    ctu[a] = (m->slice_idx ? m->slice_idx[a] : 0u) | (uint32_t)(m->tile_idx ? m->tile_idx[a] : 0u) << 16;
  for (int gr = 0; gr < kGroups; gr++) {
    if (!(groups >> gr & 1)) continue;
    const Runs& r = runs[gr];
    memcpy(base + h.sec[sec_starts(gr)][0], r.start.data(), 4 * (n + 1));
    memcpy(base + h.sec[sec_ends(gr)][0], r.end.data(), 2 * r.end.size());
    memcpy(base + h.sec[sec_tuples(gr)][0], r.tuple.data(), 8 * r.tuple.size());
  }
  for (int k = 0; k < 3; k++) memcpy(base + h.sec[S_LSTART][0] + 4 * (n + 1) * k, st[k], 4 * (n + 1));
  uint32_t* lt = (uint32_t*)(base + h.sec[S_LTAB][0]);
  char* data = base + h.sec[S_LDATA][0];
  size_t doff = 0;
  for (size_t a = 0; a < n; a++)
    for (int k = 0; k < 3; k++) {
      const int16_t* p = lv[k] + st[k][a];
      const uint32_t len = st[k][a + 1] - st[k][a], c = nnz[a * 3 + k];
      bool raw;
      const size_t pb = piece_bytes(len, c, &raw);
      lt[a * 6 + 2 * k] = (uint32_t)(doff / 4);
      lt[a * 6 + 2 * k + 1] = raw ? kRaw : c;
      if (raw) {
        memcpy(data + doff, p, 2 * (size_t)len);
      } else {
        uint16_t* pos = (uint16_t*)(data + doff);
        int16_t* val = (int16_t*)(data + doff + pad4(2 * (size_t)c));
        uint32_t j = 0;
        for (uint32_t i = 0; i < len; i++)
          if (p[i]) { pos[j] = (uint16_t)i; val[j] = p[i]; j++; }
      }
      doff += pb;
    }
  *bytes_out = off;
  return HMGPU_OK;
}

hmgpu_status hmgpu_unpack_input(const hmgpu_seq_params* seq, const void* blob, size_t bytes, const hmgpu_ctu_meta_out* out_meta,
                                int16_t* const out_level[3], uint32_t* const out_start[3]) {
  Summary sm;
  const hmgpu_status s = validate(seq, blob, bytes, &sm, true);
  if (s != HMGPU_OK) return s;
  Geo g;
  geometry(seq, &g);
  const size_t n = (size_t)g.n;
  const char* base = (const char*)blob;
  Header h;
  memcpy(&h, base, sizeof(h));
  if (out_meta) {
    const hmgpu_ctu_meta_out& m = *out_meta;
    for (size_t a = 0; a < n; a++) {
      if (m.slice_idx) m.slice_idx[a] = (uint16_t)(sm.ctu[a] & 0xffff);
      if (m.tile_idx) m.tile_idx[a] = (uint16_t)(sm.ctu[a] >> 16);
    }
    for (int gr = 0; gr < kGroups; gr++) {
      const bool present = h.groups >> gr & 1;
      const uint32_t* st = present ? at<uint32_t>(base, h, sec_starts(gr)) : nullptr;
      const uint16_t* en = present ? at<uint16_t>(base, h, sec_ends(gr)) : nullptr;
      const uint8_t* tu = present ? at<uint8_t>(base, h, sec_tuples(gr)) : nullptr;
      const uint64_t dflt = gr == G_L1 ? kDefaultL1 : 0;
      for (size_t a = 0; a < n; a++) {
        uint32_t r = present ? st[a] : 0, z = 0;
        while (z < (uint32_t)g.parts) {
          uint8_t t[8];
          uint32_t e = (uint32_t)g.parts;
          if (present) { memcpy(t, tu + 8 * (size_t)r, 8); e = en[r++]; } else memcpy(t, &dflt, 8);
          for (; z < e; z++) {
            const size_t i = a * g.parts + z;
            auto put = [&](auto* arr, uint8_t v) { if (arr) arr[i] = (std::remove_pointer_t<decltype(arr)>)v; };
            switch (gr) {
              case G_CU: put(m.depth, t[0]); put(m.part_size, t[1]); put(m.pred_mode, t[2]); put(m.qp, t[3]);
                         put(m.transquant_bypass, t[4]); put(m.ipcm, t[5]); break;
              case G_TU: put(m.tr_idx, t[0]); for (int k = 0; k < 3; k++) { put(m.cbf[k], t[1 + k]); put(m.transform_skip[k], t[4 + k]); } break;
              case G_L0: case G_L1: {
                const int l = gr - G_L0;
                if (m.mv[l]) memcpy(m.mv[l] + 2 * i, t, 4);
                put(m.ref_idx[l], t[4]);
                break;
              }
              default: put(m.intra_dir[0], t[0]); put(m.intra_dir[1], t[1]);
            }
          }
        }
      }
    }
  }
  const uint32_t* ls = at<uint32_t>(base, h, S_LSTART);
  const uint32_t* lt = at<uint32_t>(base, h, S_LTAB);
  const char* data = base + h.sec[S_LDATA][0];
  for (int k = 0; k < 3; k++) {
    const uint32_t* s = ls + k * (n + 1);
    if (out_start && out_start[k]) memcpy(out_start[k], s, 4 * (n + 1));
    if (!out_level || !out_level[k]) continue;
    for (size_t a = 0; a < n; a++) {
      int16_t* dst = out_level[k] + s[a];
      const uint32_t len = s[a + 1] - s[a], w1 = lt[a * 6 + 2 * k + 1];
      const char* src = data + 4 * (size_t)lt[a * 6 + 2 * k];
      if (w1 == kRaw) { memcpy(dst, src, 2 * (size_t)len); continue; }
      memset(dst, 0, 2 * (size_t)len);
      const uint16_t* pos = (const uint16_t*)src;
      const int16_t* val = (const int16_t*)(src + pad4(2 * (size_t)w1));
      for (uint32_t j = 0; j < w1; j++) dst[pos[j]] = val[j];
    }
  }
  return HMGPU_OK;
}

}  // extern "C"
