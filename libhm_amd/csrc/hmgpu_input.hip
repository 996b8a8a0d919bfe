// hmgpu_input.hip -- the input side of the host runtime: slice registration, staging of HM's per-CTU arrays and of the packed form,
// staging blocks, the slice / picture / batch decompress entry points and the filter entry points.
#include "hmgpu_host.h"
#include "packed_format.h"

#include <algorithm>
#include <cstring>
#include <iterator>
#include <new>
#include <thread>
#include <vector>

static void mark_use(hmgpu_ctx* c, const Batch& b) {
  for (int i = 0; i < b.n; i++) touch(c, b.pic[i]);
  commit_use(c);
}

extern "C" {

// slice table entry of one slice (validation, SliceDev, scaling lists): the part of a slice call that does not depend on CTUs
static hmgpu_status register_slice(hmgpu_ctx* c, hmgpu_pic cur, int32_t slice_idx, const hmgpu_slice_params* sl, hipStream_t hs) {
  if (slice_idx < 0 || slice_idx >= HMGPU_MAX_SLICES || !sl) return HMGPU_EINVAL;
  if (sl->weighted_pred && (sl->wp_log2_denom[0] < 0 || sl->wp_log2_denom[0] > 7 || sl->wp_log2_denom[1] < 0 || sl->wp_log2_denom[1] > 7)) return HMGPU_EINVAL;
  Picture& p = c->pics[cur];
  // reference pictures must be live device pictures
  for (int l = 0; l < 2; l++) {
    if (sl->num_ref_idx[l] < 0 || sl->num_ref_idx[l] > HMGPU_MAX_REF) return HMGPU_EINVAL;
    for (int i = 0; i < sl->num_ref_idx[l]; i++) if (!valid_pic(c, sl->ref_pic[l][i]) || sl->ref_pic[l][i] == cur) return HMGPU_EINVAL;
  }
  hipSetDevice(c->device);
  SliceDev sd;
  memset(&sd, 0, sizeof(sd));
  sd.slice_type = sl->slice_type; sd.cb_qp_offset = sl->cb_qp_offset; sd.cr_qp_offset = sl->cr_qp_offset;
  sd.pps_cb_qp_offset = sl->pps_cb_qp_offset; sd.pps_cr_qp_offset = sl->pps_cr_qp_offset;
  sd.deblocking_disable = sl->deblocking_disable; sd.beta_offset_div2 = sl->beta_offset_div2; sd.tc_offset_div2 = sl->tc_offset_div2;
  sd.lf_across_slices = sl->lf_across_slices;
  sd.constrained_intra_pred = sl->constrained_intra_pred ? 1 : 0;
  sd.weighted_pred = sl->weighted_pred ? 1 : 0;
  sd.wp_log2_denom[0] = sl->wp_log2_denom[0]; sd.wp_log2_denom[1] = sl->wp_log2_denom[1];
  memcpy(sd.wp_weight, sl->wp_weight, sizeof(sd.wp_weight));
  memcpy(sd.wp_offset, sl->wp_offset, sizeof(sd.wp_offset));
  for (int l = 0; l < 2; l++)
    for (int i = 0; i < HMGPU_MAX_REF; i++) {
      sd.ref_poc[l][i] = i < sl->num_ref_idx[l] ? sl->ref_poc[l][i] : 0;
      sd.ref_pic[l][i] = i < sl->num_ref_idx[l] ? (int8_t)sl->ref_pic[l][i] : (int8_t)-1;
    }
  p.slices[slice_idx] = sd;
  p.max_slice = std::max(p.max_slice, (int)slice_idx);
  p.dev.lf_across_tiles = sl->lf_across_tiles;
  p.dev.sl_m = nullptr;
  if (sl->scaling_lists) {
    // xSetScalingListDec / processScalingListDec (TComTrQuant.cpp:2992-3012, 3092-3106) without the per-QP factor: m per position
    const hmgpu_scaling_lists& L = *sl->scaling_lists;
    p.sl_host.assign(4 * 6 * 1024, 16);
    for (int sz = 0; sz < 4; sz++)
      for (int l = 0; l < 6; l++) {
        const int n = 4 << sz, ratio = n > 8 ? n / 8 : 1, mn = n > 8 ? 8 : n;
        uint8_t* t = p.sl_host.data() + (sz * 6 + l) * 1024;
        for (int y = 0; y < n; y++)
          for (int x = 0; x < n; x++) {
            const int v = (ratio > 1 && x == 0 && y == 0) ? L.dc[sz][l] : L.coef[sz][l][mn * (y / ratio) + x / ratio];
            if (v < 1 || v > 255) return HMGPU_EINVAL;
            t[y * n + x] = (uint8_t)v;
          }
      }
    HIP_TRY(c, h2d_small(c, p.sl_table, p.sl_host.data(), p.sl_host.size(), hs));
    p.dev.sl_m = p.sl_table;
  }
  HIP_TRY(c, h2d_small(c, (void*)(p.dev.slices + slice_idx), &p.slices[slice_idx], sizeof(SliceDev), hs));
  return HMGPU_OK;
}

static bool stg_starts_contiguous(const hmgpu_coeffs* co, int num_ctus) {
  return co->ctu_level_start[1] == co->ctu_level_start[0] + (num_ctus + 1) && co->ctu_level_start[2] == co->ctu_level_start[1] + (num_ctus + 1);
}

// a staging block whose arrays the caller handed over for a whole picture: its metadata is ONE copy, its levels another
static const hmgpu_staging* staging_of(const hmgpu_ctx* c, const hmgpu_ctu_meta* m, const hmgpu_coeffs* co) {
  for (size_t i = 0; i < c->stagings.size() + c->shared_stagings.size(); i++) {
    const hmgpu_staging* st = i < c->stagings.size() ? c->stagings[i] : c->shared_stagings[i - c->stagings.size()];
    const hmgpu_ctu_meta& h = st->m;
    if (m->depth != h.depth) continue;
    // the required arrays are the block's; the optional ones are the block's or left out (NULL: that group does not travel)
    bool ok = m->part_size == h.part_size && m->pred_mode == h.pred_mode && m->qp == h.qp && m->tr_idx == h.tr_idx && m->slice_idx == h.slice_idx &&
              m->tile_idx == h.tile_idx;
    for (int k = 0; k < 3 && ok; k++) ok = m->cbf[k] == h.cbf[k] && (!m->transform_skip[k] || m->transform_skip[k] == h.transform_skip[k]);
    for (int k = 0; k < 2 && ok; k++) ok = m->mv[k] == h.mv[k] && m->ref_idx[k] == h.ref_idx[k] && (!m->intra_dir[k] || m->intra_dir[k] == h.intra_dir[k]);
    ok = ok && (!m->transquant_bypass || m->transquant_bypass == h.transquant_bypass) && (!m->ipcm || m->ipcm == h.ipcm);
    for (int k = 0; k < 3 && ok; k++) ok = co->level[k] == st->co.level[k];
    if (ok) return st;
  }
  return nullptr;
}

// what every way of staging a CTU range ends with: PCM samples, the picture's descriptor, and the record of the call (which kernels run)
static hmgpu_status finish_stage(hmgpu_ctx* c, hmgpu_pic cur, int32_t slice_idx, const std::vector<int>& slices, bool any_wp,
                                 const int16_t* const pcm_sample[3], bool any_pcm, bool any_bypass, int32_t first_ctu, int32_t num_ctus,
                                 size_t n_intra, bool cells, hipStream_t hs, SliceCall* call_out) {
  Picture& p = c->pics[cur];
  const size_t pn = (size_t)num_ctus * c->parts;
  {
    if (any_pcm) {
      size_t bytes = 0;
      for (int k = 0; k < 3; k++) bytes += align_up(c->coef_elems[k] * sizeof(int16_t), 256);
      if (!p.pcm) {
        HIP_TRY(c, hipMalloc(&p.pcm, bytes));
        Carver cp(p.pcm);
        for (int k = 0; k < 3; k++) p.dev.pcm[k] = cp.take<int16_t>(c->coef_elems[k]);
      }
      for (int k = 0; k < 3; k++) {
        const size_t per = (size_t)(c->ctu * c->ctu) >> (k ? c->csx + c->csy : 0);
        HIP_TRY(c, hipMemcpyAsync((void*)(p.dev.pcm[k] + first_ctu * per), pcm_sample[k] + first_ctu * per, (size_t)num_ctus * per * 2,
                                  hipMemcpyHostToDevice, hs));
      }
      p.dev.pcm_shift[0] = c->seq.bit_depth_luma - c->seq.pcm_bit_depth_luma;
      p.dev.pcm_shift[1] = p.dev.pcm_shift[2] = c->seq.bit_depth_chroma - c->seq.pcm_bit_depth_chroma;
    }
    if (any_bypass || (any_pcm && c->seq.pcm_loop_filter_disable)) p.dev.any_nofilt = 1;
    HIP_TRY(c, h2d_small(c, c->d_pics + cur, &p.dev, sizeof(PicDev), hs));
  }
  // a range decoded again (picture buffer reused without release/acquire) replaces the earlier record
  p.calls.erase(std::remove_if(p.calls.begin(), p.calls.end(), [&](const SliceCall& o) {
                  return o.first_ctu < first_ctu + num_ctus && first_ctu < o.first_ctu + o.num_ctus; }), p.calls.end());
  const bool has_intra = p.dev.has_intra_dir && n_intra != 0;
  bool any_b = false, any_i = false;
  for (int si : slices) { any_b |= p.slices[si].slice_type == HMGPU_B_SLICE; any_i |= p.slices[si].slice_type == HMGPU_I_SLICE; }
  // I slices, or a range at least half intra, take the intra kernel that stages whole CTUs
  if (has_intra && !any_i) any_i = 2 * n_intra >= pn;
  SliceCall call = {first_ctu, num_ctus, slice_idx, has_intra, any_wp, cells, any_b, any_i, p.dev.has_intra_dir != 0};
  p.calls.push_back(call);
  p.extended = false;
  coverage_add(c, p, first_ctu, num_ctus);
  *call_out = call;
  return HMGPU_OK;
}

// HM arrays of a CTU range to the device (on stream hs) and the record of the call.  `slices` lists the slice table entries whose
// reference pictures the range may read; slice_idx is the one a missing meta->slice_idx array stands for.
static hmgpu_status stage_inputs(hmgpu_ctx* c, hmgpu_pic cur, int32_t slice_idx, const std::vector<int>& slices, bool any_wp,
                                 const hmgpu_ctu_meta* m, const hmgpu_coeffs* co, int32_t first_ctu, int32_t num_ctus, hipStream_t hs,
                                 SliceCall* call_out) {
  Picture& p = c->pics[cur];
  const size_t po = (size_t)first_ctu * c->parts, pn = (size_t)num_ctus * c->parts;
  // lossless / PCM CUs need their own inputs
  const bool any_pcm = m->ipcm && memchr(m->ipcm + po, 1, pn) != nullptr;
  const bool any_bypass = m->transquant_bypass && memchr(m->transquant_bypass + po, 1, pn) != nullptr;
  if (any_pcm && (!co->pcm_sample[0] || !co->pcm_sample[1] || !co->pcm_sample[2] || !m->intra_dir[0])) return HMGPU_EINVAL;
  if (any_pcm && (c->seq.pcm_bit_depth_luma < 1 || c->seq.pcm_bit_depth_luma > c->seq.bit_depth_luma ||
                  c->seq.pcm_bit_depth_chroma < 1 || c->seq.pcm_bit_depth_chroma > c->seq.bit_depth_chroma)) return HMGPU_EINVAL;
  p.dev.has_intra_dir = (m->intra_dir[0] && m->intra_dir[1]) ? 1 : 0;      // without the modes intra CUs are left untouched
  const hmgpu_staging* stg = (first_ctu == 0 && num_ctus == c->num_ctus) ? staging_of(c, m, co) : nullptr;
  const bool compact = co->ctu_level_start[0] && co->ctu_level_start[1] && co->ctu_level_start[2];
  if (!compact && (co->ctu_level_start[0] || co->ctu_level_start[1] || co->ctu_level_start[2])) return HMGPU_EINVAL;
  if (compact) {
    if (c->fmt != 1) return HMGPU_EUNSUPPORTED;                              // (4:2:2 / 4:4:4: HM's dense layout only)
    if (first_ctu != 0 || num_ctus != c->num_ctus) return HMGPU_EINVAL;      // whole pictures only
    for (int k = 0; k < 3; k++) {
      // the CTUs' pieces follow each other and none is longer than a CTU (k_intra stages a CTU's piece into LDS by these numbers)
      const uint32_t per = (uint32_t)(c->ctu * c->ctu) >> (k ? 2 : 0);
      const uint32_t* st = co->ctu_level_start[k];
      if (st[c->num_ctus] > c->coef_elems[k]) return HMGPU_EINVAL;
      for (int i = 0; i < c->num_ctus; i++) if (st[i + 1] < st[i] || st[i + 1] - st[i] > per) return HMGPU_EINVAL;
    }
    // the CTU starts (from a staging block: its three arrays in one copy)
    const bool one = stg_starts_contiguous(co, c->num_ctus);
    for (int k = 0; k < (one ? 1 : 3); k++)
      HIP_TRY(c, hipMemcpyAsync(p.coef_start + (size_t)k * (c->num_ctus + 1), co->ctu_level_start[k],
                                (size_t)(one ? 3 : 1) * (c->num_ctus + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, hs));
    for (int k = 0; k < 3; k++) {
      p.dev.coef_start[k] = p.coef_start + (size_t)k * (c->num_ctus + 1);
      const size_t n = co->ctu_level_start[k][c->num_ctus];
      if (n) HIP_TRY(c, hipMemcpyAsync((void*)p.dev.coef[k], co->level[k], n * sizeof(int16_t), hipMemcpyHostToDevice, hs));
    }
  } else {
    for (int k = 0; k < 3; k++) p.dev.coef_start[k] = nullptr;
  }
  if (stg) {
    // the caller filled a staging block: the metadata block in one DMA (the dense levels in another) -- minus the groups this
    // picture does without: list 1 when no slice is a B slice (k_prep ignores it then), the intra modes and the transform-skip /
    // lossless / PCM flags when the caller left them out (the device copies of the flags are cleared if an earlier picture set them)
    bool any_b_slice = false;
    for (int si : slices) any_b_slice |= p.slices[si].slice_type == HMGPU_B_SLICE;
    const bool flags_used = m->transform_skip[0] || m->transform_skip[1] || m->transform_skip[2] || m->transquant_bypass || m->ipcm;
    const bool want[4] = {true, any_b_slice, p.dev.has_intra_dir != 0, flags_used};
    for (int g0 = 0; g0 < 4;) {
      if (!want[g0]) { g0++; continue; }
      int g1 = g0 + 1;
      while (g1 < 4 && want[g1]) g1++;
      HIP_TRY(c, hipMemcpyAsync((char*)p.meta + stg->grp[g0], stg->host + stg->grp[g0], stg->grp[g1] - stg->grp[g0], hipMemcpyHostToDevice, hs));
      g0 = g1;
    }
    if (!flags_used && p.flags_staged) HIP_TRY(c, hipMemsetAsync((char*)p.meta + stg->grp[3], 0, stg->grp[4] - stg->grp[3], hs));
    p.flags_staged = flags_used;
    if (!compact) HIP_TRY(c, hipMemcpyAsync(p.coef, stg->host + stg->meta_bytes, stg->coef_bytes, hipMemcpyHostToDevice, hs));
    p.h_slice_idx.assign(m->slice_idx, m->slice_idx + c->num_ctus);
    p.h_tile_idx.assign(m->tile_idx, m->tile_idx + c->num_ctus);
  } else {
    ProfScope ps(c, K_H2D);
    p.flags_staged = true;
    // ---- HM arrays of the CTU range (field-by-field, exactly the arrays TComDataCU owns)
#define STAGE(dst, src, elem_bytes)                                                                                       \
    if (src) HIP_TRY(c, hipMemcpyAsync((char*)(dst) + po * (elem_bytes), (const char*)(src) + po * (elem_bytes), pn * (elem_bytes), \
                                       hipMemcpyHostToDevice, hs));                                                \
    else HIP_TRY(c, hipMemsetAsync((char*)(dst) + po * (elem_bytes), 0, pn * (elem_bytes), hs))
    STAGE(p.dev.depth, m->depth, 1); STAGE(p.dev.part_size, m->part_size, 1); STAGE(p.dev.pred_mode, m->pred_mode, 1);
    STAGE(p.dev.qp, m->qp, 1); STAGE(p.dev.tr_idx, m->tr_idx, 1);
    for (int k = 0; k < 3; k++) { STAGE(p.dev.cbf[k], m->cbf[k], 1); STAGE(p.dev.tskip[k], m->transform_skip[k], 1); }
    for (int k = 0; k < 2; k++) { STAGE(p.dev.mv[k], m->mv[k], 4); STAGE(p.dev.ref_idx[k], m->ref_idx[k], 1); }
    if (p.dev.has_intra_dir) { STAGE(p.dev.intra_dir[0], m->intra_dir[0], 1); STAGE(p.dev.intra_dir[1], m->intra_dir[1], 1); }
    STAGE(p.dev.bypass, m->transquant_bypass, 1); STAGE(p.dev.ipcm, m->ipcm, 1);
#undef STAGE
    // per-CTU slice / tile index (the slice index of this call wins over a missing array)
    {
      // (the host mirrors are what the asynchronous copies read from: they live as long as the picture)
      p.h_slice_idx.resize(c->num_ctus);
      p.h_tile_idx.resize(c->num_ctus);
      for (int i = 0; i < num_ctus; i++) p.h_slice_idx[first_ctu + i] = m->slice_idx ? m->slice_idx[first_ctu + i] : (uint16_t)slice_idx;
      for (int i = 0; i < num_ctus; i++) p.h_tile_idx[first_ctu + i] = m->tile_idx ? m->tile_idx[first_ctu + i] : (uint16_t)0;
      HIP_TRY(c, h2d_small(c, (void*)(p.dev.slice_idx + first_ctu), p.h_slice_idx.data() + first_ctu, (size_t)num_ctus * 2, hs));
      HIP_TRY(c, h2d_small(c, (void*)(p.dev.tile_idx + first_ctu), p.h_tile_idx.data() + first_ctu, (size_t)num_ctus * 2, hs));
    }
    for (int k = 0; k < 3 && !compact; k++) {
      const size_t per = (size_t)(c->ctu * c->ctu) >> (k ? c->csx + c->csy : 0);
      HIP_TRY(c, hipMemcpyAsync((void*)(p.dev.coef[k] + first_ctu * per), co->level[k] + first_ctu * per, (size_t)num_ctus * per * 2,
                                hipMemcpyHostToDevice, hs));
    }
  }
  // cross-component prediction weights (4:4:4; m_crossComponentPredictionAlpha): device copies allocated with the first picture that carries them
  p.dev.ccp[0] = p.dev.ccp[1] = nullptr;
  if (c->fmt == 3 && m->ccp_alpha[0] && m->ccp_alpha[1]) {
    const size_t np = (size_t)c->num_ctus * c->parts;
    if (!p.ccp) HIP_TRY(c, hipMalloc(&p.ccp, 2 * np));
    for (int k = 0; k < 2; k++) {
      HIP_TRY(c, hipMemcpyAsync((char*)p.ccp + k * np + po, m->ccp_alpha[k] + po, pn, hipMemcpyHostToDevice, hs));
      p.dev.ccp[k] = (const int8_t*)p.ccp + k * np;
    }
  }
  // The caller's arrays are at hand: ONE pass over three of them (branch-free, so that the compiler vectorises it: ~1.5 MB per 2160p picture)
  // says whether the range holds intra CUs at all and how many (which intra kernel, if any: launch_intra) and whether it holds PUs that cut
  // an 8x8 luma tile -- 2NxN / Nx2N (/ NxN) parts of 8x8 CUs, the 4- and 12-sample parts of AMP in 16x16 CUs -- (the cells kernels).
  // (Round 4: the search for such PUs was a loop with an early exit over every 8x8 area; on pictures without them it walked all of them,
  // 0.2 ms of the calling thread per 2160p picture; this pass takes ~0.05.)
  size_t n_intra = 0;
  unsigned cells_u = 0;
  {
    // (byte lanes throughout -- 16 or 32 partitions per vector instruction --: the counts of a chunk of 192 stay below 256)
    const uint8_t d8 = (uint8_t)(c->seq.log2_ctu_size - 3), d8m = (uint8_t)(d8 - 1);
    const int8_t* __restrict ps = m->part_size + po;
    const uint8_t* __restrict dp = m->depth + po;
    const int8_t* __restrict pm = m->pred_mode + po;
    for (size_t base = 0; base < pn; base += 192) {
      const size_t n = std::min<size_t>(192, pn - base);
      uint8_t cnt = 0, cel = 0;
      for (size_t i = 0; i < n; i++) {
        const uint8_t ptn = (uint8_t)ps[base + i], d = dp[base + i];
        const uint8_t intra = (uint8_t)(pm[base + i] == HMGPU_MODE_INTRA);
        const uint8_t part = (uint8_t)((ptn != HMGPU_SIZE_2Nx2N) & (ptn != HMGPU_SIZE_NONE));
        const uint8_t small = (uint8_t)((d >= d8) | ((d == d8m) & (ptn >= HMGPU_SIZE_2NxnU)));
        cnt = (uint8_t)(cnt + intra);
        cel = (uint8_t)(cel | (part & (intra ^ 1) & small));
      }
      n_intra += cnt; cells_u |= cel;
    }
  }
  return finish_stage(c, cur, slice_idx, slices, any_wp, co->pcm_sample, any_pcm, any_bypass, first_ctu, num_ctus, n_intra, cells_u != 0, hs,
                      call_out);
}

// reference pictures named by the slice table entries `slices` of picture `cur`: their borders must be extended before the kernels read them
static hmgpu_status extend_refs_of(hmgpu_ctx* c, hmgpu_pic cur, const std::vector<int>& slices) {
  const Picture& p = c->pics[cur];
  for (int si : slices) {
    const SliceDev& sd = p.slices[si];
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < HMGPU_MAX_REF; r++)
        if (sd.ref_pic[l][r] >= 0) { hmgpu_status st = ensure_extended(c, sd.ref_pic[l][r]); if (st != HMGPU_OK) return st; }
  }
  return HMGPU_OK;
}

// staging + the reconstruction kernels of ONE call, everything on the context's stream
static hmgpu_status stage_and_run(hmgpu_ctx* c, hmgpu_pic cur, int32_t slice_idx, const std::vector<int>& slices, bool any_wp,
                                  const hmgpu_ctu_meta* m, const hmgpu_coeffs* co, int32_t first_ctu, int32_t num_ctus) {
  SliceCall call;
  hmgpu_status st = stage_inputs(c, cur, slice_idx, slices, any_wp, m, co, first_ctu, num_ctus, c->stream, &call);
  if (st == HMGPU_OK) st = extend_refs_of(c, cur, slices);
  if (st != HMGPU_OK) return st;
  Batch b; memset(&b, 0, sizeof(b));
  b.n = 1; b.pic[0] = cur; b.first_ctu[0] = first_ctu; b.num_ctus[0] = num_ctus;
  st = run_recon(c, b, call.intra, call.wp, call.cells, call.bi, call.islice);
  mark_use(c, b);
  return st;
}

static bool meta_complete(const hmgpu_ctu_meta* m, const hmgpu_coeffs* co) {
  return m && co && m->depth && m->part_size && m->pred_mode && m->qp && m->tr_idx && m->cbf[0] && m->cbf[1] && m->cbf[2] && m->mv[0] &&
         m->mv[1] && m->ref_idx[0] && m->ref_idx[1] && co->level[0] && co->level[1] && co->level[2];
}

static hmgpu_status reopen_picture(hmgpu_ctx* c, hmgpu_pic cur, hipStream_t hs) {
  Picture& p = c->pics[cur];
  filter_forget(p);                    // (whatever a filter call left belongs to what the handle held before this call)
  if (p.sao_applied) {                 // picture buffer decoded again without release/acquire: reconstruction planes again
    p.sao_applied = false; p.dev.sao_applied = 0;
    return push_final(c, cur, hs);
  }
  return HMGPU_OK;
}

hmgpu_status hmgpu_decompress_slice(hmgpu_ctx* c, hmgpu_pic cur, int32_t slice_idx, const hmgpu_slice_params* sl,
                                    const hmgpu_ctu_meta* m, const hmgpu_coeffs* co, int32_t first_ctu, int32_t num_ctus) {
  if (!c || !valid_pic(c, cur) || !sl || !meta_complete(m, co)) return HMGPU_EINVAL;
  if (first_ctu < 0 || num_ctus <= 0 || first_ctu + num_ctus > c->num_ctus) return HMGPU_EINVAL;
  hmgpu_status st = reopen_picture(c, cur, c->stream);
  if (st == HMGPU_OK) st = register_slice(c, cur, slice_idx, sl, c->stream);
  if (st != HMGPU_OK) return st;
  return stage_and_run(c, cur, slice_idx, std::vector<int>{slice_idx}, sl->weighted_pred != 0, m, co, first_ctu, num_ctus);
}

hmgpu_status hmgpu_decompress_picture(hmgpu_ctx* c, hmgpu_pic cur, int32_t num_slices, const hmgpu_slice_params* const* slices,
                                      const hmgpu_ctu_meta* m, const hmgpu_coeffs* co) {
  if (!c || !valid_pic(c, cur) || !slices || num_slices < 1 || num_slices > HMGPU_MAX_SLICES || !meta_complete(m, co)) return HMGPU_EINVAL;
  if (num_slices > 1 && !m->slice_idx) return HMGPU_EINVAL;
  if (m->slice_idx) for (int i = 0; i < c->num_ctus; i++) if (m->slice_idx[i] >= num_slices) return HMGPU_EINVAL;
  hmgpu_status st = reopen_picture(c, cur, c->stream);
  std::vector<int> all;
  bool any_wp = false;
  for (int i = 0; i < num_slices && st == HMGPU_OK; i++) {
    st = register_slice(c, cur, i, slices[i], c->stream);
    all.push_back(i);
    any_wp |= slices[i] && slices[i]->weighted_pred != 0;
  }
  if (st != HMGPU_OK) return st;
  return stage_and_run(c, cur, 0, all, any_wp, m, co, 0, c->num_ctus);
}

// HM's dense level arrays -> compact streams.  The same walk as k_prep's count (k_prep.hip): per 8x8 luma area in z-order, the TUs
// that originate there; a TU is coded iff its cbf bits are set down to its transform depth.
hmgpu_status hmgpu_pack_levels(const hmgpu_seq_params* seq, const hmgpu_ctu_meta* m, const hmgpu_coeffs* dense,
                               int16_t* const out_level[3], uint32_t* const out_start[3]) {
  if (!seq || !m || !dense || !out_level || !out_start || !m->depth || !m->part_size || !m->tr_idx || !m->cbf[0] || !m->cbf[1] || !m->cbf[2]) return HMGPU_EINVAL;
  for (int k = 0; k < 3; k++) if (!dense->level[k] || !out_level[k] || !out_start[k]) return HMGPU_EINVAL;
  if (seq->chroma_format > 1) return HMGPU_EUNSUPPORTED;       // (the compact form is defined for 4:2:0 / 4:0:0 pictures)
  const int log2ctu = seq->log2_ctu_size, ctu_sz = 1 << log2ctu, pw = ctu_sz / 4, parts = pw * pw;
  const int ctus_w = (seq->width + ctu_sz - 1) / ctu_sz, n_ctus = hmgpu_num_ctus(seq);
  uint32_t pos[3] = {0, 0, 0};
  for (int a = 0; a < n_ctus; a++) {
    const int cx = (a % ctus_w) * ctu_sz, cy = (a / ctus_w) * ctu_sz;
    for (int k = 0; k < 3; k++) out_start[k][a] = pos[k];
    for (int z0 = 0; z0 < parts; z0 += 4) {
      const size_t idx = (size_t)a * parts + z0;
      const int x4 = zscan_x(z0), y4 = zscan_y(z0);
      if (cx + 4 * x4 >= seq->width || cy + 4 * y4 >= seq->height || m->part_size[idx] == HMGPU_SIZE_NONE) continue;
      const int tr = m->tr_idx[idx], log2tu = log2ctu - m->depth[idx] - tr;
      if (log2tu > 5) continue;
      auto emit = [&](int comp, size_t src_off, uint32_t n) {
        memcpy(out_level[comp] + pos[comp], dense->level[comp] + src_off, n * sizeof(int16_t));
        pos[comp] += n;
      };
      const size_t base_l = (size_t)a * ctu_sz * ctu_sz, base_c = base_l / 4;
      if (log2tu > 2) {
        const int tu_parts = 1 << (log2tu - 2);
        if ((x4 & (tu_parts - 1)) || (y4 & (tu_parts - 1))) continue;
        if (cbf_coded(m->cbf[0][idx], tr)) emit(0, base_l + 16 * (size_t)z0, 1u << (2 * log2tu));
        if (cbf_coded(m->cbf[1][idx], tr)) emit(1, base_c + 4 * (size_t)z0, 1u << (2 * log2tu - 2));
        if (cbf_coded(m->cbf[2][idx], tr)) emit(2, base_c + 4 * (size_t)z0, 1u << (2 * log2tu - 2));
      } else {
        for (int j = 0; j < 4; j++) if (cbf_coded(m->cbf[0][idx + j], tr)) emit(0, base_l + 16 * (size_t)(z0 + j), 16);
        if (cbf_coded(m->cbf[1][idx], tr)) emit(1, base_c + 4 * (size_t)z0, 16);
        if (cbf_coded(m->cbf[2][idx], tr)) emit(2, base_c + 4 * (size_t)z0, 16);
      }
    }
  }
  for (int k = 0; k < 3; k++) out_start[k][n_ctus] = pos[k];
  return HMGPU_OK;
}

// ---- staging blocks
hmgpu_status hmgpu_staging_alloc(hmgpu_ctx* c, hmgpu_staging** out, hmgpu_ctu_meta* meta, hmgpu_coeffs* coeffs) {
  if (!c || !out || !meta || !coeffs) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  hmgpu_staging* st = new (std::nothrow) hmgpu_staging();
  if (!st) return HMGPU_ENOMEM;
  const size_t np = (size_t)c->num_ctus * c->parts;
  PicDev lay;
  memset(&lay, 0, sizeof(lay));
  { Carver m(nullptr); carve_meta(m, lay, np, c->num_ctus, st->grp); st->meta_bytes = m.off; }
  for (int k = 0; k < 3; k++) st->coef_bytes += align_up(c->coef_elems[k] * sizeof(int16_t), 256);
  st->start_bytes = align_up((size_t)3 * (c->num_ctus + 1) * sizeof(uint32_t), 256);
  const size_t total = st->meta_bytes + st->coef_bytes + st->start_bytes;
  // (portable: every device of the process may copy from the block -- hmgpu_staging_share)
  if (hipHostMalloc((void**)&st->host, total, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); delete st; return HMGPU_ENOMEM; }
  st->owner = c;
  memset(st->host, 0, total);
  { Carver m(st->host); carve_meta(m, lay, np, c->num_ctus); }
  hmgpu_ctu_meta& h = st->m;
  memset(&h, 0, sizeof(h));
  h.depth = lay.depth; h.part_size = lay.part_size; h.pred_mode = lay.pred_mode; h.qp = lay.qp; h.tr_idx = lay.tr_idx;
  for (int k = 0; k < 3; k++) { h.cbf[k] = lay.cbf[k]; h.transform_skip[k] = lay.tskip[k]; }
  for (int k = 0; k < 2; k++) { h.mv[k] = lay.mv[k]; h.ref_idx[k] = lay.ref_idx[k]; h.intra_dir[k] = lay.intra_dir[k]; }
  h.transquant_bypass = lay.bypass; h.ipcm = lay.ipcm; h.slice_idx = lay.slice_idx; h.tile_idx = lay.tile_idx;
  // (decoded nowhere yet: HM marks that with part_size = NUMBER_OF_PART_SIZES and ref_idx = -1)
  memset(const_cast<int8_t*>(h.part_size), HMGPU_SIZE_NONE, np);
  memset(const_cast<int8_t*>(h.ref_idx[0]), 0xff, np); memset(const_cast<int8_t*>(h.ref_idx[1]), 0xff, np);
  memset(&st->co, 0, sizeof(st->co));
  { Carver m(st->host + st->meta_bytes); for (int k = 0; k < 3; k++) st->co.level[k] = m.take<int16_t>(c->coef_elems[k]); }
  for (int k = 0; k < 3; k++) st->co.ctu_level_start[k] = reinterpret_cast<const uint32_t*>(st->host + st->meta_bytes + st->coef_bytes) + (size_t)k * (c->num_ctus + 1);
  c->stagings.push_back(st);
  *meta = st->m; *coeffs = st->co; *out = st;
  return HMGPU_OK;
}

// the block may be rewritten once the copies of the call that last read it have been made (events of the copy stream are recorded in
// order: one that has since been re-recorded stands for a later point of the same stream)
hmgpu_status hmgpu_staging_wait(hmgpu_ctx* c, hmgpu_staging* st) {
  if (!c || !st) return HMGPU_EINVAL;
  if (st->copy_seq == 0) return HMGPU_OK;
  hmgpu_ctx* r = st->reader ? st->reader : c;              // the context whose copy stream read the block last
  hipSetDevice(r->device);
  if (hipEventSynchronize(r->copy_ev[st->copy_seq % 8]) != hipSuccess) return HMGPU_EDEVICE;
  return HMGPU_OK;
}

// A decoder that places pictures on several contexts parses into ONE set of blocks and decides late which context decodes a picture:
// `other` -- a context of the same geometry, on any device -- recognises the block's arrays from now on as `owner` does.
hmgpu_status hmgpu_staging_share(hmgpu_ctx* owner, hmgpu_staging* st, hmgpu_ctx* other) {
  if (!owner || !st || !other || st->owner != owner) return HMGPU_EINVAL;
  if (other == owner || std::find(st->sharers.begin(), st->sharers.end(), other) != st->sharers.end()) return HMGPU_OK;
  const hmgpu_seq_params &a = owner->seq, &b = other->seq;
  if (a.width != b.width || a.height != b.height || a.log2_ctu_size != b.log2_ctu_size || a.chroma_format != b.chroma_format ||
      owner->num_ctus != other->num_ctus || owner->parts != other->parts) return HMGPU_EINVAL;
  for (int k = 0; k < 3; k++) if (owner->coef_elems[k] != other->coef_elems[k]) return HMGPU_EINVAL;
  st->sharers.push_back(other);
  other->shared_stagings.push_back(st);
  return HMGPU_OK;
}

void hmgpu_staging_free(hmgpu_ctx* c, hmgpu_staging* st) {
  if (!c || !st) return;
  hipSetDevice(c->device);
  if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (st->reader && st->reader != c && st->reader->copy_stream) { hipSetDevice(st->reader->device); (void)hipStreamSynchronize(st->reader->copy_stream); }
  for (hmgpu_ctx* o : st->sharers) o->shared_stagings.erase(std::remove(o->shared_stagings.begin(), o->shared_stagings.end(), st), o->shared_stagings.end());
  c->stagings.erase(std::remove(c->stagings.begin(), c->stagings.end(), st), c->stagings.end());
  if (st->host) (void)hipHostFree(st->host);
  delete st;
}

// the copy stream may overwrite a picture's input arrays once the kernels that last read them have finished
static void wait_for_last_use(hmgpu_ctx* c, const Picture& p, hipStream_t hs) {
  if (!p.last_use) return;
  // (events older than the ring are gone: the newest one was recorded later and is a safe stand-in)
  const uint64_t seq = c->use_seq - p.last_use < 8 ? p.last_use : c->use_seq;
  (void)hipStreamWaitEvent(hs, c->use_ev[seq % 8], 0);
}

}  // extern "C"

// What the batch decompress entries share: n independent pictures, staged on the two copy lanes beside the kernels of the call before,
// then one set of reconstruction launches.  The entry brings four callables -- check(): its own refusals, behind the shared ones;
// stage(i, slices, wp, hs, &call): the inputs of picture i onto its lane; copied(): its record of what this pass of copies read,
// made in front of the pass's event; expand(): what it launches once the context's stream waits for the copies, in front of the kernels.
template <typename Job, typename Check, typename Stage, typename Copied, typename Expand>
static hmgpu_status decompress_batch(hmgpu_ctx* c, int32_t n, const Job* jobs, Check check, Stage stage, Copied copied, Expand expand) {
  if (!c || !jobs || n < 1 || n > kMaxBatch) return HMGPU_EINVAL;
  c->host_calls++;
  { HostTimer tv(c, 0);
  // everything is checked before anything is enqueued
  for (int i = 0; i < n; i++) {
    const Job& j = jobs[i];
    if (!valid_pic(c, j.pic) || !j.slices || j.num_slices < 1 || j.num_slices > HMGPU_MAX_SLICES) return HMGPU_EINVAL;
    for (int k = 0; k < i; k++) if (jobs[k].pic == j.pic) return HMGPU_EINVAL;
    // independent pictures only: none of them may be a reference of another one of the call
    for (int s2 = 0; s2 < j.num_slices; s2++)
      for (int l = 0; l < 2 && j.slices[s2]; l++)
        for (int r = 0; r < j.slices[s2]->num_ref_idx[l] && r < HMGPU_MAX_REF; r++)
          for (int k = 0; k < n; k++) if (j.slices[s2]->ref_pic[l][r] == jobs[k].pic) return HMGPU_EINVAL;
  }
  { const hmgpu_status st = check(); if (st != HMGPU_OK) return st; }
  }
  hipSetDevice(c->device);
  Batch b; memset(&b, 0, sizeof(b));
  b.n = n;
  bool any_intra = false, any_wp = false, any_cells = false, any_bi = false, any_islice = false;
  hmgpu_status st = HMGPU_OK;
  std::vector<std::vector<int>> all(n);
  {
    ProfScope ps(c, K_H2D);              // (events on the compute stream: the staging itself runs beside it on the copy stream)
    // (no path leaves this loop but through the join below: an error sets st and ends the loop)
    for (int i = 0; i < n && st == HMGPU_OK; i++) {
      const Job& j = jobs[i];
      Picture& p = c->pics[j.pic];
      const hipStream_t hs = (i & 1) ? c->copy_stream2 : c->copy_stream;       // two copy lanes: two DMA engines
      wait_for_last_use(c, p, hs);
      st = reopen_picture(c, j.pic, hs);
      bool wp = false;
      { HostTimer ts(c, 1);
      for (int k = 0; k < j.num_slices && st == HMGPU_OK; k++) {
        st = register_slice(c, j.pic, k, j.slices[k], hs);
        all[i].push_back(k);
        wp |= j.slices[k] && j.slices[k]->weighted_pred != 0;
      }
      }
      SliceCall call;
      HostTimer ti(c, 2);
      if (st == HMGPU_OK) st = stage(i, all[i], wp, hs, &call);
      if (st != HMGPU_OK) break;
      b.pic[i] = j.pic; b.first_ctu[i] = 0; b.num_ctus[i] = c->num_ctus;
      any_intra |= call.intra; any_wp |= call.wp; any_cells |= call.cells; any_bi |= call.bi; any_islice |= call.islice;
    }
    if (n > 1) {                        // (also after an error: whatever the second lane was given is ordered in front of the next event of the first)
      (void)hipEventRecord(c->copy_join, c->copy_stream2);
      (void)hipStreamWaitEvent(c->copy_stream, c->copy_join, 0);
    }
    if (st != HMGPU_OK) return st;
    c->copy_seq++;
    copied();
    HIP_TRY(c, hipEventRecord(c->copy_ev[c->copy_seq % 8], c->copy_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->copy_ev[c->copy_seq % 8], 0));
  }
  HostTimer tr(c, 3);
  st = expand();
  if (st != HMGPU_OK) return st;
  for (int i = 0; i < n && st == HMGPU_OK; i++) st = extend_refs_of(c, jobs[i].pic, all[i]);
  if (st == HMGPU_OK) st = run_recon(c, b, any_intra, any_wp, any_cells, any_bi, any_islice);
  mark_use(c, b);
  return st;
}

extern "C" {

hmgpu_status hmgpu_decompress_pictures(hmgpu_ctx* c, int32_t n, const hmgpu_picture_job* jobs) {
  auto check = [&]() -> hmgpu_status {
    for (int i = 0; i < n; i++) {
      const hmgpu_picture_job& j = jobs[i];
      if (!meta_complete(j.meta, j.coeffs)) return HMGPU_EINVAL;
      if (j.num_slices > 1 && !j.meta->slice_idx) return HMGPU_EINVAL;
      if (j.meta->slice_idx) for (int k = 0; k < c->num_ctus; k++) if (j.meta->slice_idx[k] >= j.num_slices) return HMGPU_EINVAL;
    }
    return HMGPU_OK;
  };
  auto stage = [&](int i, const std::vector<int>& slices, bool wp, hipStream_t hs, SliceCall* call) {
    return stage_inputs(c, jobs[i].pic, 0, slices, wp, jobs[i].meta, jobs[i].coeffs, 0, c->num_ctus, hs, call);
  };
  auto copied = [&] {                                    // the staging blocks this pass read (hmgpu_staging_wait)
    for (int i = 0; i < n; i++)
      if (const hmgpu_staging* sb = staging_of(c, jobs[i].meta, jobs[i].coeffs)) { const_cast<hmgpu_staging*>(sb)->copy_seq = c->copy_seq; const_cast<hmgpu_staging*>(sb)->reader = c; }
  };
  return decompress_batch(c, n, jobs, check, stage, copied, [] { return HMGPU_OK; });
}

// ---- packed input (include/hmgpu.h "packed input"): validated here, copied in one DMA, expanded by k_unpack.hip
static hmgpu_status stage_packed(hmgpu_ctx* c, const hmgpu_packed_job& j, const packed::Summary& sm, const std::vector<int>& slices,
                                 bool any_wp, hipStream_t hs, SliceCall* call_out) {
  Picture& p = c->pics[j.pic];
  if (!p.blob) HIP_TRY(c, hipMalloc(&p.blob, hmgpu_packed_max_bytes(&c->seq)));
  HIP_TRY(c, hipMemcpyAsync(p.blob, j.blob, j.bytes, hipMemcpyHostToDevice, hs));
  // what stage_inputs derives from the arrays, from the runs (packed::validate): the same values, so that the same kernels are chosen
  p.dev.has_intra_dir = (sm.groups >> packed::G_INTRA) & 1;
  for (int k = 0; k < 3; k++) p.dev.coef_start[k] = p.coef_start + (size_t)k * (c->num_ctus + 1);
  p.flags_staged = sm.flags_used;           // (the expansion writes the transform-skip / lossless / PCM flags of every partition)
  p.h_slice_idx.resize(c->num_ctus);
  p.h_tile_idx.resize(c->num_ctus);
  for (int a = 0; a < c->num_ctus; a++) { p.h_slice_idx[a] = (uint16_t)(sm.ctu[a] & 0xffff); p.h_tile_idx[a] = (uint16_t)(sm.ctu[a] >> 16); }
  p.dev.ccp[0] = p.dev.ccp[1] = nullptr;
  return finish_stage(c, j.pic, 0, slices, any_wp, j.pcm_sample, sm.any_pcm, sm.any_bypass, 0, c->num_ctus, sm.n_intra, sm.cells, hs, call_out);
}

hmgpu_status hmgpu_decompress_pictures_packed(hmgpu_ctx* c, int32_t n, const hmgpu_packed_job* jobs) {
  const bool args_ok = c && jobs && n >= 1 && n <= kMaxBatch;              // (decompress_batch refuses the call when they are not)
  if (args_ok && c->seq.chroma_format > 1) return HMGPU_EUNSUPPORTED;      // in front of every other refusal
  std::vector<packed::Summary> sums(args_ok ? n : 0);
  UnpackArgs ua; memset(&ua, 0, sizeof(ua));
  ua.n = n;
  // every blob is checked before anything is enqueued: the device expansion trusts what passed
  auto check = [&]() -> hmgpu_status {
    for (int i = 0; i < n; i++) if (!jobs[i].blob) return HMGPU_EINVAL;
    // every blob in full (the walk over the level positions included: ~1.1 M of them per 2160p picture, a few tenths of a millisecond),
    // the blobs of a call side by side on threads of their own
    {
      std::vector<hmgpu_status> vs(n, HMGPU_OK);
      std::vector<std::thread> th;
      for (int i = 1; i < n; i++) {
        auto one = [&, i] { vs[i] = packed::validate(&c->seq, jobs[i].blob, jobs[i].bytes, &sums[i], true); };
        try { th.emplace_back(one); } catch (...) { one(); }      // (no thread to be had: on this one)
      }
      vs[0] = packed::validate(&c->seq, jobs[0].blob, jobs[0].bytes, &sums[0], true);
      for (std::thread& t : th) t.join();
      for (int i = 0; i < n; i++) if (vs[i] != HMGPU_OK) return vs[i];
    }
    for (int i = 0; i < n; i++) {
      const hmgpu_packed_job& j = jobs[i];
      const packed::Summary& sm = sums[i];
      if (sm.max_slice >= (uint32_t)j.num_slices) return HMGPU_EINVAL;
      if (sm.any_pcm && (!j.pcm_sample[0] || !j.pcm_sample[1] || !j.pcm_sample[2] || !((sm.groups >> packed::G_INTRA) & 1))) return HMGPU_EINVAL;
      if (sm.any_pcm && (c->seq.pcm_bit_depth_luma < 1 || c->seq.pcm_bit_depth_luma > c->seq.bit_depth_luma ||
                         c->seq.pcm_bit_depth_chroma < 1 || c->seq.pcm_bit_depth_chroma > c->seq.bit_depth_chroma)) return HMGPU_EINVAL;
    }
    return HMGPU_OK;
  };
  auto stage = [&](int i, const std::vector<int>& slices, bool wp, hipStream_t hs, SliceCall* call) {
    const hmgpu_status st = stage_packed(c, jobs[i], sums[i], slices, wp, hs, call);
    if (st == HMGPU_OK) { ua.pic[i] = jobs[i].pic; ua.blob[i] = (const char*)c->pics[jobs[i].pic].blob; }
    return st;
  };
  auto copied = [&] {                                    // the blobs this pass read (hmgpu_packed_wait)
    // the oldest pass the event ring still stands for: once its event has passed, every copy of that pass and before it is done
    if (c->copy_seq > 8 && hipEventQuery(c->copy_ev[(c->copy_seq - 7) % 8]) == hipSuccess)
      for (auto it = c->packed_reads.begin(); it != c->packed_reads.end();) it = it->second <= c->copy_seq - 7 ? c->packed_reads.erase(it) : std::next(it);
    for (int i = 0; i < n; i++) c->packed_reads[jobs[i].blob] = c->copy_seq;
  };
  auto expand = [&]() -> hmgpu_status {
    { ProfScope ps(c, K_UNPACK); launch_unpack_input(c->d_pics, ua, c->num_ctus, c->stream); }
    HIP_TRY(c, hipGetLastError());
    return HMGPU_OK;
  };
  return decompress_batch(c, n, jobs, check, stage, copied, expand);
}

hmgpu_status hmgpu_packed_wait(hmgpu_ctx* c, const void* blob) {
  if (!c || !blob) return HMGPU_EINVAL;
  const auto it = c->packed_reads.find(blob);
  if (it == c->packed_reads.end()) return HMGPU_OK;           // never read, or its copy is known to be done
  hipSetDevice(c->device);
  // (the ring of copy events holds the last 8 passes; an older pass is behind the newest event)
  const uint64_t seq = c->copy_seq - it->second < 8 ? it->second : c->copy_seq;
  if (hipEventSynchronize(c->copy_ev[seq % 8]) != hipSuccess) return HMGPU_EDEVICE;
  return HMGPU_OK;
}

// SAO parameters of one picture, with the slice / tile index per CTU as handed over with the slices (host mirrors: no device round
// trip, the stream keeps running)
static hmgpu_status stage_sao_of(hmgpu_ctx* c, Picture& p, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao) {
  std::vector<uint16_t> sidx = p.h_slice_idx, tidx = p.h_tile_idx;
  sidx.resize(c->num_ctus, 0);
  tidx.resize(c->num_ctus, 0);
  return stage_sao(c, p, pp, sao, sidx, tidx);
}

// SAOProcess ran: the SAO planes are the picture now (HM: resYuv written in place after the snapshot copy)
static hmgpu_status sao_became_picture(hmgpu_ctx* c, hmgpu_pic pic) {
  Picture& p = c->pics[pic];
  p.sao_applied = true; p.dev.sao_applied = 1;
  hmgpu_status st = push_final(c, pic, c->stream);
  if (st == HMGPU_OK) st = push_picdev(c, pic);
  return st;
}

hmgpu_status hmgpu_filter_pictures(hmgpu_ctx* c, int32_t n, const hmgpu_filter_job* jobs) {
  if (!c || !jobs || n < 1 || n > kMaxBatch) return HMGPU_EINVAL;
  for (int i = 0; i < n; i++) {
    if (!valid_pic(c, jobs[i].pic) || !jobs[i].pp) return HMGPU_EINVAL;
    if (jobs[i].pp->sao_enabled && !jobs[i].sao) return HMGPU_EINVAL;
    for (int k = 0; k < i; k++) if (jobs[k].pic == jobs[i].pic) return HMGPU_EINVAL;
  }
  hipSetDevice(c->device);
  Batch b; memset(&b, 0, sizeof(b));
  b.n = n;
  { HostTimer tsao(c, 4);
  for (int i = 0; i < n; i++) {
    Picture& p = c->pics[jobs[i].pic];
    p.sao_any = false;
    if (jobs[i].pp->sao_enabled) {
      hmgpu_status st = stage_sao_of(c, p, jobs[i].pp, jobs[i].sao);
      if (st != HMGPU_OK) return st;
    }
    p.filter_ready = true;
    p.lf_called = true; p.lf_sao = jobs[i].pp->sao_enabled != 0;
    b.pic[i] = jobs[i].pic; b.first_ctu[i] = 0; b.num_ctus[i] = c->num_ctus;
  }
  }
  HostTimer tf(c, 5);
  bool fused = false;
  hmgpu_status st = run_filter(c, b, 7, &fused);
  if (st != HMGPU_OK) return st;
  for (int i = 0; i < n && st == HMGPU_OK; i++) {
    Picture& p = c->pics[jobs[i].pic];
    if (p.sao_any) st = sao_became_picture(c, jobs[i].pic);
    p.extended = true;                   // (the fused kernel's border tiles, or the batched border extension below)
  }
  if (st != HMGPU_OK) return st;
  if (!fused) {
    { ProfScope ps(c, K_EXTEND); launch_extend(c->d_pics, b, c->seq.width, c->seq.height, c->mx[0], c->my[0], c->csx, c->csy, c->stream); }
    HIP_TRY(c, hipGetLastError());
  }
  mark_use(c, b);
  return HMGPU_OK;
}

hmgpu_status hmgpu_filter_picture_stages(hmgpu_ctx* c, hmgpu_pic cur, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao,
                                         int32_t stages) {
  if (!c || !valid_pic(c, cur) || !pp) return HMGPU_EINVAL;
  if ((stages & 4) && pp->sao_enabled && !sao) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  Picture& p = c->pics[cur];
  p.sao_any = false;
  if ((stages & 4) && pp->sao_enabled) {
    hmgpu_status st = stage_sao_of(c, p, pp, sao);
    if (st != HMGPU_OK) return st;
  }
  p.filter_ready = true;
  p.lf_called = true; p.lf_sao = (stages & 4) && pp->sao_enabled;
  Batch b; memset(&b, 0, sizeof(b));
  b.n = 1; b.pic[0] = cur; b.first_ctu[0] = 0; b.num_ctus[0] = c->num_ctus;
  bool fused = false;
  hmgpu_status st = run_filter(c, b, stages, &fused);
  if (st != HMGPU_OK) return st;
  if ((stages & 4) && p.sao_any) {
    st = sao_became_picture(c, cur);
    if (st != HMGPU_OK) return st;
  }
  if (!fused) p.extended = false;        // (the fused kernel wrote the margins: nothing to launch)
  st = ensure_extended(c, cur);          // the finished picture is ready to be referenced
  commit_use(c);
  return st;
}

hmgpu_status hmgpu_filter_picture(hmgpu_ctx* c, hmgpu_pic cur, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao) {
  return hmgpu_filter_picture_stages(c, cur, pp, sao, 7);
}

}  // extern "C"
