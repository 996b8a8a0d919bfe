// hmgpu_api.hip -- core of the host runtime of libhmgpu.so: the context and its event rings, device pictures (the DPB lives in HBM),
// kernel sequencing (run_recon, run_filter, stage_sao), stats / profiling / replay and the KAT entry points.  Input staging, output and
// export live in hmgpu_input.hip, hmgpu_output.hip, hmgpu_export.hip, hmgpu_side.hip and hmgpu_analysis.hip; hmgpu_host.h holds what the units share.
//
// Host-side counterpart of TDecGop/TDecSlice/TDecCu's control flow (TDecGop.cpp:105-217), reduced to what is left
// once every traversal runs on the device: copy arrays, launch kernels, keep per-picture state.  The only serial
// host computation is reconstructBlkSAOParams' merge resolution (a dependent chain over CTUs, 3 x num_ctus items).
#include "hmgpu_host.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <new>
#include <vector>

namespace hmgpu_host __attribute__((visibility("hidden"))) {

// host -> device copy of a small structure on stream hs: through the context's page-locked ring (hmgpu_ctx::bounce) when it fits
hipError_t h2d_small(hmgpu_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t hs, bool* staged) {
  const size_t need = (bytes + 63) & ~(size_t)63;
  if (staged) *staged = false;
  if (!c->bounce || need > hmgpu_ctx::kBounceSeg) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, hs);
  if (staged) *staged = true;
  if (c->bounce_off + need > hmgpu_ctx::kBounceSeg) {
    hipStream_t streams[3] = {c->stream, c->copy_stream, c->copy_stream2};
    for (int k = 0; k < 3; k++) (void)hipEventRecord(c->bounce_ev[c->bounce_seg][k], streams[k]);
    c->bounce_used[c->bounce_seg] = true;
    c->bounce_seg = (c->bounce_seg + 1) % hmgpu_ctx::kBounceSegs;
    c->bounce_off = 0;
    if (c->bounce_used[c->bounce_seg]) for (int k = 0; k < 3; k++) (void)hipEventSynchronize(c->bounce_ev[c->bounce_seg][k]);
  }
  char* at = c->bounce + (size_t)c->bounce_seg * hmgpu_ctx::kBounceSeg + c->bounce_off;
  memcpy(at, src, bytes);
  c->bounce_off += need;
  return hipMemcpyAsync(dst, at, bytes, hipMemcpyHostToDevice, hs);
}


size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// device scratch of the output side: one allocation that lives with the context (hipMalloc / hipFree per call are device-wide
// synchronisations on the per-picture output path)
void* ctx_scratch(hmgpu_ctx* c, size_t bytes) {
  if (bytes > c->scratch_bytes) {
    if (c->scratch) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->scratch); c->scratch = nullptr; c->scratch_bytes = 0; }
    const size_t want = align_up(bytes + bytes / 4, 1 << 20);
    if (hipMalloc(&c->scratch, want) != hipSuccess) { c->scratch = nullptr; return nullptr; }
    c->scratch_bytes = want;
  }
  return c->scratch;
}

// after a synchronisation: did an intra wavefront give up waiting (k_intra.hip)?  The flag is sticky on the device until read here.
hmgpu_status check_faults(hmgpu_ctx* c) {
  hmgpu_status st = HMGPU_OK;
  for (int pic : c->intra_launched) {
    uint32_t f = 0;
    if (hipMemcpy(&f, c->pics[pic].dev.fault, 4, hipMemcpyDeviceToHost) != hipSuccess) { st = HMGPU_EDEVICE; continue; }
    if (f) { (void)hipMemset(c->pics[pic].dev.fault, 0, 4); c->last_err = -2; st = HMGPU_EDEVICE; }
  }
  c->intra_launched.clear();
  return st;
}

// Which submission last enqueued work on a picture, in ANY role (decoded, filtered, read as a reference, downloaded, hashed): the copy
// stream of hmgpu_decompress_pictures may rewrite a picture's descriptors and input arrays only behind that point.  Every entry point
// names the pictures it touches and ends with commit_use (one event on the context's stream).
void touch(hmgpu_ctx* c, int pic) { c->touched.push_back(pic); }
void commit_use(hmgpu_ctx* c) {
  if (c->touched.empty()) return;
  c->use_seq++;
  (void)hipEventRecord(c->use_ev[c->use_seq % 8], c->stream);
  for (int pic : c->touched) c->pics[pic].last_use = c->use_seq;
  c->touched.clear();
}

// profiling: a pair of events around one launch, resolved lazily
void prof_begin(hmgpu_ctx* c, int kind, EventPair* ep) {
  if (!c->profiling) return;
  if (c->free_events.empty()) {
    hipEventCreate(&ep->a); hipEventCreate(&ep->b);
  } else { *ep = c->free_events.back(); c->free_events.pop_back(); }
  ep->kind = kind;
  hipEventRecord(ep->a, c->stream);
}
void prof_end(hmgpu_ctx* c, EventPair* ep) {
  if (!c->profiling) return;
  hipEventRecord(ep->b, c->stream);
  c->pending.push_back(*ep);
}
void prof_drain(hmgpu_ctx* c) {
  for (EventPair& ep : c->pending) {
    float ms = 0.f;
    hipEventSynchronize(ep.b);
    if (hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) { c->kernel_ms[ep.kind] += ms; c->kernel_launches[ep.kind]++; }
    c->free_events.push_back(ep);
  }
  c->pending.clear();
}

// the raw HM arrays of one picture inside one block (device allocation; staging blocks mirror it, so that one copy moves them all).
// Order: what every picture needs first, then the groups a picture may do without -- list 1 (P slices), intra modes (no intra CUs),
// transform skip / lossless / PCM flags -- so that a copy from a staging block moves a prefix, or a prefix and one more piece.
// grp[0..4]: byte offsets where the groups start / the block ends.
void carve_meta(Carver& m, PicDev& d, size_t np, int num_ctus, size_t* grp) {
  size_t g[5];
  g[0] = m.off;
  d.slice_idx = m.take<uint16_t>(num_ctus); d.tile_idx = m.take<uint16_t>(num_ctus);
  d.depth = m.take<uint8_t>(np); d.part_size = m.take<int8_t>(np); d.pred_mode = m.take<int8_t>(np);
  d.qp = m.take<int8_t>(np); d.tr_idx = m.take<uint8_t>(np);
  for (int k = 0; k < 3; k++) d.cbf[k] = m.take<uint8_t>(np);
  d.mv[0] = m.take<int16_t>(np * 2); d.ref_idx[0] = m.take<int8_t>(np);
  g[1] = m.off;
  d.mv[1] = m.take<int16_t>(np * 2); d.ref_idx[1] = m.take<int8_t>(np);
  g[2] = m.off;
  for (int k = 0; k < 2; k++) d.intra_dir[k] = m.take<uint8_t>(np);
  g[3] = m.off;
  for (int k = 0; k < 3; k++) d.tskip[k] = m.take<uint8_t>(np);
  d.bypass = m.take<uint8_t>(np); d.ipcm = m.take<uint8_t>(np);
  g[4] = m.off;
  if (grp) memcpy(grp, g, sizeof(g));
}

hmgpu_status push_picdev(hmgpu_ctx* c, int pic) {
  HIP_TRY(c, h2d_small(c, c->d_pics + pic, &c->pics[pic].dev, sizeof(PicDev), c->stream));
  return HMGPU_OK;
}
hmgpu_status push_final(hmgpu_ctx* c, int pic, hipStream_t hs) {
  Picture& p = c->pics[pic];
  for (int k = 0; k < 3; k++) c->h_finals[pic].p[k] = p.sao_applied ? p.dev.sao[k] : p.dev.rec[k];
  HIP_TRY(c, h2d_small(c, c->d_finals + pic, &c->h_finals[pic], sizeof(PlaneSet), hs));
  return HMGPU_OK;
}

bool valid_pic(const hmgpu_ctx* c, hmgpu_pic pic) { return pic >= 0 && pic < (int)c->pics.size() && c->pics[pic].in_use; }

// the record of which CTUs of a picture carry staged side information (Picture::covered)
void coverage_clear(Picture& p) { p.covered.clear(); p.covered_ctus = 0; }
void coverage_add(const hmgpu_ctx* c, Picture& p, int first_ctu, int num_ctus) {
  if (p.covered.empty()) p.covered.assign((size_t)c->num_ctus, false);
  for (int a = first_ctu; a < first_ctu + num_ctus; a++)
    if (!p.covered[(size_t)a]) { p.covered[(size_t)a] = true; p.covered_ctus++; }
}

// lazy border extension, as HM does when a picture first enters a reference list (TComSlice.cpp:350: extendPicBorder)
hmgpu_status ensure_extended(hmgpu_ctx* c, int pic) {
  Picture& p = c->pics[pic];
  touch(c, pic);                        // (called for every reference picture of a submission)
  if (p.extended) return HMGPU_OK;
  Batch b; memset(&b, 0, sizeof(b));
  b.n = 1; b.pic[0] = pic;
  { ProfScope ps(c, K_EXTEND); launch_extend(c->d_pics, b, c->seq.width, c->seq.height, c->mx[0], c->my[0], c->csx, c->csy, c->stream); }
  HIP_TRY(c, hipGetLastError());
  p.extended = true;
  return HMGPU_OK;
}

}  // namespace hmgpu_host

namespace {

const char* const kKernelNames[HMGPU_NUM_KERNELS] = {"prep", "mc_luma", "mc_chroma", "itx", "deblock_ver", "deblock_hor", "sao",
                                                     "extend_border", "h2d_stage", "intra", "filter_fused", "unpack", "mc_cells"};    // mc_cells: the launches of k_mc_cells.hip, inside the mc_luma / mc_chroma spans

// one set of planes of a picture: luma, then the plane that holds Cb and Cr
size_t plane_set_bytes(const hmgpu_ctx* c) {
  size_t n = 0;
  for (int k = 0; k < 2; k++) n += align_up((size_t)c->pitch[k] * c->rows[k] * sizeof(int16_t), 256);
  return n;
}

hmgpu_status alloc_picture(hmgpu_ctx* c, Picture& p) {
  const hmgpu_seq_params& s = c->seq;
  const size_t plane_bytes = c->plane_bytes;
  p.planes = c->plane_slab + (size_t)(&p - c->pics.data()) * 2 * plane_bytes;     // (zeroed with the slab)
  const size_t np = (size_t)c->num_ctus * c->parts;
  // raw metadata: 11 byte arrays + 2 mv arrays (4 B) + 2 ref_idx + slice/tile idx
  for (int pass = 0; pass < 2; pass++) {
    Carver m(pass ? p.meta : nullptr);
    carve_meta(m, p.dev, np, c->num_ctus);
    if (!pass) { HIP_TRY(c, hipMalloc(&p.meta, m.off)); HIP_TRY(c, hipMemset(p.meta, 0, m.off)); }
  }
  {
    size_t bytes = 0;
    for (int k = 0; k < 3; k++) bytes += align_up(c->coef_elems[k] * sizeof(int16_t), 256);
    HIP_TRY(c, hipMalloc(&p.coef, bytes));
    HIP_TRY(c, hipMemset(p.coef, 0, bytes));
    Carver m(p.coef);
    for (int k = 0; k < 3; k++) p.dev.coef[k] = m.take<int16_t>(c->coef_elems[k]);
  }
  for (int pass = 0; pass < 2; pass++) {
    Carver m(pass ? p.derived : nullptr);
    PicDev& d = p.dev;
    d.blk = m.take<BlkInfo>((size_t)c->grid_w * c->grid_h);
    d.edges = m.take<EdgeRec>((size_t)(c->grid_w / 2) * (c->grid_h / 2));
    d.tmv = m.take<TileMv>((size_t)(c->grid_w / 2) * (c->grid_h / 2));
    for (int k = 0; k < 3; k++) d.resid[k] = m.take<int16_t>(c->coef_elems[k]);
    p.coef_start = m.take<uint32_t>((size_t)3 * (c->num_ctus + 1));
    d.fault = m.take<uint32_t>(1);
    for (int k = 0; k < 4; k++) d.tu[k] = m.take<TuRec>((size_t)c->tu_cap[k] * kTuShards);
    d.tu_count = m.take<uint32_t>(4 * kTuShards);
    d.tu_work = m.take<uint32_t>(4 * kTuShards + 1);
    d.stats = m.take<unsigned long long>(2 * kTuShards);
    d.saoprm = m.take<SaoDev>((size_t)c->num_ctus * 3);
    d.slices = m.take<SliceDev>(HMGPU_MAX_SLICES);
    d.ctu_intra = m.take<uint8_t>((size_t)c->num_ctus);
    p.sl_table = m.take<uint8_t>(4 * 6 * 1024);
    d.intra_done = m.take<uint32_t>((size_t)3 * c->num_ctus);
    if (!pass) { HIP_TRY(c, hipMalloc(&p.derived, m.off)); HIP_TRY(c, hipMemset(p.derived, 0, m.off)); }
  }
  PicDev& d = p.dev;
  d.width = s.width; d.height = s.height;
  d.bd[0] = s.bit_depth_luma; d.bd[1] = d.bd[2] = s.bit_depth_chroma;
  d.log2ctu = s.log2_ctu_size; d.ctus_w = c->ctus_w; d.ctus_h = c->ctus_h; d.num_ctus = c->num_ctus; d.parts = c->parts; d.pw = c->pw;
  for (int k = 0; k < 3; k++) d.pitch[k] = c->pitch[k];
  d.grid_w = c->grid_w; d.grid_h = c->grid_h;
  d.lf_across_tiles = 1; d.sao_applied = 0;
  d.has_intra_dir = 0; d.strong_intra_smoothing = s.strong_intra_smoothing ? 1 : 0;
  d.range_ext = s.range_ext_flags;
  d.mono = s.chroma_format == 0 ? 1 : 0;
  d.fmt = c->fmt; d.csx = c->csx; d.csy = c->csy;
  d.ccp[0] = d.ccp[1] = nullptr;
  d.debug_skip_ctu = -1;
  d.sl_m = nullptr;
  for (int k = 0; k < 3; k++) { d.pcm[k] = nullptr; d.pcm_shift[k] = 0; d.coef_start[k] = nullptr; }
  d.pcm_lf_disable = s.pcm_loop_filter_disable ? 1 : 0; d.any_nofilt = 0;
  for (int k = 0; k < 4; k++) d.tu_cap[k] = c->tu_cap[k];
  {
    // plane pointers address sample (0,0); the margins lie at negative coordinates
    Carver m(p.planes);
    for (int k = 0; k < 3; k++) { d.mx[k] = c->mx[k]; d.my[k] = c->my[k]; }
    d.rec[0] = m.take<int16_t>((size_t)c->pitch[0] * c->rows[0]) + (size_t)c->my[0] * c->pitch[0] + c->mx[0];
    d.rec[1] = m.take<int16_t>((size_t)c->pitch[1] * c->rows[1]) + (size_t)c->my[1] * c->pitch[1] + kCStep * c->mx[1];
    d.rec[2] = d.rec[1] + 1;
    d.sao[0] = m.take<int16_t>((size_t)c->pitch[0] * c->rows[0]) + (size_t)c->my[0] * c->pitch[0] + c->mx[0];
    d.sao[1] = m.take<int16_t>((size_t)c->pitch[1] * c->rows[1]) + (size_t)c->my[1] * c->pitch[1] + kCStep * c->mx[1];
    d.sao[2] = d.sao[1] + 1;
  }
  p.slices.assign(HMGPU_MAX_SLICES, SliceDev());
  return HMGPU_OK;
}

void free_picture(Picture& p) {
  if (p.pcm) hipFree(p.pcm);                       // (the planes belong to the context's slab)
  if (p.ccp) hipFree(p.ccp);
  p.ccp = nullptr;
  if (p.blob) hipFree(p.blob);
  p.blob = nullptr;
  if (p.meta) hipFree(p.meta);
  if (p.coef) hipFree(p.coef);
  if (p.derived) hipFree(p.derived);
  p.planes = p.meta = p.coef = p.derived = nullptr; p.pcm = nullptr;
}

hmgpu_status ensure_refs_extended(hmgpu_ctx* c, const Batch& b, size_t call_idx) {
  for (int i = 0; i < b.n; i++) {
    const Picture& p = c->pics[b.pic[i]];
    if (call_idx >= p.calls.size()) continue;
    const SliceDev& sd = p.slices[p.calls[call_idx].slice_idx];
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < HMGPU_MAX_REF; r++)
        if (sd.ref_pic[l][r] >= 0) { hmgpu_status st = ensure_extended(c, sd.ref_pic[l][r]); if (st != HMGPU_OK) return st; }
  }
  return HMGPU_OK;
}

}  // namespace

namespace hmgpu_host __attribute__((visibility("hidden"))) {

// device work of one batch of slice calls (one call per picture): counters, prep, inverse transforms, MC (+ residual), intra
hmgpu_status run_recon(hmgpu_ctx* c, const Batch& b, bool any_intra, bool any_wp, bool any_cells, bool any_bi, bool any_islice) {
  int max_ctus = 0;
  for (int i = 0; i < b.n; i++) max_ctus = std::max(max_ctus, b.num_ctus[i]);
  // 4:2:2 / 4:4:4: the chroma of every inter cell comes from the format-generic kernel, which reads the BlkInfo grid
  { ProfScope ps(c, K_PREP); launch_prep(c->d_pics, b, max_ctus, c->parts, any_intra, any_bi, any_cells || c->fmt != 1, c->fmt, c->stream); }
  if (c->fmt != 1) {
    // ... and adds the residual wherever it predicts: tiles no coded block covers must read as zero (Cb and Cr tiles are neighbours in memory)
    for (int i = 0; i < b.n; i++) {
      const PicDev& d = c->pics[b.pic[i]].dev;
      HIP_TRY(c, hipMemsetAsync(d.resid[1], 0, (size_t)((char*)d.resid[2] - (char*)d.resid[1]) + c->coef_elems[2] * sizeof(int16_t), c->stream));
    }
  }
  McArgs ma;
  memset(&ma, 0, sizeof(ma));
  ma.n = b.n; ma.width = c->seq.width; ma.height = c->seq.height; ma.log2ctu = c->seq.log2_ctu_size; ma.ctus_w = c->ctus_w;
  ma.tw = c->grid_w / 2; ma.npics = c->seq.max_pictures;
  ma.slab = c->plane_slab; ma.pic_stride = 2 * c->plane_bytes; ma.slab_bytes = ma.pic_stride * c->pics.size(); ma.sao_off = (uint32_t)c->plane_bytes;
  for (size_t i = 0; i < c->pics.size(); i++)
    if (c->pics[i].sao_applied) (i < 32 ? ma.sao_mask_lo : ma.sao_mask_hi) |= 1u << (i & 31);
  for (int i = 0; i < b.n; i++) {
    const PicDev& d = c->pics[b.pic[i]].dev;
    ma.first_ctu[i] = b.first_ctu[i]; ma.num_ctus[i] = b.num_ctus[i];
    ma.tmv[i] = d.tmv; ma.slices[i] = d.slices;
  }
  const PicDev& d0 = c->pics[b.pic[0]].dev;           // plane offsets inside a picture's part of the slab: the same for every picture
  const char* const base0 = (const char*)c->pics[b.pic[0]].planes;
  // the residual of the inter TUs first: the motion-compensation kernels add it when they write the prediction
  // workgroups per shard and size class: enough to keep the chip busy on one picture (768 per 2160p picture), fewer and longer-lived
  // ones when a batch of pictures fills it anyway (measured at 16 pictures: 12 -> 0.115 ms, 24 -> 0.122, 48 -> 0.135, 6 -> 0.120)
  uint32_t bps = (uint32_t)std::max(4, std::min(b.n >= 4 ? 12 : 24, max_ctus / 8 + 1));
  {
    ItxArgs ia;
    memset(&ia, 0, sizeof(ia));
    ia.n = b.n; ia.class_mask = 0xf;                        // all four size classes
    for (int k = 0; k < 3; k++) { ia.rtw[k] = (c->grid_w / 2) >> (k ? c->csx : 0); ia.bd[k] = d0.bd[k]; }
    ia.csx = c->csx; ia.csy = c->csy;
    for (int k = 0; k < 4; k++) ia.tu_cap[k] = c->tu_cap[k];
    for (int i = 0; i < b.n; i++) {
      const PicDev& d = c->pics[b.pic[i]].dev;
      for (int k = 0; k < 4; k++) ia.tu[i][k] = d.tu[k];
      ia.tu_count[i] = d.tu_count;
      for (int k = 0; k < 3; k++) { ia.coef[i][k] = d.coef[k]; ia.resid[i][k] = d.resid[k]; }
      ia.sl_m[i] = d.sl_m;
    }
    ProfScope ps(c, K_ITX);
    launch_itx(ia, bps, c->stream);
    bool any_ccp = false;
    for (int i = 0; i < b.n; i++) any_ccp |= c->pics[b.pic[i]].dev.ccp[0] != nullptr;
    if (any_ccp) launch_ccp(c->d_pics, b, max_ctus, c->stream);
  }
  {
    ProfScope ps(c, K_MC_LUMA);
    ma.pitch = c->pitch[0]; ma.bd = c->seq.bit_depth_luma;
    ma.origin_off = (uint32_t)((const char*)d0.rec[0] - base0);
    ma.rtw = c->grid_w / 2;
    for (int i = 0; i < b.n; i++) { ma.dst[i] = c->pics[b.pic[i]].dev.rec[0]; ma.resid[i] = c->pics[b.pic[i]].dev.resid[0]; }
    launch_mc_luma(ma, max_ctus, any_wp, any_bi, c->stream);
    if (any_cells) { ProfScope pc(c, K_MC_CELLS); launch_mc_luma_cells(c->d_pics, c->d_finals, b, max_ctus, c->seq.log2_ctu_size, any_wp, c->stream); }
  }
  if (c->fmt != 1) {
    ProfScope ps(c, K_MC_CHROMA);
    launch_mc_chroma_fmt(c->d_pics, c->d_finals, b, max_ctus, c->seq.log2_ctu_size, c->fmt, any_wp, c->stream);
  } else if (c->seq.chroma_format != 0) {
    ProfScope ps(c, K_MC_CHROMA);
    ma.pitch = c->pitch[1]; ma.bd = c->seq.bit_depth_chroma;
    ma.origin_off = (uint32_t)((const char*)d0.rec[1] - base0);      // the plane of both components (hmgpu_dev.h "chroma planes")
    ma.cr_off = 0;
    ma.rtw = c->grid_w / 4;
    for (int i = 0; i < b.n; i++) {
      const PicDev& d = c->pics[b.pic[i]].dev;
      ma.dst[i] = d.rec[1]; ma.dst2[i] = d.rec[2]; ma.resid[i] = d.resid[1]; ma.resid2[i] = d.resid[2];
    }
    launch_mc_chroma(ma, max_ctus, any_wp, any_bi, c->stream);
    if (any_cells) { ProfScope pc(c, K_MC_CELLS); launch_mc_chroma_cells(c->d_pics, c->d_finals, b, max_ctus, c->seq.log2_ctu_size, any_wp, c->stream); }
  }
  // intra CUs predict from finished neighbours (inter ones included): after motion compensation and the inter residuals
  if (any_intra) {
    ProfScope ps(c, K_INTRA);
    launch_intra(c->d_pics, b, c->d_ctu_order, c->num_ctus, !any_islice, c->stream);
    if (c->fmt == 2) launch_intra_chroma_422(c->d_pics, b, c->stream);        // (k_intra leaves the chroma of 4:2:2 pictures to it)
    for (int i = 0; i < b.n; i++) if (std::find(c->intra_launched.begin(), c->intra_launched.end(), b.pic[i]) == c->intra_launched.end()) c->intra_launched.push_back(b.pic[i]);
  }
  HIP_TRY(c, hipGetLastError());
  return HMGPU_OK;
}

// *fused: the fused kernel ran for the batch.  Its border tiles write the margins of the SAO planes, which are these pictures' final planes:
// the pictures are marked extended here and the caller launches no k_extend for them.  Every other route (a picture without SAO in the
// batch, single stages, 4:2:2 / 4:4:4) leaves the margins to the caller's k_extend as before.
hmgpu_status run_filter(hmgpu_ctx* c, const Batch& b, int stages, bool* fused) {
  *fused = false;
  // all three stages on pictures that all carry SAO: one pass through LDS instead of three through HBM (k_filter.hip)
  bool all_sao = stages == 7 && c->fmt == 1;            // (the fused kernel's tiles are those of 4:2:0 pictures)
  for (int i = 0; i < b.n && all_sao; i++) all_sao = c->pics[b.pic[i]].sao_any;
  if (all_sao) {
    bool nofilt = false;
    for (int i = 0; i < b.n; i++) nofilt |= c->pics[b.pic[i]].dev.any_nofilt != 0;
    { ProfScope ps(c, K_FILTER); launch_filter_fused(c->d_pics, b, c->seq.width, c->seq.height, nofilt, c->stream); }
    HIP_TRY(c, hipGetLastError());
    for (int i = 0; i < b.n; i++) c->pics[b.pic[i]].extended = true;
    *fused = true;
    return HMGPU_OK;
  }
  // (4:2:2 / 4:4:4: k_deblock filters luma only, the chroma edges of the format's own grid follow from k_cfmt.hip -- per direction, as in HM)
  if (stages & 1) { ProfScope ps(c, K_DBK_VER); launch_deblock(c->d_pics, b, 0, c->seq.width, c->seq.height, c->stream);
                    if (c->fmt != 1) launch_deblock_chroma_fmt(c->d_pics, b, 0, c->seq.width, c->seq.height, c->stream); }
  if (stages & 2) { ProfScope ps(c, K_DBK_HOR); launch_deblock(c->d_pics, b, 1, c->seq.width, c->seq.height, c->stream);
                    if (c->fmt != 1) launch_deblock_chroma_fmt(c->d_pics, b, 1, c->seq.width, c->seq.height, c->stream); }
  if (stages & 4) {
    bool any = false;
    for (int i = 0; i < b.n; i++) any |= c->pics[b.pic[i]].sao_any;
    if (any) { ProfScope ps(c, K_SAO); launch_sao(c->d_pics, b, c->seq.width, c->seq.height, c->csx, c->csy, c->stream); }
  }
  HIP_TRY(c, hipGetLastError());
  return HMGPU_OK;
}

// reconstructBlkSAOParams (TComSampleAdaptiveOffset.cpp:229-372) + deriveLoopFilterBoundaryAvailibility
// (TComPicSym.cpp:365-471), host side: a dependent chain over CTUs, a few microseconds of work.
hmgpu_status stage_sao(hmgpu_ctx* c, Picture& p, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao,
                       const std::vector<uint16_t>& slice_idx, const std::vector<uint16_t>& tile_idx) {
  const int n = c->num_ctus;
  // merge resolution by reference: res[a][comp] = the NEW / OFF entry that CTU a's parameters come from (a merged CTU takes all
  // three components of its left / upper neighbour's RESOLVED parameters); nothing of the caller's array is copied
  std::vector<const hmgpu_sao_param*> res((size_t)n * 3);
  std::vector<SaoDev>& dev = p.h_saoprm;  // lives with the picture: the upload below is asynchronous
  dev.resize((size_t)n * 3);
  bool any = false;
  for (int a = 0; a < n; a++) {
    const int cx = a % c->ctus_w, cy = a / c->ctus_w;
    const hmgpu_sao_param* const* merge[2] = {nullptr, nullptr};
    auto same = [&](int o) { return slice_idx[o] == slice_idx[a] && tile_idx[o] == tile_idx[a]; };
    if (cx > 0 && same(a - 1)) merge[HMGPU_SAO_MERGE_LEFT] = &res[(size_t)(a - 1) * 3];
    if (cy > 0 && same(a - c->ctus_w)) merge[HMGPU_SAO_MERGE_ABOVE] = &res[(size_t)(a - c->ctus_w) * 3];
    // neighbour availability as a 3x3 grid (SaoDev::avail): bit 3 * (dy + 1) + (dx + 1)
    unsigned avail = 1u << 4;
    for (int k = 0; k < 9; k++) {
      if (k == 4) continue;
      const int nx = cx + k % 3 - 1, ny = cy + k / 3 - 1;
      if (nx < 0 || nx >= c->ctus_w || ny < 0 || ny >= c->ctus_h) continue;
      const int o = ny * c->ctus_w + nx;
      bool ok = true;
      if (slice_idx[o] != slice_idx[a]) {
        // the slice that comes later in decoding order decides with its own flag (TComPicSym.cpp:403-452)
        const SliceDev& later = p.slices[std::max(slice_idx[o], slice_idx[a])];
        ok = later.lf_across_slices != 0;
      }
      if (ok && !pp->lf_across_tiles) ok = tile_idx[o] == tile_idx[a];
      if (ok) avail |= 1u << k;
    }
    for (int comp = 0; comp < 3; comp++) {
      const hmgpu_sao_param* r = &sao[(size_t)a * 3 + comp];
      if (r->mode_idc == HMGPU_SAO_MERGE) {
        if (r->type_idc < 0 || r->type_idc > 1 || !merge[r->type_idc]) return HMGPU_EINVAL;     // HM: assert(mergeTarget != NULL)
        r = merge[r->type_idc][comp];
      }
      res[(size_t)a * 3 + comp] = r;
      const int shift = comp == 0 ? pp->sao_offset_shift_luma : pp->sao_offset_shift_chroma;
      SaoDev& d = dev[(size_t)a * 3 + comp];
      memset(&d, 0, sizeof(d));
      d.type = r->mode_idc == HMGPU_SAO_OFF ? -1 : (int8_t)r->type_idc;
      d.avail = (uint16_t)avail;
      // offsets of a NEW entry: the coded ones scaled by log2_sao_offset_scale (reconstructBlkSAOParam, TComSampleAdaptiveOffset.cpp:229-372)
      if (d.type == HMGPU_SAO_BO) {
        d.band = (uint8_t)(r->type_aux_info & 31);
        for (int i = 0; i < 4; i++) d.off[i] = (int8_t)(r->offset[(r->type_aux_info + i) & 31] * (1 << shift));
      } else if (d.type >= 0) {
        for (int i = 0; i < 5; i++) d.off[i] = (int8_t)(r->offset[i] * (1 << shift));
      }
      any |= d.type >= 0;
    }
  }
  p.sao_any = any;
  HIP_TRY(c, h2d_small(c, p.dev.saoprm, dev.data(), dev.size() * sizeof(SaoDev), c->stream));
  return HMGPU_OK;
}

}  // namespace hmgpu_host

// ======================================================================================================= C ABI
extern "C" {

const char* hmgpu_status_string(hmgpu_status s) {
  switch (s) {
    case HMGPU_OK: return "ok";
    case HMGPU_EINVAL: return "invalid argument";
    case HMGPU_EDEVICE: return "device (HIP) error";
    case HMGPU_EUNSUPPORTED: return "coding tool not supported";
    case HMGPU_ENOMEM: return "out of memory";
  }
  return "?";
}
const char* hmgpu_kernel_name(int32_t k) { return (k >= 0 && k < HMGPU_NUM_KERNELS) ? kKernelNames[k] : ""; }

int32_t hmgpu_num_ctus(const hmgpu_seq_params* seq) {
  const int c = 1 << seq->log2_ctu_size;
  return ((seq->width + c - 1) / c) * ((seq->height + c - 1) / c);
}
int32_t hmgpu_parts_per_ctu(const hmgpu_seq_params* seq) { return 1 << (2 * seq->log2_ctu_size - 4); }

hmgpu_status hmgpu_create(const hmgpu_seq_params* seq, int device_ordinal, hmgpu_ctx** out) {
  if (!seq || !out) return HMGPU_EINVAL;
  *out = nullptr;
  if (seq->width <= 0 || seq->height <= 0 || (seq->width & 7) || (seq->height & 7)) return HMGPU_EINVAL;
  if (seq->log2_ctu_size < 4 || seq->log2_ctu_size > 6) return HMGPU_EINVAL;
  if (seq->max_pictures < 1 || seq->max_pictures > kMaxPics) return HMGPU_EINVAL;
  if (seq->chroma_format < 0 || seq->chroma_format > 3) return HMGPU_EINVAL;              // 0: monochrome -- the chroma planes exist and are left alone
  if (seq->range_ext_flags & ~(HMGPU_REXT_ROTATION | HMGPU_REXT_IMPLICIT_RDPCM | HMGPU_REXT_EXPLICIT_RDPCM | HMGPU_REXT_INTRA_SMOOTHING_DISABLED)) return HMGPU_EUNSUPPORTED;
  if (seq->bit_depth_luma < 8 || seq->bit_depth_luma > 12 || seq->bit_depth_chroma < 8 || seq->bit_depth_chroma > 12) return HMGPU_EUNSUPPORTED;
  hmgpu_ctx* c = new (std::nothrow) hmgpu_ctx();
  if (!c) return HMGPU_ENOMEM;
  c->seq = *seq;
  c->device = device_ordinal;
  c->host_timing = getenv("HMGPU_HOST_TIMING") != nullptr;
  hipError_t e = hipSetDevice(device_ordinal);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->copy_join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void**)&c->bounce, hmgpu_ctx::kBounceSegs * hmgpu_ctx::kBounceSeg, hipHostMallocDefault);
  for (int g = 0; g < hmgpu_ctx::kBounceSegs && e == hipSuccess; g++)
    for (int k = 0; k < 3 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->bounce_ev[g][k], hipEventDisableTiming);
  for (int k = 0; k < 8 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->copy_ev[k], hipEventDisableTiming);
  for (int k = 0; k < 8 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->use_ev[k], hipEventDisableTiming);
  for (int k = 0; k < 32 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->dl_ev[k], hipEventDisableTiming | hipEventBlockingSync);   // (waited for by helper threads: sleep, do not spin)
  if (e == hipSuccess) { e = hipHostMalloc((void**)&c->dl_fault, 32 * sizeof(uint32_t), hipHostMallocDefault); if (e == hipSuccess) memset(c->dl_fault, 0, 32 * sizeof(uint32_t)); }
  for (int k = 0; k < 2 && e == hipSuccess; k++) e = hipEventCreateWithFlags(&c->lane_ev[k], hipEventDisableTiming);
  if (e != hipSuccess) { delete c; return HMGPU_EDEVICE; }
  c->ctu = 1 << seq->log2_ctu_size; c->pw = c->ctu / 4; c->parts = c->pw * c->pw;
  c->ctus_w = (seq->width + c->ctu - 1) / c->ctu; c->ctus_h = (seq->height + c->ctu - 1) / c->ctu;
  c->num_ctus = c->ctus_w * c->ctus_h;
  c->grid_w = c->ctus_w * c->pw; c->grid_h = c->ctus_h * c->pw;
  // planes: HM's picture-buffer shape (TComPicYuv.cpp:89-100: margins of maxCU + 16 luma samples all around, extended by
  // replication) with device-friendly numbers: 128-sample (256-byte) horizontal margins keep sample (0,y) cache-line
  // aligned, rows are a multiple of 128 bytes plus one spare line (vector loads may run past the margin; the pitch is
  // never a power of two)
  c->fmt = seq->chroma_format == 0 ? 1 : seq->chroma_format;
  c->csx = c->fmt == 3 ? 0 : 1; c->csy = c->fmt == 1 ? 1 : 0;
  c->mx[0] = 128; c->mx[1] = c->mx[2] = 128 >> c->csx;
  c->my[0] = 80; c->my[1] = c->my[2] = 80 >> c->csy;
  c->pitch[0] = (int)align_up((size_t)seq->width, 64) + 2 * c->mx[0] + 64;
  // (Cb and Cr alternate in one plane, hmgpu_dev.h "chroma planes": its pitch is that of kCStep rows of one component)
  c->pitch[1] = c->pitch[2] = kCStep * ((int)align_up((size_t)seq->width >> c->csx, 64) + 2 * c->mx[1] + 64);
  c->rows[0] = c->ctus_h * c->ctu + 2 * c->my[0] + 8; c->rows[1] = c->rows[2] = ((c->ctus_h * c->ctu) >> c->csy) + 2 * c->my[1] + 8;
  c->coef_elems[0] = (size_t)c->num_ctus * c->ctu * c->ctu;
  c->coef_elems[1] = c->coef_elems[2] = c->coef_elems[0] >> (c->csx + c->csy);
  {
    // TU list capacity of one shard: prep blocks (256 threads x 4 partitions = 1024 partitions) go round-robin to the
    // shards; 256 partitions (one 64x64 luma area) hold at most 256+128 4x4, 64+32 8x8, 16+8 16x16 and 4 32x32 TUs
    const size_t blocks = ((size_t)c->num_ctus * (c->parts / 4) + 255) / 256;
    const size_t per_shard = (blocks + kTuShards - 1) / kTuShards;
    const uint32_t per_block[4] = {4 * 384, 4 * 96, 4 * 24, 4 * 4};
    // (4:2:2 / 4:4:4: up to as many chroma blocks per component as luma blocks, of every size)
    for (int k = 0; k < 4; k++) c->tu_cap[k] = (uint32_t)(per_shard * (c->fmt == 1 ? per_block[k] : 3u * (1024u >> (2 * k))));
  }
  c->pics.resize(seq->max_pictures);
  c->h_finals.resize(seq->max_pictures);
  hmgpu_status st = HMGPU_OK;
  c->plane_bytes = plane_set_bytes(c);
  if (hipMalloc((void**)&c->plane_slab, c->plane_bytes * 2 * seq->max_pictures) != hipSuccess ||
      hipMemset(c->plane_slab, 0, c->plane_bytes * 2 * seq->max_pictures) != hipSuccess) st = HMGPU_EDEVICE;
  for (int i = 0; i < seq->max_pictures && st == HMGPU_OK; i++) st = alloc_picture(c, c->pics[i]);
  if (st == HMGPU_OK) {
    {
      std::vector<int32_t> order;
      for (int d = 0; d <= 2 * (c->ctus_h - 1) + c->ctus_w - 1; d++)
        for (int r = 0; r < c->ctus_h; r++) { const int col = d - 2 * r; if (col >= 0 && col < c->ctus_w) order.push_back(r * c->ctus_w + col); }
      if (hipMalloc((void**)&c->d_ctu_order, order.size() * sizeof(int32_t)) != hipSuccess ||
          hipMemcpy(c->d_ctu_order, order.data(), order.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) st = HMGPU_EDEVICE;
    }
    if (hipMalloc((void**)&c->d_pics, sizeof(PicDev) * seq->max_pictures) != hipSuccess ||
        hipMalloc((void**)&c->d_finals, sizeof(PlaneSet) * seq->max_pictures) != hipSuccess) st = HMGPU_EDEVICE;
  }
  if (st == HMGPU_OK) {
    for (int i = 0; i < seq->max_pictures && st == HMGPU_OK; i++) { st = push_picdev(c, i); if (st == HMGPU_OK) st = push_final(c, i, c->stream); }
    if (st == HMGPU_OK && hipStreamSynchronize(c->stream) != hipSuccess) st = HMGPU_EDEVICE;
  }
  if (st != HMGPU_OK) { hmgpu_destroy(c); return st; }
  *out = c;
  return HMGPU_OK;
}

void hmgpu_destroy(hmgpu_ctx* c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  prof_drain(c);
  for (EventPair& ep : c->free_events) { hipEventDestroy(ep.a); hipEventDestroy(ep.b); }
  if (c->host_timing && c->host_calls)
    fprintf(stderr, "hmgpu host time per hmgpu_decompress_pictures + hmgpu_filter_pictures (%llu calls): validate %.3f ms, slices %.3f, stage_inputs %.3f, recon launches %.3f, sao staging %.3f, filter launches %.3f\n",
            (unsigned long long)c->host_calls, 1e3 * c->host_s[0] / c->host_calls, 1e3 * c->host_s[1] / c->host_calls, 1e3 * c->host_s[2] / c->host_calls,
            1e3 * c->host_s[3] / c->host_calls, 1e3 * c->host_s[4] / c->host_calls, 1e3 * c->host_s[5] / c->host_calls);
  for (Picture& p : c->pics) free_picture(p);
  if (c->d_pics) hipFree(c->d_pics);
  if (c->d_finals) hipFree(c->d_finals);
  if (c->plane_slab) hipFree(c->plane_slab);
  if (c->scratch) hipFree(c->scratch);
  if (c->conceal_masks) hipFree(c->conceal_masks);
  if (c->d_ctu_order) hipFree(c->d_ctu_order);
  if (c->stream) hipStreamDestroy(c->stream);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->copy_stream2) { hipStreamSynchronize(c->copy_stream2); hipStreamDestroy(c->copy_stream2); }
  if (c->copy_stream) { hipStreamSynchronize(c->copy_stream); hipStreamDestroy(c->copy_stream); }
  if (c->copy_join) hipEventDestroy(c->copy_join);
  for (int g = 0; g < hmgpu_ctx::kBounceSegs; g++) for (int k = 0; k < 3; k++) if (c->bounce_ev[g][k]) hipEventDestroy(c->bounce_ev[g][k]);
  if (c->bounce) (void)hipHostFree(c->bounce);
  for (int k = 0; k < 8; k++) { if (c->copy_ev[k]) hipEventDestroy(c->copy_ev[k]); if (c->use_ev[k]) hipEventDestroy(c->use_ev[k]); }
  for (hmgpu_staging* st : c->shared_stagings) {
    st->sharers.erase(std::remove(st->sharers.begin(), st->sharers.end(), c), st->sharers.end());
    if (st->reader == c) { st->reader = nullptr; st->copy_seq = 0; }      // (the copy stream was drained above)
  }
  for (hmgpu_staging* st : c->stagings) {
    for (hmgpu_ctx* o : st->sharers) o->shared_stagings.erase(std::remove(o->shared_stagings.begin(), o->shared_stagings.end(), st), o->shared_stagings.end());
    if (st->host) hipHostFree(st->host);
    delete st;
  }
  for (int k = 0; k < 32; k++) if (c->dl_ev[k]) hipEventDestroy(c->dl_ev[k]);
  if (c->dl_fault) (void)hipHostFree(c->dl_fault);
  for (int k = 0; k < hmgpu_ctx::kHashStreams; k++) if (c->hash_stream[k]) { (void)hipStreamSynchronize(c->hash_stream[k]); (void)hipStreamDestroy(c->hash_stream[k]); }
  for (int k = 0; k < hmgpu_ctx::kHashSlots; k++) {
    if (c->hash_packed[k]) hipEventDestroy(c->hash_packed[k]);
    if (c->hash_done[k]) hipEventDestroy(c->hash_done[k]);
    if (c->hash_buf[k]) (void)hipFree(c->hash_buf[k]);
  }
  if (c->hash_dev) (void)hipFree(c->hash_dev);
  for (int k = 0; k < 2; k++) if (c->xfer_ev[k]) hipEventDestroy(c->xfer_ev[k]);
  for (int k = 0; k < 2; k++) if (c->exp_ev[k]) hipEventDestroy(c->exp_ev[k]);
  for (auto& sl : c->scale_slot) sl.release();
  for (auto& wb : c->window_buf) wb.release();
  for (auto& cs : c->colour_slot) cs.release();
  if (c->hash_host) (void)hipHostFree(c->hash_host);
  for (int k = 0; k < 2; k++) if (c->lane_ev[k]) hipEventDestroy(c->lane_ev[k]);
  delete c;
}

int32_t hmgpu_last_device_error(const hmgpu_ctx* c) { return c ? c->last_err : 0; }

hmgpu_status hmgpu_debug_stall_intra(hmgpu_ctx* c, hmgpu_pic pic, int32_t ctu) {
  if (!c || !valid_pic(c, pic) || ctu < -1 || ctu >= c->num_ctus) return HMGPU_EINVAL;
  c->pics[pic].dev.debug_skip_ctu = ctu;               // (reaches the device with the picture's next decompress call)
  return HMGPU_OK;
}

void* hmgpu_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void hmgpu_host_free(void* p) { if (p) (void)hipHostFree(p); }

hmgpu_status hmgpu_sync(hmgpu_ctx* c) {
  if (c && c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
  if (!c) return HMGPU_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  return check_faults(c);
}

hmgpu_status hmgpu_picture_acquire(hmgpu_ctx* c, hmgpu_pic* out) {
  if (!c || !out) return HMGPU_EINVAL;
  for (size_t i = 0; i < c->pics.size(); i++) {
    Picture& p = c->pics[i];
    if (!p.in_use) {
      p.in_use = true; p.sao_applied = false; p.filter_ready = false; p.sao_any = false; p.calls.clear(); p.max_slice = -1;
      p.extended = false;
      coverage_clear(p);
      filter_forget(p);
      p.concealed.clear(); p.concealed_ctus = 0;
      p.dev.sao_applied = 0; p.dev.any_nofilt = 0;
      *out = (hmgpu_pic)i;
      hmgpu_status st = push_final(c, (int)i, c->stream);
      return st;
    }
  }
  return HMGPU_ENOMEM;
}

hmgpu_status hmgpu_picture_release(hmgpu_ctx* c, hmgpu_pic pic) {
  if (!c || !valid_pic(c, pic)) return HMGPU_EINVAL;
  c->pics[pic].in_use = false;
  return HMGPU_OK;
}

hmgpu_status hmgpu_picture_upload(hmgpu_ctx* c, hmgpu_pic pic, const int16_t* const planes[3], const int32_t strides[3]) {
  if (!c || !valid_pic(c, pic) || !planes || !strides) return HMGPU_EINVAL;
  Picture& p = c->pics[pic];
  coverage_clear(p);                   // (uploaded samples come without side information)
  filter_forget(p);
  if (p.sao_applied) {                 // uploaded samples ARE the picture: back to the reconstruction planes
    p.sao_applied = false; p.dev.sao_applied = 0;
    hmgpu_status st = push_final(c, pic, c->stream);
    if (st == HMGPU_OK) st = push_picdev(c, pic);
    if (st != HMGPU_OK) return st;
  }
  HIP_TRY(c, hipMemcpy2DAsync(p.dev.rec[0], (size_t)c->pitch[0] * 2, planes[0], (size_t)strides[0] * 2, (size_t)c->seq.width * 2, c->seq.height,
                              hipMemcpyHostToDevice, c->stream));
  {
    // the chroma components arrive as HM's two planes and are laid sample by sample into the device's one (hmgpu_dev.h "chroma planes")
    const int w = c->seq.width >> c->csx, h = c->seq.height >> c->csy;
    int16_t* d = static_cast<int16_t*>(ctx_scratch(c, (size_t)2 * w * h * sizeof(int16_t)));
    if (!d) return HMGPU_ENOMEM;
    for (int k = 1; k < 3; k++) {
      int16_t* dk = d + (size_t)(k - 1) * w * h;
      HIP_TRY(c, hipMemcpy2DAsync(dk, (size_t)w * 2, planes[k], (size_t)strides[k] * 2, (size_t)w * 2, h, hipMemcpyHostToDevice, c->stream));
      launch_unpack(dk, w, h, p.dev.rec[k], c->pitch[k], kCStep, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  p.extended = false;
  return HMGPU_OK;
}

// the final planes of a picture to HM's three host planes, enqueued on the context's stream: luma straight from its plane, the chroma
// components taken apart into a dense block of device scratch first (later users of the scratch follow on the same stream)
static hmgpu_status enqueue_download(hmgpu_ctx* c, Picture& p, int16_t* const planes[3], const int32_t strides[3]) {
  const int16_t* y = p.sao_applied ? p.dev.sao[0] : p.dev.rec[0];
  HIP_TRY(c, hipMemcpy2DAsync(planes[0], (size_t)strides[0] * 2, y, (size_t)c->pitch[0] * 2, (size_t)c->seq.width * 2, c->seq.height, hipMemcpyDeviceToHost, c->stream));
  const int w = c->seq.width >> c->csx, h = c->seq.height >> c->csy;
  int16_t* d = static_cast<int16_t*>(ctx_scratch(c, (size_t)2 * w * h * sizeof(int16_t)));
  if (!d) return HMGPU_ENOMEM;
  for (int k = 1; k < 3; k++) {
    const int16_t* src = p.sao_applied ? p.dev.sao[k] : p.dev.rec[k];
    int16_t* dk = d + (size_t)(k - 1) * w * h;
    launch_pack(src, c->pitch[k], kCStep, 0, 0, w, h, 2, reinterpret_cast<uint8_t*>(dk), w * 2, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy2DAsync(planes[k], (size_t)strides[k] * 2, dk, (size_t)w * 2, (size_t)w * 2, h, hipMemcpyDeviceToHost, c->stream));
  }
  return HMGPU_OK;
}

hmgpu_status hmgpu_picture_download(hmgpu_ctx* c, hmgpu_pic pic, int16_t* const planes[3], const int32_t strides[3]) {
  if (!c || !valid_pic(c, pic) || !planes || !strides) return HMGPU_EINVAL;
  Picture& p = c->pics[pic];
  { const hmgpu_status st = enqueue_download(c, p, planes, strides); if (st != HMGPU_OK) return st; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  return check_faults(c);
}

hmgpu_status hmgpu_picture_download_begin(hmgpu_ctx* c, hmgpu_pic pic, int16_t* const planes[3], const int32_t strides[3], uint64_t* ticket) {
  if (!c || !valid_pic(c, pic) || !planes || !strides || !ticket) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  Picture& p = c->pics[pic];
  { const hmgpu_status st = enqueue_download(c, p, planes, strides); if (st != HMGPU_OK) return st; }
  const uint64_t t = c->dl_seq.load() + 1;
  // the picture's fault word (an intra wavefront that gave up waiting) as it stands behind these copies: hmgpu_download_wait reports it
  HIP_TRY(c, hipMemcpyAsync(&c->dl_fault[t % 32], p.dev.fault, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->dl_ev[t % 32], c->stream));
  c->dl_seq.store(t);
  *ticket = t;
  touch(c, pic);
  commit_use(c);
  return HMGPU_OK;
}

hmgpu_status hmgpu_download_wait(hmgpu_ctx* c, uint64_t ticket) {
  if (!c || ticket == 0 || ticket > c->dl_seq.load()) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  // a ticket whose event has been re-recorded is 32 downloads old: the event now stands for a LATER point of the same stream
  if (hipEventSynchronize(c->dl_ev[ticket % 32]) != hipSuccess) return HMGPU_EDEVICE;
  // (read-only here: this may be a helper thread; the word on the device stays set until the context's own thread reads it in check_faults)
  if (c->dl_seq.load() - ticket < 32 && reinterpret_cast<volatile uint32_t*>(c->dl_fault)[ticket % 32]) return HMGPU_EDEVICE;
  return HMGPU_OK;
}


hmgpu_status hmgpu_picture_device_region(hmgpu_ctx* c, hmgpu_pic pic, int32_t which, void** base, int64_t* bytes) {
  if (!c || !valid_pic(c, pic) || !base || !bytes || (which != HMGPU_REGION_FINISHED && which != HMGPU_REGION_RECEIVE)) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  Picture& p = c->pics[pic];
  const size_t plane_bytes = plane_set_bytes(c);
  if (which == HMGPU_REGION_FINISHED) {
    hmgpu_status st = ensure_extended(c, pic);
    if (st != HMGPU_OK) return st;
    *base = (char*)p.planes + (p.sao_applied ? plane_bytes : 0);     // rec planes first, SAO planes behind (alloc_picture)
  } else {
    if (p.sao_applied) {               // a received picture lives in the reconstruction planes, like an uploaded one
      p.sao_applied = false; p.dev.sao_applied = 0;
      hmgpu_status st = push_final(c, pic, c->stream);
      if (st == HMGPU_OK) st = push_picdev(c, pic);
      if (st != HMGPU_OK) return st;
    }
    p.extended = false;
    filter_forget(p);
    *base = p.planes;
  }
  *bytes = (int64_t)plane_bytes;
  return HMGPU_OK;
}

hmgpu_status hmgpu_picture_commit_received(hmgpu_ctx* c, hmgpu_pic pic) {
  if (!c || !valid_pic(c, pic)) return HMGPU_EINVAL;
  Picture& p = c->pics[pic];
  if (p.sao_applied) return HMGPU_EINVAL;          // hmgpu_picture_device_region(RECEIVE) was not called
  coverage_clear(p);                               // (only the planes travelled)
  filter_forget(p);
  p.extended = true;                               // the margins travelled with the planes
  return HMGPU_OK;
}

// A finished picture of one context into a picture of another context of the same geometry -- on another GPU of the process (a peer
// copy over xGMI) or on the same one -- ordered behind the work of both contexts' streams: what a decoder that spreads the pictures of
// one temporal level over several devices does with each reference picture (TComPrediction.cpp:593 reads it on the other device).
hmgpu_status hmgpu_picture_transfer(hmgpu_ctx* src, hmgpu_pic src_pic, hmgpu_ctx* dst, hmgpu_pic dst_pic) {
  if (!src || !dst || !valid_pic(src, src_pic) || !valid_pic(dst, dst_pic) || (src == dst && src_pic == dst_pic)) return HMGPU_EINVAL;
  const hmgpu_seq_params &a = src->seq, &b = dst->seq;
  if (a.width != b.width || a.height != b.height || a.log2_ctu_size != b.log2_ctu_size || a.bit_depth_luma != b.bit_depth_luma ||
      a.bit_depth_chroma != b.bit_depth_chroma) return HMGPU_EINVAL;
  void *from = nullptr, *to = nullptr;
  int64_t n_from = 0, n_to = 0;
  hmgpu_status st = hmgpu_picture_device_region(src, src_pic, HMGPU_REGION_FINISHED, &from, &n_from);      // (extends the border if needed)
  if (st == HMGPU_OK) st = hmgpu_picture_device_region(dst, dst_pic, HMGPU_REGION_RECEIVE, &to, &n_to);
  if (st != HMGPU_OK) return st;
  if (n_from != n_to) return HMGPU_EINVAL;
  if (src->device != dst->device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst->device, src->device) == hipSuccess && can) {
      hipSetDevice(dst->device);
      const hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return HMGPU_EDEVICE;
      (void)hipGetLastError();
    }
  }
  // source ready -> copy on the receiver's stream -> the source may be rewritten again
  hipSetDevice(src->device);
  if (!src->xfer_ev[0]) for (int k = 0; k < 2; k++) HIP_TRY(src, hipEventCreateWithFlags(&src->xfer_ev[k], hipEventDisableTiming));
  HIP_TRY(src, hipEventRecord(src->xfer_ev[0], src->stream));
  hipSetDevice(dst->device);
  HIP_TRY(dst, hipStreamWaitEvent(dst->stream, src->xfer_ev[0], 0));
  HIP_TRY(dst, hipMemcpyPeerAsync(to, dst->device, from, src->device, (size_t)n_from, dst->stream));
  HIP_TRY(dst, hipEventRecord(src->xfer_ev[1], dst->stream));
  hipSetDevice(src->device);
  HIP_TRY(src, hipStreamWaitEvent(src->stream, src->xfer_ev[1], 0));
  src->xfer_bytes += (uint64_t)n_from;
  touch(src, src_pic); commit_use(src);
  touch(dst, dst_pic); commit_use(dst);
  return hmgpu_picture_commit_received(dst, dst_pic);
}
uint64_t hmgpu_transfer_bytes(const hmgpu_ctx* c) { return c ? c->xfer_bytes : 0; }

void* hmgpu_stream(hmgpu_ctx* c) { return c ? (void*)c->stream : nullptr; }

hmgpu_status hmgpu_replay_batch(hmgpu_ctx* c, const hmgpu_pic* pics, int32_t n, int32_t stages, int32_t iters) {
  if (!c || !pics || n < 1 || n > kMaxBatch || iters < 0) return HMGPU_EINVAL;
  size_t ncalls = 0;
  for (int i = 0; i < n; i++) {
    if (!valid_pic(c, pics[i])) return HMGPU_EINVAL;
    if (i == 0) ncalls = c->pics[pics[i]].calls.size();
    else if (c->pics[pics[i]].calls.size() != ncalls) return HMGPU_EINVAL;
  }
  if ((stages & 8) && ncalls == 0) return HMGPU_EINVAL;
  hipSetDevice(c->device);
  // Two lanes: the batch is cut in two halves that run the same kernel sequence on two streams.  The halves are independent
  // pictures, so the lanes drift apart and kernels of different kinds (latency-bound motion compensation, ALU-heavier filters)
  // share the chip -- measured +12..25 % pictures/s over one lane.  One lane while profiling: per-kernel event
  // times are only meaningful when a kernel has the chip to itself.
  const int lanes = (c->replay_streams == 2 && n >= 2 && !c->profiling) ? 2 : 1;
  hipStream_t const main_stream = c->stream;
  if (lanes == 2) {                       // the second lane starts after everything enqueued so far on the context's stream
    HIP_TRY(c, hipEventRecord(c->lane_ev[0], main_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream2, c->lane_ev[0], 0));
  }
  hmgpu_status result = HMGPU_OK;
  for (int it = 0; it < iters && result == HMGPU_OK; it++) {
    for (int lane = 0; lane < lanes && result == HMGPU_OK; lane++) {
      const int lo = lanes == 2 ? (lane == 0 ? 0 : n / 2) : 0, hi = lanes == 2 ? (lane == 0 ? n / 2 : n) : n;
      c->stream = lane == 0 ? main_stream : c->stream2;      // every launcher below enqueues on c->stream
      if (stages & 8) {
        for (size_t k = 0; k < ncalls && result == HMGPU_OK; k++) {
          Batch b; memset(&b, 0, sizeof(b));
          b.n = hi - lo;
          bool any_intra = false, any_wp = false, any_cells = false, any_bi = false, any_islice = false;
          for (int i = lo; i < hi; i++) {
            const SliceCall& sc = c->pics[pics[i]].calls[k];
            b.pic[i - lo] = pics[i]; b.first_ctu[i - lo] = sc.first_ctu; b.num_ctus[i - lo] = sc.num_ctus;
            any_intra |= sc.intra; any_wp |= sc.wp; any_cells |= sc.cells; any_bi |= sc.bi; any_islice |= sc.islice;
          }
          result = ensure_refs_extended(c, b, k);
          if (result == HMGPU_OK) result = run_recon(c, b, any_intra, any_wp, any_cells, any_bi, any_islice);
        }
      }
      if ((stages & 7) && result == HMGPU_OK) {
        Batch b; memset(&b, 0, sizeof(b));
        b.n = hi - lo;
        for (int i = lo; i < hi; i++) { b.pic[i - lo] = pics[i]; b.first_ctu[i - lo] = 0; b.num_ctus[i - lo] = c->num_ctus; }
        // a lane's step: prep, inverse transform, luma and chroma motion compensation (run_recon), then the loop filter; the border
        // extension follows as a launch of its own only where the fused kernel did not run (its border tiles write the margins)
        bool fused = false;
        result = run_filter(c, b, stages & 7, &fused);
        if (result == HMGPU_OK && !fused) {
          { ProfScope ps(c, K_EXTEND); launch_extend(c->d_pics, b, c->seq.width, c->seq.height, c->mx[0], c->my[0], c->csx, c->csy, c->stream); }
          if (hipGetLastError() != hipSuccess) result = HMGPU_EDEVICE;
        }
      }
    }
  }
  c->stream = main_stream;
  if (lanes == 2) {                       // whatever follows on the context's stream (sync, download) sees both lanes finished
    HIP_TRY(c, hipEventRecord(c->lane_ev[1], c->stream2));
    HIP_TRY(c, hipStreamWaitEvent(main_stream, c->lane_ev[1], 0));
  }
  for (int i = 0; i < n; i++) touch(c, pics[i]);
  commit_use(c);                          // (the references were named by ensure_refs_extended)
  return result;
}

hmgpu_status hmgpu_set_streams(hmgpu_ctx* c, int32_t n) {
  if (!c || n < 1 || n > 2) return HMGPU_EINVAL;
  c->replay_streams = n;
  return HMGPU_OK;
}

hmgpu_status hmgpu_replay(hmgpu_ctx* c, hmgpu_pic cur, int32_t stages, int32_t iters) { return hmgpu_replay_batch(c, &cur, 1, stages, iters); }

hmgpu_status hmgpu_set_profiling(hmgpu_ctx* c, int32_t enable) {
  if (!c) return HMGPU_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  c->profiling = enable != 0;
  return HMGPU_OK;
}

hmgpu_status hmgpu_get_stats(hmgpu_ctx* c, hmgpu_stats* out, int32_t reset) {
  if (!c || !out) return HMGPU_EINVAL;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_drain(c);
  memset(out, 0, sizeof(*out));
  for (int k = 0; k < HMGPU_NUM_KERNELS; k++) { out->kernel_ms[k] = c->kernel_ms[k]; out->kernel_launches[k] = c->kernel_launches[k]; }
  for (Picture& p : c->pics) {
    if (!p.in_use) continue;
    unsigned long long st[2 * kTuShards];
    HIP_TRY(c, hipMemcpy(st, p.dev.stats, sizeof(st), hipMemcpyDeviceToHost));
    for (int s = 0; s < kTuShards; s++) { out->intra_partitions += st[s]; out->inter_partitions += st[kTuShards + s]; }
    if (reset) HIP_TRY(c, hipMemset(p.dev.stats, 0, sizeof(st)));
  }
  if (reset) for (int k = 0; k < HMGPU_NUM_KERNELS; k++) { c->kernel_ms[k] = 0; c->kernel_launches[k] = 0; }
  return HMGPU_OK;
}

// ---------------------------------------------------------------------------------------------- finer seams
hmgpu_status hmgpu_inverse_transform_batch(hmgpu_ctx* c, int32_t log2_size, int32_t bit_depth, int32_t n, const int16_t* levels,
                                           const int8_t* qp_per, const int8_t* qp_rem, const uint8_t* flags, int16_t* resid) {
  if (!c || log2_size < 2 || log2_size > 5 || n < 1 || !levels || !qp_per || !qp_rem || !flags || !resid) return HMGPU_EINVAL;
  if (bit_depth < 8 || bit_depth > 12) return HMGPU_EUNSUPPORTED;
  hipSetDevice(c->device);
  const size_t elems = (size_t)n << (2 * log2_size);
  int16_t *d_lev = nullptr, *d_res = nullptr; int8_t *d_per = nullptr, *d_rem = nullptr; uint8_t* d_fl = nullptr;
  hmgpu_status st = HMGPU_OK;
  auto fail = [&](hipError_t e) { if (e != hipSuccess && st == HMGPU_OK) { c->last_err = (int32_t)e; st = HMGPU_EDEVICE; } };
  fail(hipMalloc((void**)&d_lev, elems * 2)); fail(hipMalloc((void**)&d_res, elems * 2));
  fail(hipMalloc((void**)&d_per, n)); fail(hipMalloc((void**)&d_rem, n)); fail(hipMalloc((void**)&d_fl, n));
  if (st == HMGPU_OK) {
    fail(hipMemcpy(d_lev, levels, elems * 2, hipMemcpyHostToDevice));
    fail(hipMemcpy(d_per, qp_per, n, hipMemcpyHostToDevice)); fail(hipMemcpy(d_rem, qp_rem, n, hipMemcpyHostToDevice));
    fail(hipMemcpy(d_fl, flags, n, hipMemcpyHostToDevice));
  }
  if (st == HMGPU_OK) {
    launch_itx_flat(log2_size, bit_depth, n, d_lev, d_per, d_rem, d_fl, d_res, c->stream);
    fail(hipGetLastError());
    fail(hipStreamSynchronize(c->stream));
    fail(hipMemcpy(resid, d_res, elems * 2, hipMemcpyDeviceToHost));
  }
  hipFree(d_lev); hipFree(d_res); hipFree(d_per); hipFree(d_rem); hipFree(d_fl);
  return st;
}

hmgpu_status hmgpu_mc_batch(hmgpu_ctx* c, int32_t is_chroma, int32_t bit_depth, const int16_t* ref_plane, int32_t ref_stride,
                            int32_t ref_w, int32_t ref_h, int32_t n, const int32_t* blocks, int32_t bi, int16_t* dst) {
  if (!c || !ref_plane || !blocks || !dst || n < 1 || ref_w < 1 || ref_h < 1 || ref_stride < ref_w) return HMGPU_EINVAL;
  if (bit_depth < 8 || bit_depth > 12) return HMGPU_EUNSUPPORTED;
  hipSetDevice(c->device);
  std::vector<int32_t> off(n);
  size_t total = 0;
  for (int i = 0; i < n; i++) {
    const int w = blocks[i * 6 + 2], h = blocks[i * 6 + 3];
    if (w < 2 || h < 2 || (w & 1) || (h & 1) || w > 64 || h > 64) return HMGPU_EINVAL;
    off[i] = (int32_t)total; total += (size_t)w * h;
  }
  // device copy of the plane with replicated margins (what extendPicBorder gives HM's xPredInterBlk); blocks and MVs must
  // keep the filter window within 96 samples of the plane
  const int M = 96;
  for (int i = 0; i < n; i++) {
    const int sh = is_chroma ? 3 : 2;
    const int bx = blocks[i * 6 + 0] + (blocks[i * 6 + 4] >> sh), by = blocks[i * 6 + 1] + (blocks[i * 6 + 5] >> sh);
    if (bx < -(M - 8) || by < -(M - 8) || bx + blocks[i * 6 + 2] > ref_w + M - 8 || by + blocks[i * 6 + 3] > ref_h + M - 8) return HMGPU_EINVAL;
  }
  const int pitch = (int)align_up((size_t)ref_w + 2 * M, 64) + 64;
  const int prow = ref_h + 2 * M;
  std::vector<int16_t> padded((size_t)pitch * prow, 0);
  for (int y = 0; y < prow; y++) {
    const int16_t* src = ref_plane + (size_t)std::min(std::max(y - M, 0), ref_h - 1) * ref_stride;
    int16_t* dstrow = padded.data() + (size_t)y * pitch;
    for (int x = 0; x < ref_w + 2 * M; x++) dstrow[x] = src[std::min(std::max(x - M, 0), ref_w - 1)];
  }
  int16_t *d_ref = nullptr, *d_dst = nullptr; int32_t *d_blk = nullptr, *d_off = nullptr;
  hmgpu_status st = HMGPU_OK;
  auto fail = [&](hipError_t e) { if (e != hipSuccess && st == HMGPU_OK) { c->last_err = (int32_t)e; st = HMGPU_EDEVICE; } };
  fail(hipMalloc((void**)&d_ref, padded.size() * 2)); fail(hipMalloc((void**)&d_dst, total * 2));
  fail(hipMalloc((void**)&d_blk, (size_t)n * 24)); fail(hipMalloc((void**)&d_off, (size_t)n * 4));
  if (st == HMGPU_OK) {
    fail(hipMemcpy(d_ref, padded.data(), padded.size() * 2, hipMemcpyHostToDevice));
    fail(hipMemcpy(d_blk, blocks, (size_t)n * 24, hipMemcpyHostToDevice));
    fail(hipMemcpy(d_off, off.data(), (size_t)n * 4, hipMemcpyHostToDevice));
  }
  if (st == HMGPU_OK) {
    launch_mc_flat(is_chroma, bit_depth, d_ref + (size_t)M * pitch + M, pitch, ref_w, ref_h, n, d_blk, d_off, bi, d_dst, c->stream);
    fail(hipGetLastError());
    fail(hipStreamSynchronize(c->stream));
    fail(hipMemcpy(dst, d_dst, total * 2, hipMemcpyDeviceToHost));
  }
  hipFree(d_ref); hipFree(d_dst); hipFree(d_blk); hipFree(d_off);
  return st;
}

}  // extern "C"
