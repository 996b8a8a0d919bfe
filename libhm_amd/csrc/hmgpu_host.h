// hmgpu_host.h -- what the units of the host runtime (hmgpu_api.hip, hmgpu_input.hip, hmgpu_output.hip, hmgpu_export.hip,
// hmgpu_side.hip, hmgpu_analysis.hip, hmgpu_import.hip, hmgpu_conceal.hip) share: the context and its pictures, the small tools every unit uses, and the helpers that
// more than one unit calls.  Internal: not installed, not included by any kernel file.
#pragma once
#include "hmgpu_dev.h"

#include <atomic>
#include <chrono>
#include <cstring>
#include <unordered_map>
#include <vector>

// Shared host-side names live in a namespace of hidden visibility: they link across the units and stay out of the library's dynamic
// symbol table.  What one unit alone uses is static or anonymous in that unit.
namespace hmgpu_host __attribute__((visibility("hidden"))) {
using namespace hmgpu;

enum { K_PREP = 0, K_MC_LUMA, K_MC_CHROMA, K_ITX, K_DBK_VER, K_DBK_HOR, K_SAO, K_EXTEND, K_H2D, K_INTRA, K_FILTER, K_UNPACK, K_MC_CELLS };

struct SliceCall { int first_ctu, num_ctus, slice_idx; bool intra, wp, cells, bi, islice, dir; };   // dir: the call came with intra_dir[]; intra: the range holds intra CUs the device reconstructs; islice: mostly intra CUs;
                                                                                    // cells: it holds PUs that cut an 8x8 luma tile (k_mc_cells.hip); bi: B slices

struct Picture {
  bool in_use = false;
  bool sao_applied = false;
  bool filter_ready = false;            // SAO parameters staged
  bool sao_any = false;
  bool extended = false;                // margins of the final planes hold the replicated border
  // loop-filter export: a filter call has run on the handle's current picture, and that call staged SAO parameters (an SAO stage with
  // sao_enabled).  Cleared with sao_applied: acquire, upload, a received picture, and every later decompress call (filter_forget)
  bool lf_called = false, lf_sao = false;
  std::vector<SliceCall> calls;
  // device allocations (owned)
  void* planes = nullptr;               // rec[3] + sao[3]
  void* meta = nullptr;                 // raw HM arrays
  void* coef = nullptr;
  void* pcm = nullptr;                  // PCM sample buffers, allocated when the first PCM CU shows up
  void* ccp = nullptr;                  // cross-component prediction weights (4:4:4), allocated with the first picture that carries them
  void* blob = nullptr;                 // device copy of a packed input (hmgpu_decompress_pictures_packed), allocated when first used
  void* derived = nullptr;              // blk, tu lists, counters, sao params, slices
  uint8_t* sl_table = nullptr;          // device: expanded scaling-list matrices (inside `derived`)
  uint32_t* coef_start = nullptr;       // device: [3][num_ctus + 1] CTU starts of compact levels (inside `derived`)
  std::vector<uint8_t> sl_host;         // host copy the asynchronous upload reads from
  PicDev dev;                           // host mirror of the device descriptor
  std::vector<SliceDev> slices;         // host mirror of the slice table
  std::vector<SaoDev> h_saoprm;         // host copy of the resolved SAO parameters the asynchronous upload reads from
  std::vector<uint16_t> h_slice_idx, h_tile_idx;   // host mirrors of the per-CTU slice / tile index (SAO merge resolution needs them)
  int max_slice = -1;
  bool flags_staged = true;             // the device copies of transform_skip / bypass / ipcm may hold non-zero values
  uint64_t last_use = 0;                // use_seq of the last batch of kernels that read this picture's input arrays (0: none)
  // CTUs whose input arrays decompress calls have staged since the picture was acquired (hmgpu_pictures_export_motion: a picture has
  // side information when all are); cleared by acquire, upload and hmgpu_picture_commit_received
  std::vector<bool> covered;
  int covered_ctus = 0;
  // CTUs hmgpu_pictures_conceal has filled since the picture was acquired (hmgpu_picture_concealed_ctus)
  std::vector<bool> concealed;
  int concealed_ctus = 0;
};

struct EventPair { hipEvent_t a, b; int kind; };

}  // namespace hmgpu_host

using namespace hmgpu;
using namespace hmgpu_host;

// one page-locked block that holds a picture's input arrays in the order the device keeps them (hmgpu_staging_alloc)
struct hmgpu_staging {
  char* host = nullptr;
  size_t meta_bytes = 0, coef_bytes = 0, start_bytes = 0;   // metadata block | dense-capacity levels | [3][num_ctus + 1] CTU starts
  size_t grp[5] = {0, 0, 0, 0, 0};                         // carve_meta: where the optional groups of the metadata block start
  uint64_t copy_seq = 0;                                   // the staging pass (hmgpu_decompress_pictures) that last read the block ...
  hmgpu_ctx* reader = nullptr;                             // ... and the context it ran on (the owner, or one the block is shared with)
  hmgpu_ctx* owner = nullptr;
  std::vector<hmgpu_ctx*> sharers;                         // hmgpu_staging_share: contexts that take the block's arrays in one DMA too
  hmgpu_ctu_meta m;
  hmgpu_coeffs co;
};

struct hmgpu_ctx {
  hmgpu_seq_params seq;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;      // second lane of the replay pipeline (hmgpu_set_streams)
  // host -> device staging of hmgpu_decompress_pictures runs on its own stream, so that the inputs of the next batch travel while the
  // kernels of this one run.  Two rings of events order it against the compute stream: copy_ev (inputs of a batch have arrived) and
  // use_ev (the kernels that read a picture's inputs have finished: its device arrays may be overwritten)
  hipStream_t copy_stream = nullptr;
  // ... and every second picture of a call on a second one: one stream's copies run on one DMA engine (~40 GB/s from page-locked memory on
  // this host), two reach 50-57 (tools/dbg/pcie.py).  The second lane joins the first before copy_ev is recorded (copy_join).
  hipStream_t copy_stream2 = nullptr;
  hipEvent_t copy_join = nullptr;
  hipEvent_t copy_ev[8] = {}, use_ev[8] = {};
  uint64_t copy_seq = 0, use_seq = 0;
  std::vector<hmgpu_staging*> stagings;
  std::vector<hmgpu_staging*> shared_stagings;   // blocks of other contexts (hmgpu_staging_share): recognised, not owned
  // packed blobs and the staging pass that last copied them (hmgpu_packed_wait); entries whose copy is known to be done are dropped
  std::unordered_map<const void*, uint64_t> packed_reads;
  // Small host structures (descriptors, slice table entries, resolved SAO parameters) travel through a ring of page-locked memory: an
  // asynchronous copy from pageable memory makes the runtime stage the bytes itself, 20-100 us of the calling thread per copy (the resolved
  // SAO parameters of a picture: 0.18 ms; sixteen pictures per call spent 7 of their 7.7 ms on the host that way, round 4).  Eight segments; a
  // segment is reused when the events recorded at its close -- one per stream that may carry its copies -- have passed.
  static constexpr int kBounceSegs = 8;
  static constexpr size_t kBounceSeg = 1u << 20;
  char* bounce = nullptr;
  int bounce_seg = 0;
  size_t bounce_off = 0;
  hipEvent_t bounce_ev[kBounceSegs][3] = {};
  bool bounce_used[kBounceSegs] = {};
  // HMGPU_HOST_TIMING=1: wall time the calling thread spends inside the batch entry points, by part (printed by hmgpu_destroy)
  bool host_timing = false;
  double host_s[6] = {0, 0, 0, 0, 0, 0};
  uint64_t host_calls = 0;
  hipEvent_t dl_ev[32] = {};           // hmgpu_picture_download_begin tickets: ticket t completes with dl_ev[t % 32]
  std::atomic<uint64_t> dl_seq{0};
  // hmgpu_picture_hash_begin: MD5 chains of finished pictures over packed copies in a ring of slots; launched in batches (one lane per
  // plane, k_md5) on low-priority streams of their own
  static constexpr int kHashSlots = 96, kHashBatch = 32, kHashStreams = 1;   // (a batch: 96 chains = two waves; several streams shared hardware queues with each other and the context's own)
  hipStream_t hash_stream[kHashStreams] = {};
  hipEvent_t hash_packed[kHashSlots] = {}, hash_done[kHashSlots] = {};
  int hash_done_slot[kHashSlots] = {};   // the slot whose hash_done event stands for the batch a slot's chains ran in
  uint8_t* hash_buf[kHashSlots] = {};    // device: the packed planes, allocated when first used
  uint32_t* hash_dev = nullptr;          // device: [kHashSlots][12] state words
  uint32_t* hash_host = nullptr;         // page-locked: the same
  uint64_t hash_seq = 0, hash_launched = 0, hash_launches = 0;
  hipEvent_t xfer_ev[2] = {};            // hmgpu_picture_transfer: source ready / copy done
  hipEvent_t exp_ev[2] = {};             // hmgpu_picture_export on a caller's stream: picture ready / export done (created when first used)
  // the export's tables in device memory and, page-locked, the same bytes on their way over; `done` is recorded behind the last export
  // that read them (pending), and the buffer is rewritten only after it (hmgpu_export.hip: table_room)
  struct TableBuf {
    char* dev = nullptr;
    char* host = nullptr;
    size_t cap = 0;
    bool pending = false;
    hipEvent_t done = nullptr;
    void release() {
      if (done) hipEventDestroy(done);
      if (dev) (void)hipFree(dev);
      if (host) (void)hipHostFree(host);
    }
  };
  // hmgpu_picture_export_scaled: one slot per export shape, least recently used slot reused
  struct ScaleSlot : TableBuf {
    int32_t key[8] = {};                 // crop[4], output width / height, filter, RGB | the classes' starting tiles (log2 tw, log2 th) << 1
    bool valid = false;
    uint64_t used = 0;
    ScaleClass cls[2];
  };
  static constexpr int kScaleSlots = 8;
  ScaleSlot scale_slot[kScaleSlots];
  uint64_t scale_tick = 0;
  // hmgpu_pictures_export_windows, windows that differ: the tables, spans and per-picture classes of one call (no key ever repeats, so
  // nothing is cached): a ring of per-call buffers, the next one rewritten only after the export that read it has finished
  static constexpr int kWindowBufs = 4;
  TableBuf window_buf[kWindowBufs];
  int window_next = 0;
  // hmgpu_colour_lut_create: the live LUTs (nodes, then the shaper, in one device allocation); `done` as for the tables above, and
  // hmgpu_colour_lut_destroy waits for it before the memory goes
  struct ColourSlot {
    int64_t handle = 0;                  // 0: free
    char* dev = nullptr;
    ColourLut lut = {};
    bool pending = false;
    hipEvent_t done = nullptr;
    void release() {
      if (done) hipEventDestroy(done);
      if (dev) (void)hipFree(dev);
      handle = 0; dev = nullptr; done = nullptr; pending = false;
    }
  };
  ColourSlot colour_slot[HMGPU_COLOUR_MAX_LUTS];
  uint64_t xfer_bytes = 0;
  uint32_t* dl_fault = nullptr;        // [32] page-locked: the picture's fault word (k_intra's bounded spin) as it stood behind the copies of ticket t
  std::vector<int> touched;            // pictures the entry point under way has enqueued work on, in any role (commit_use)
  std::vector<int> intra_launched;    // pictures whose intra kernel ran since the last fault check (k_intra's bounded spin)
  void* scratch = nullptr;            // device scratch of the output calls (packed download, picture hash): grown on demand, kept
  size_t scratch_bytes = 0;
  uint8_t* conceal_masks = nullptr;   // device: the CTU masks of one hmgpu_pictures_conceal call, kMaxBatch of them (allocated when first used)
  hipEvent_t lane_ev[2] = {nullptr, nullptr};
  int replay_streams = 1;
  int32_t last_err = 0;
  // geometry
  int ctu = 64, pw = 16, parts = 256, ctus_w = 0, ctus_h = 0, num_ctus = 0;
  int fmt = 1, csx = 1, csy = 1;          // chroma_format_idc (0 handled as 1: the chroma planes exist and are left alone) and its subsampling
  int pitch[3] = {0, 0, 0}, rows[3] = {0, 0, 0};
  int mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
  int grid_w = 0, grid_h = 0;
  uint32_t tu_cap[4] = {0, 0, 0, 0};
  size_t coef_elems[3] = {0, 0, 0};
  std::vector<Picture> pics;
  PicDev* d_pics = nullptr;
  PlaneSet* d_finals = nullptr;
  // sample planes of all device pictures in ONE allocation: picture i at plane_slab + i * 2 * plane_bytes (reconstruction planes, then
  // SAO planes), so that a kernel finds the final planes of a reference picture by arithmetic on its handle (McArgs, k_mc.hip)
  char* plane_slab = nullptr;
  size_t plane_bytes = 0;
  int32_t* d_ctu_order = nullptr;     // CTU addresses by anti-diagonal (dispatch order of the intra wavefront)
  std::vector<PlaneSet> h_finals;
  // profiling
  bool profiling = false;
  std::vector<EventPair> pending;
  std::vector<EventPair> free_events;
  double kernel_ms[HMGPU_NUM_KERNELS] = {0};
  uint64_t kernel_launches[HMGPU_NUM_KERNELS] = {0};
};

namespace hmgpu_host __attribute__((visibility("hidden"))) {

struct HostTimer {                      // adds the time between construction and destruction to one slot (when timing is on)
  hmgpu_ctx* c; int slot; std::chrono::steady_clock::time_point t0;
  HostTimer(hmgpu_ctx* c_, int slot_) : c(c_), slot(slot_) { if (c->host_timing) t0 = std::chrono::steady_clock::now(); }
  ~HostTimer() { if (c->host_timing) c->host_s[slot] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};

#define HIP_TRY(ctx, expr)                                   \
  do {                                                       \
    hipError_t e__ = (expr);                                 \
    if (e__ != hipSuccess) {                                 \
      (ctx)->last_err = (int32_t)e__;                        \
      return HMGPU_EDEVICE;                                  \
    }                                                        \
  } while (0)

// host -> device copy of a small structure on stream hs: through the context's page-locked ring (hmgpu_ctx::bounce) when it fits.
// *staged (if asked for): the bytes were taken into the ring, so `src` is the caller's again on return; false: the copy reads `src` itself
hipError_t h2d_small(hmgpu_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t hs, bool* staged = nullptr);

size_t align_up(size_t v, size_t a);

struct Carver {                       // sub-allocates one device block, 256-byte aligned pieces
  char* base; size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename T> T* take(size_t n) { T* p = base ? (T*)(base + off) : nullptr; off += align_up(n * sizeof(T), 256); return p; }
};

void* ctx_scratch(hmgpu_ctx* c, size_t bytes);          // device scratch of the output side, grown on demand
hmgpu_status check_faults(hmgpu_ctx* c);                // after a synchronisation: did an intra wavefront give up waiting?
void touch(hmgpu_ctx* c, int pic);                      // the entry point under way enqueues work on `pic` ...
void commit_use(hmgpu_ctx* c);                          // ... and ends: one use event for every picture touched

void prof_begin(hmgpu_ctx* c, int kind, EventPair* ep);
void prof_end(hmgpu_ctx* c, EventPair* ep);
void prof_drain(hmgpu_ctx* c);
struct ProfScope {
  hmgpu_ctx* c; EventPair ep;
  ProfScope(hmgpu_ctx* ctx, int kind) : c(ctx) { prof_begin(c, kind, &ep); }
  ~ProfScope() { prof_end(c, &ep); if (c->pending.size() > 8192) prof_drain(c); }
};

void carve_meta(Carver& m, PicDev& d, size_t np, int num_ctus, size_t* grp = nullptr);
hmgpu_status push_picdev(hmgpu_ctx* c, int pic);
hmgpu_status push_final(hmgpu_ctx* c, int pic, hipStream_t hs);
bool valid_pic(const hmgpu_ctx* c, hmgpu_pic pic);
void coverage_clear(Picture& p);
inline void filter_forget(Picture& p) { p.lf_called = false; p.lf_sao = false; }
void coverage_add(const hmgpu_ctx* c, Picture& p, int first_ctu, int num_ctus);
hmgpu_status ensure_extended(hmgpu_ctx* c, int pic);

// kernel sequencing (hmgpu_api.hip)
hmgpu_status run_recon(hmgpu_ctx* c, const Batch& b, bool any_intra, bool any_wp, bool any_cells, bool any_bi, bool any_islice);
hmgpu_status run_filter(hmgpu_ctx* c, const Batch& b, int stages, bool* fused);   // *fused: the fused kernel ran and wrote the margins
hmgpu_status stage_sao(hmgpu_ctx* c, Picture& p, const hmgpu_pic_params* pp, const hmgpu_sao_param* sao,
                       const std::vector<uint16_t>& slice_idx, const std::vector<uint16_t>& tile_idx);

// validation rules and the stream bracket of the exports (hmgpu_export.hip), shared with hmgpu_side.hip and hmgpu_analysis.hip
void chroma_shifts(int fmt, int* csx, int* csy);
hmgpu_status scale_desc_ok(const hmgpu_export_scale* sc);
hmgpu_status crop_ok(const hmgpu_seq_params* seq, const int32_t cr[4], const hmgpu_export_scale* sc, int* w, int* h);
hmgpu_status window_ok(const hmgpu_seq_params* seq, const hmgpu_export_window& win, const hmgpu_export_scale* sc, int* w, int* h);
bool device_span_ok(const void* p, size_t bytes, int device);
// packed YUV (include/hmgpu.h "packed YUV"): what a word format is made of -- chroma format, depth, the alignment of its element, the
// kernel family of the export (kPack*) with what tells its members apart, the largest A; false: no such format.  The export and the
// import entries look a format up after their rules have accepted it (yuvpack_rules, import_yuvpack_rules): the later look-ups of a
// call cannot fail.  yuvpack_row_bytes: the bytes of a row of w pixels
struct YuvPackFormat { int cf, depth, align, fam, yfirst, shift, amax; };
bool yuvpack_format(int format, YuvPackFormat* p);
int yuvpack_row_bytes(const YuvPackFormat& p, int w);
hmgpu_status export_open(hmgpu_ctx* c, int32_t on_stream, void* stream, hipStream_t* hs);
hmgpu_status export_end(hmgpu_ctx* c, int n, const hmgpu_pic* pics, int32_t on_stream, hipStream_t hs);

// the destinations of a side-information export, `slots` of them, a null one not written: element alignment, strides against the extents
// they step over (pstride null: one plane per slot), and the whole span of n pictures inside one allocation of the context's device,
// which it makes the current one.
// vec: bit k set when slot k may take stores of `granule` bytes (0: four elements)
template <class Plan>
hmgpu_status strided_dst_ok(const hmgpu_ctx* c, const Plan& plan, int slots, int n, void* const* dst, const int64_t* pitch,
                            const int64_t* pstride, const int64_t* bstride, int granule, int* vec) {
  hipSetDevice(c->device);
  bool any = false;
  *vec = 0;
  for (int k = 0; k < slots; k++) {
    if (!dst[k]) continue;
    if (!plan.channels[k]) return HMGPU_EINVAL;                       // a slot this call does not have
    any = true;
    const int64_t es = plan.elem_bytes[k], g = granule ? granule : 4 * es;
    if (pitch[k] < plan.row_bytes[k] || pitch[k] > ((int64_t)1 << 40)) return HMGPU_EINVAL;
    const int64_t plane = pitch[k] * (plan.height[k] - 1) + plan.row_bytes[k];
    int64_t pic = plane;
    if (pstride) {
      if (pstride[k] < plane || pstride[k] > ((int64_t)1 << 48) || pstride[k] % es) return HMGPU_EINVAL;
      pic = pstride[k] * (plan.channels[k] - 1) + plane;
    }
    if (bstride[k] < pic || bstride[k] > ((int64_t)1 << 56)) return HMGPU_EINVAL;
    if ((uintptr_t)dst[k] % es || pitch[k] % es || bstride[k] % es) return HMGPU_EINVAL;
    if (!device_span_ok(dst[k], (size_t)((n - 1) * bstride[k] + pic), c->device)) return HMGPU_EINVAL;
    if ((uintptr_t)dst[k] % g == 0 && pitch[k] % g == 0 && bstride[k] % g == 0 && (!pstride || pstride[k] % g == 0)) *vec |= 1 << k;
  }
  return any ? HMGPU_OK : HMGPU_EINVAL;
}

}  // namespace hmgpu_host
