// packed_format.h -- layout of the packed picture input (hmgpu_pack_input / hmgpu_decompress_pictures_packed), shared by the host
// packer / validator (hmgpu_packed.hip), the runtime (hmgpu_api.hip) and the device expansion (k_unpack.hip).  The contract is the
// one include/hmgpu.h states; this file names the offsets.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/hmgpu.h"

namespace hmgpu {
namespace packed {

constexpr uint32_t kMagic = 0x4B504D48u;   // "HMPK"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kAlign = 16;            // every section starts on a 16-byte boundary

// run groups: fields a run carries together (one 8-byte tuple per run)
enum { G_CU = 0, G_TU, G_L0, G_L1, G_INTRA, kGroups };
// sections: per-CTU indices, then per group (run starts, run ends, tuples), then the levels (CTU starts, piece table, piece data)
enum { S_CTU = 0, S_RUN0 = 1, S_LSTART = S_RUN0 + 3 * kGroups, S_LTAB, S_LDATA, kSections };
constexpr int sec_starts(int g) { return S_RUN0 + 3 * g; }
constexpr int sec_ends(int g) { return S_RUN0 + 3 * g + 1; }
constexpr int sec_tuples(int g) { return S_RUN0 + 3 * g + 2; }

// header: 8 words, then {offset, size} in bytes per section; padded to a multiple of kAlign
struct Header {
  uint32_t magic, version, num_ctus, parts, groups /* bit g: run group g present */, bytes /* the whole blob */, reserved[2];
  uint32_t sec[kSections][2];
};
constexpr size_t kHeaderBytes = (sizeof(Header) + kAlign - 1) / kAlign * kAlign;
static_assert(sizeof(Header) == 8 * 4 + kSections * 8, "packed header layout");

// tuple bytes per group
//   CU:    depth, part_size, pred_mode, qp, transquant_bypass, ipcm, 0, 0
//   TU:    tr_idx, cbf[0..2], transform_skip[0..2], 0
//   L0/L1: mv hor (int16), mv ver (int16), ref_idx, 0, 0, 0
//   INTRA: intra_dir[0], intra_dir[1], 0 x 6
// a group left out reads as one run per CTU of its default tuple: zero, except ref_idx = -1 (list 1)
constexpr uint32_t kRaw = 0x80000000u;     // level table word 1: the piece is stored raw (else: the number of (position, value) pairs)

inline size_t align(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

}  // namespace packed
}  // namespace hmgpu

namespace hmgpu {
namespace packed {

// what the runtime takes from a validated blob (host side; the same values stage_inputs derives from the arrays)
struct Summary {
  uint32_t groups = 0;
  size_t n_intra = 0;                  // partitions of intra CUs
  bool cells = false;                  // PUs that cut an 8x8 luma tile (k_mc_cells.hip)
  bool any_pcm = false, any_bypass = false, flags_used = false;
  uint32_t max_slice = 0;
  const uint32_t* ctu = nullptr;       // [num_ctus] slice | tile << 16 (inside the blob)
};

// validation of `bytes` bytes at `blob` against the geometry of `seq` (4:0:0 / 4:2:0 only): every offset, every run end and every level
// piece's place and size are checked, so that the device expansion may trust the blob.  HMGPU_EINVAL when anything is out of place.
// positions: also walk every (position, value) pair (strictly ascending, inside the piece).  Both hmgpu_unpack_input and the runtime do
// (the runtime validates the blobs of one call on threads of their own: 1.1 M positions of a 2160p picture take 0.2 to 0.4 ms).
hmgpu_status validate(const hmgpu_seq_params* seq, const void* blob, size_t bytes, Summary* out, bool positions);

}  // namespace packed
}  // namespace hmgpu
