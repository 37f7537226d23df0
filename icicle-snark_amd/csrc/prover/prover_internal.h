// prover_internal.h — types and helpers shared by the translation units of the prover host
// (containers.cpp, cache.cpp, prover.cpp, assemble.cpp, multi.cpp).  Nothing here crosses the C ABI.
//
//   containers.cpp  snarkjs .zkey / .wtns containers        ← src/file_wrapper.rs:45-208, src/zkey.rs:47-85
//   cache.cpp       CacheManager::compute (ZKeyCache build) ← src/cache.rs:117-241
//   prover.cpp      construct_r1cs + groth16_commitments on ONE device, the C API        ← src/proof_helper.rs:31-241, src/lib.rs:33-61
//   assemble.cpp    blinding, affine conversion, JSON       ← src/proof_helper.rs:274-316, src/conversions.rs:30-56
//   multi.cpp       the same prove over a GROUP of devices in one process (device string "HIP:0-7"), SURVEY.md §8e
#pragma once
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <stdarg.h>
#include <string.h>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/groth16_prover.h"
#include "../common.h"
#include "../ec.h"
#include "../msm_plan.h"
#include "../ntt_fuse.h"
#include "../workers.h"
#include "cold_feed.h"
#include "qap.h"
#include "shard_ranges.h"

namespace isnark {
const bn254::fe* ntt_domain_table(int* log_n); // ntt.hip
namespace vb {
struct DeviceSession; // verify_batch.h
}

namespace prover {
using namespace bn254;

// ---- errors: one thread-local text per thread (groth16_last_error); worker threads hand theirs to the caller
int fail(int code, const char* fmt, ...);
const char* last_error_text();
void set_error_text(const char* text);
#define P_HIP(call)                                                                                                              \
  do {                                                                                                                           \
    hipError_t e__ = (call);                                                                                                     \
    if (e__ != hipSuccess) return ::isnark::prover::fail((int)ICICLE_UNKNOWN_ERROR, "%s: %s", #call, hipGetErrorString(e__));    \
  } while (0)
#define P_ICICLE(call)                                                                                                           \
  do {                                                                                                                           \
    eIcicleError e__ = (call);                                                                                                   \
    if (e__ != ICICLE_SUCCESS) return ::isnark::prover::fail((int)e__, "%s failed (%d): %s", #call, (int)e__, icicle_snark_last_error()); \
  } while (0)
enum { ERR_IO = -1, ERR_FORMAT = -2, ERR_ARG = -3, ERR_NOCACHE = -4, ERR_DEVICE = -5 /* groth16_zkey_check, where > 0 is a verdict */ };

using isnark::ms_since; // common.h

// the domain of a circuit: the smallest power of two >= mConstraints + n_public + 1 (snarkjs' rule), *log2 its exponent
inline uint64_t circuit_domain(uint64_t n_constraints, uint64_t n_public, uint32_t* log2)
{
  uint64_t domain = 1;
  *log2 = 0;
  while (domain < n_constraints + n_public + 1) domain <<= 1, (*log2)++;
  return domain;
}

// ---- containers (containers.cpp)
struct Section {
  const uint8_t* p = nullptr;
  uint64_t size = 0;
  int count = 0;
};
int read_sections(const uint8_t* data, size_t len, const char* type, uint32_t max_version, std::vector<Section>& out);
int unique_section(const std::vector<Section>& s, size_t id, const Section** sec);
struct SectionEntry { // of a container read_sections has passed, as the file orders them (a writer that keeps the order walks these)
  uint32_t id;
  uint64_t size;
  const uint8_t* p;
};
std::vector<SectionEntry> sections_in_order(const uint8_t* data);
// what a writer puts in front: the container's 12 bytes, a section's 12 bytes; w moves behind them
inline void put_container_head(uint8_t*& w, const char* magic, uint32_t version, uint32_t n_sections)
{
  memcpy(w, magic, 4);
  memcpy(w + 4, &version, 4);
  memcpy(w + 8, &n_sections, 4);
  w += 12;
}
inline void put_section(uint8_t*& w, uint32_t id, uint64_t size)
{
  memcpy(w, &id, 4);
  memcpy(w + 4, &size, 8);
  w += 12;
}
// What a zkey says about itself: the sections 2 … 9 and the header's fields.  zkey_layout is the ONE statement of the container
// and header rules — the loader (build_cache), the key check and the vk export all read a key through it.  Checked, in this
// order: section 1 and the protocol; sections 2, (3,) 4 … 9 present once; header length, field sizes, moduli, a power-of-two
// domain, n_public; the coefficient section's size and count (n_coef comes from the section's length — the declared count in its
// first four bytes is not read, like src/cache.rs:129); the point sections' sizes.  Unknown sections are ignored.
// `need_ic`: section 3 (IC) is part of the checks, as the key check and the vk export want it; the prover does not read it and
// loads keys without it (need_ic = false: sec[3] is the section when there is exactly one, else null, and nothing of it is checked).
// `secs` owns the table L->sec points into; all pointers lead into the caller's `data`.
constexpr size_t COEF_RECORD_BYTES = 12 + 32;
struct PackedZkey;
struct ZkeyLayout {
  uint32_t n8q = 0, n8r = 0, n_vars = 0, n_public = 0, domain = 0, n_coef = 0;
  fe q, r;
  const uint8_t* header_points = nullptr; // α₁ β₁ β₂ γ₂ δ₁ δ₂: 64 / 128 bytes each, Montgomery form
  const Section* sec[10] = {};
  const uint8_t* records() const { return sec[4]->p + 4; } // n_coef × COEF_RECORD_BYTES: {m:u32 c:u32 s:u32 value[32]}, src/cache.rs:126-166
  const PackedZkey* packed = nullptr; // set by zkez_layout alone: sec[3 … 9] are then the PACKED sections and records() is not to be read
};
int zkey_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, ZkeyLayout* L, bool need_ic = true);
// A PACKED proving key ("zkez", version 1; include/groth16_prover.h has the container, zkey_pack29.h the coefficient's form).
// Section 4 of it, and the body groth16_zkey_coefs_pack writes: {u32 declared_count, u32 n_coef, u64 payload_bytes}, n_coef × 12
// bytes of {m, c, s}, n_coef code bytes, the directory of n_blocks + 1 u64 (blocks of 256 coefficients), the payload.
// zkez_coefs_layout demands that the size equals the sum of these parts and runs wz_check_directory (ERR_FORMAT, each rule with its
// text): block b's payload [dir[b], dir[b + 1]) then lies inside the payload and spans at most 8192 bytes whatever the codes say.
struct ZkezCoefs {
  uint32_t declared = 0, n_coef = 0;
  uint64_t n_blocks = 0, payload_bytes = 0;
  const uint8_t *triples = nullptr, *codes = nullptr, *dir = nullptr, *payload = nullptr; // into the caller's image, unaligned
};
int zkez_coefs_layout(const uint8_t* body, uint64_t size, ZkezCoefs* C);
constexpr uint64_t ZKEZ_COEFS_HEAD = 16;
inline uint64_t zkez_coefs_bytes(uint64_t n_coef, uint64_t payload_bytes) { return ZKEZ_COEFS_HEAD + 13 * n_coef + 8 * ((n_coef + 255) / 256 + 1) + payload_bytes; }
// zkez_layout: the section table under magic "zkez", version 1 — a .zkey is refused as any foreign magic is, and zkey_layout takes
// none of these; zkey_layout's rules for sections 1 and 2 (the same code); sections 3 … 9 once each; every point section with
// exactly HALF the bytes zkey_layout demands (ERR_FORMAT naming the section and both sizes); section 4 through zkez_coefs_layout.
// All of it before a byte goes up.  L is filled as zkey_layout fills it, n_coef from section 4's second word, and L->packed = P.
struct PackedZkey {
  ZkezCoefs coefs;
  uint64_t unpacked_bytes = 0; // of the .zkey it came from
};
int zkez_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, ZkeyLayout* L, PackedZkey* P);
struct MappedFile {
  const uint8_t* data = nullptr;
  size_t len = 0;
  int fd = -1;
  ~MappedFile();
  int open_ro(const char* path, bool read_ahead = true); // read_ahead = false: a file of which only ranges are read (a .ptau)
};
struct Wtns {
  uint32_t n8 = 0, n_witness = 0;
  fe q;
  const uint8_t* values = nullptr; // n_witness × 32 B standard form
};
int parse_wtns(const uint8_t* data, size_t len, Wtns& w);
// A PACKED witness (wtns_pack.h has the value's form; include/groth16_prover.h the container): the section table under magic "wtnz",
// version 1 — a .wtns is refused as any foreign magic is, and parse_wtns takes none of these — sections 1 … 4 once each; section 1
// is a .wtns header (n8 = 32, 40 bytes); section 2 holds n_witness codes; section 3 the directory of n_blocks + 1 u64; and the
// directory begins at 0, never decreases, spans at most 8192 bytes a block and ends at section 4's size (ERR_FORMAT, each with its
// own text).  The prime is read, not judged: wtnz_is_bn254 / check_witness do that.  Every pointer leads into the caller's `data`.
struct WtnzLayout {
  uint32_t n8 = 0, n_witness = 0;
  fe q;
  const uint8_t* header = nullptr;  // section 1, 40 bytes
  const uint8_t* codes = nullptr;   // n_witness bytes
  const uint8_t* dir = nullptr;     // (n_blocks + 1) × u64, unaligned
  const uint8_t* payload = nullptr; // payload_bytes
  uint64_t n_blocks = 0, payload_bytes = 0;
};
int wtnz_layout(const uint8_t* data, size_t len, WtnzLayout* L);
int wtnz_is_bn254(const WtnzLayout& L); // ERR_FORMAT unless the header's prime is r
// ---- the decode on a device (wtns_pack.hip)
// The fault of a decode: kind 0 = none, else GROTH16_WTNZ_* of the LOWEST faulty element, and how many there are
struct WtnzFault {
  int kind = 0;
  uint64_t element = 0, count = 0;
};
int wtnz_fail(const WtnzFault& f); // ERR_FORMAT "wtnz: element E: kind"
size_t wtnz_device_bytes(const WtnzLayout& L); // the room wtnz_decode_on_device wants at d_buf (a hipMalloc'd base)
// Sections 2 … 4 up into d_buf (pinned staging; landed on return), ONE launch on `st` that writes n_witness standard-form values to
// d_out, the tally down: synchronous.  0 and *fault, or a device error.  upload_ms / kernel_ms (may be null; kernel_ms costs two
// events) are ADDED to / set.  The caller has made `dev` the active device.
int wtnz_decode_on_device(int dev, hipStream_t st, const WtnzLayout& L, uint8_t* d_buf, fe* d_out, WtnzFault* fault, double* upload_ms, double* kernel_ms);
// What an .r1cs says about itself (iden3 binary format): the header's fields and section 2, the constraints —
// n_constraints × {A, B, C}, each linear combination a u32 count and count × {u32 wire, 32-byte standard-form value}.
// r1cs_layout checks the container, section 1 and 2 present once, the field; r1cs_walk bounds every record (containers.cpp).
// With rowptr from the walk, term t of row ρ sits at byte R1CS_TERM_BYTES·t + 4·(ρ + 1) of the payload.
constexpr size_t R1CS_TERM_BYTES = 4 + 32;
struct R1csLayout {
  uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, n_constraints = 0;
  uint64_t n_labels = 0;
  const uint8_t* payload = nullptr; // section 2
  uint64_t payload_bytes = 0;
  uint32_t n_public() const { return n_pub_out + n_pub_in; }
};
int r1cs_layout(const uint8_t* data, size_t len, R1csLayout* L);
int r1cs_walk(const R1csLayout& L, std::vector<uint32_t>& rowptr, uint64_t* n_terms);
// What a prepared .ptau says about itself (snarkjs' powers-of-tau container after `powersoftau prepare phase2`): section 1 is
// {n8 = 32, q, power, ceremonyPower}; sections 4, 5, 6 hold [α·τ^i]₁, [β·τ^i]₁ and [β]₂; sections 12, 13, 14, 15 hold [L_j(τ)]₁,
// [L_j(τ)]₂, [α·L_j(τ)]₁ and [β·L_j(τ)]₁, one block per power p = 0, 1, … of 2^p elements beginning at element 2^p − 1 (section
// 12 goes on to power + 1).  All points uncompressed, affine, Montgomery form.  ptau_layout checks the container, the header
// and that sections 4, 5, 6 (with their first element) and 12 … 15 are present once; of the lengths it demands nothing more —
// ptau_block is what bounds a block a caller is about to read.
struct PtauLayout {
  uint32_t power = 0, ceremony_power = 0;
  const Section* sec[16] = {};
};
int ptau_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L);
// An UNPREPARED .ptau, what groth16_ptau_prepare takes: the same container and section 1; sections 2 … 7 once each — [τ^i]₁ for
// i < 2^(power+1) − 1, [τ^i]₂, [α·τ^i]₁ and [β·τ^i]₁ for i < 2^power, [β]₂, the contributions — with exactly these element counts; a
// file that has one of 12 … 15 is refused with a message of its own.  ptau_prepared_section_bytes: what prepare writes for 12 … 15.
int ptau_unprepared_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L);
uint64_t ptau_prepared_section_bytes(uint32_t power, int sid);
// A .ptau in EITHER form, what groth16_ptau_verify takes: sections 2 … 7 as ptau_unprepared_layout demands them, and of 12 … 15 none
// (*prepared = false) or all four, each with exactly ptau_prepared_section_bytes (ERR_FORMAT otherwise).  A power above 27 is ERR_ARG.
int ptau_either_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L, bool* prepared);
// A PACKED powers-of-tau file, what groth16_ptau_unpack takes (ptau_pack.hip; include/groth16_prover.h has the form): a .ptau's
// section table and section 1 under magic "ptaz", version 1 — a .ptau is refused as any foreign magic is, and no .ptau reader takes
// this — sections 2 … 7 once each and of 12 … 15 none or all four, every point section with exactly ptau_packed_section_bytes
// (ERR_FORMAT naming the section and both sizes).  A power above 27 is ERR_ARG.
int ptau_packed_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L, bool* prepared);
uint64_t ptau_packed_section_bytes(uint32_t power, int sid); // sid 2 … 6, 12 … 15
// block p of section sid (elements of elem_bytes): its first byte, after checking that it lies inside the section
int ptau_block(const PtauLayout& L, int sid, uint32_t p, size_t elem_bytes, const uint8_t** out);
// the blocks a verify of a key with domain 2^k reads — block k of 12 … 15 and block k + 1 of 12 — lie inside their sections
// (ERR_FORMAT), after power >= k (ERR_ARG, both numbers in the text)
int ptau_blocks_for_domain(const PtauLayout& L, uint32_t k);

// ---- the device-resident cache of one zkey on ONE device (cache.cpp)
constexpr size_t PARTIALS_STRIDE = 64 * 16 * 256; // ≥ W·bpw·sizeof(XYZZ) for any geometry (W ≤ 64, bpw ≤ 16, G2 256 B)

struct Shard {
  uint32_t lo = 0, hi = 0; // [lo, hi) of the full base array
  void* d_points = nullptr; // internal encoding; in table mode W rows of len() points (row w = 2^(c·w)·P, msm_plan.h)
  uint32_t stride = 1, first = 0; // H of a power-of-two shard count: elements first + k·stride, k < len() (lo = 0, hi = len)
  uint32_t len() const { return hi - lo; }
};

// Deferred build of a key's fixed-base tables (cache.cpp).  The tables cost 0.26 s at 1.6 M constraints and buy 2–3 ms per
// prove: a key is therefore usable — in the classic layout, bases converted in place — as soon as its sections are on the
// device, and a worker thread builds the five tables on a low-priority stream behind (and beside) the first proofs.  The prove
// that finds them complete swaps pointers and geometry in, all five at once (adopt_tables; the caller holds the manager's mutex).
constexpr int TABLE_BUILD_GRACE_MS = 150;
struct TableBuild {
  std::thread th;
  std::atomic<int> state{0}; // 0 nothing pending, 1 building, 2 complete (fresh[] valid, not adopted yet), 3 failed / cancelled
  std::atomic<bool> cancel{false};
  std::atomic<bool> go{false}; // set at the end of the key's first prove: the build starts behind it, not beside it (or after TABLE_BUILD_GRACE_MS without one)
  std::atomic<bool> hold{false}; // cold pipeline: the base arrays are still being uploaded — nothing may read them before cold_prove clears this (neither `go` nor the grace time counts)
  void* fresh[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // A, B1, B2, C, H
  MsmGeom gw, gh;            // the table geometries the build works towards
  int dense_c = 0;           // digit width of the dense witness geometry (gw may be narrower: the first prove's witness was light)
  uint64_t pending_bytes = 0; // table bytes already counted in the entry's device_bytes while the first build is under way
  // A first build that takes a NARROWER witness digit than the dense one pending_bytes was sized for (more table rows) asks here:
  // `narrow_room` = bytes beyond pending_bytes it may take (set by whoever admitted the key: what the cache budget has left, or no
  // limit), `extra_bytes` = what it took (counted by evict_for_budget until adopt_tables has corrected device_bytes)
  std::atomic<uint64_t> narrow_room{0};
  std::atomic<uint64_t> extra_bytes{0};
  bool witness_only = false; // a re-build of the four witness tables with another digit width (the key follows its witnesses): H stays
  double build_ms = 0;       // wall clock of the build (beside whatever proves ran meanwhile)
};

// (ColdFeed: prover/cold_feed.h)
struct ZKeyCache {
  // header — src/zkey.rs:6-21
  uint32_t n8q = 0, n8r = 0, n_vars = 0, n_public = 0, domain_size = 0, n_coef = 0;
  fe q, r;
  G1::P vk_alpha_1, vk_beta_1, vk_delta_1; // standard form projective (host)
  G2::P vk_beta_2, vk_gamma_2, vk_delta_2;
  // device
  int device_id = 0, shard_rank = 0, shard_count = 1;
  bool in_group = false; // a shard of an in-process device group (multi.cpp), as opposed to the one shard of a rank-per-GPU process
  MsmGeom geom_w, geom_h; // window geometry of the witness MSMs (A, B1, B2, C) and of the H MSM; geom_w follows the witnesses (cache.cpp)
  int geom_w_default_c = 0;        // digit width of the dense geometry chosen at cache build
  uint32_t* h_stats = nullptr;     // pinned: offset and count of the last bucket of the witness sort = its entry count
  uint64_t witness_entries = 0;    // non-zero digits of the witness range in the most recent prove
  uint32_t proves_since_rebuild = 0;
  uint32_t* d_rowptr = nullptr; // 2n+1
  uint32_t* d_cols = nullptr;   // n_coef
  fe* d_vals = nullptr;         // n_coef, Montgomery form
  Shard A, B1, B2, C, H;
  fe* d_witness = nullptr; // n_vars
  uint8_t* d_wtnz = nullptr; // sections 2 … 4 of a packed witness on their way into d_witness (groth16_prove_packed): grown on demand
  size_t wtnz_cap = 0;
  fe* d_vec = nullptr;     // 3n
  fe* d_fold = nullptr;    // 3·n/G: folded rows of a strided H shard (qap_coset_fold3)
  // distributed front end (groth16_dist_stage1/2; strided H shards only): Y rows of stage 1, what exchange 1 delivers,
  // what stage 2 sends, the scale table n⁻¹·ω_n^{−r·k2} — 3·m elements each, m = n / shard_count; exchange 2 delivers into d_fold
  fe *d_dist_y = nullptr, *d_dist_recv1 = nullptr, *d_dist_send2 = nullptr, *d_tw1 = nullptr;
  // d_fold holds the Z rows of this rank for the witness now resident: the next commitments call WITHOUT a new witness skips
  // its own inverse transform + fold.  Set only by the caller's confirmation that exchange 2 has delivered
  // (groth16_dist_exchange_done, or the in-process group prove); cleared by every witness upload and every stage 1.
  bool dist_ready = false;
  bool dist_stage2_done = false; // stage 2 has run for the resident witness (what groth16_dist_exchange_done checks)
  fe* d_skeys = nullptr;   // n: n⁻¹·g^i — 1/n and the coset keys folded into the inverse transform's last pass (ntt_fuse.h); built on first use
  uint8_t* d_partials = nullptr; // 5 × PARTIALS_STRIDE: per-window partial sums of the five MSMs
  uint8_t* h_partials = nullptr; // pinned mirror
  hipStream_t s_g1 = nullptr, s_g2 = nullptr, s_g3 = nullptr, s_g4 = nullptr, s_g5 = nullptr, s_qap = nullptr;
  hipEvent_t ev_witness = nullptr, ev_sort = nullptr, ev_sort_h = nullptr, ev[4] = {nullptr, nullptr, nullptr, nullptr}, ev_done[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // head / tail of a witness on its way in (prover.cpp): head resident (pinned source), the head's four accumulations done;
  // with timing: end of the head's chain, end of the upload
  hipEvent_t ev_lfork[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, ev_ljoin[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; // large-bucket kernels on a side stream (msm_plan.h: LargeSide)
  hipEvent_t ev_head_in = nullptr, ev_head_done = nullptr, ev_t_head_start = nullptr, ev_t_head_end = nullptr, ev_t_witness = nullptr;
  int head_units = -1; // upload chunks of the witness that are sorted and accumulated while the rest is still on its way (follows the measured upload, prover.cpp); −1: not chosen yet
  uint64_t device_bytes = 0;
  bool witness_resident = false; // d_witness holds the witness of the last call (wtns == NULL reuses it)
  bool witness_event_set = false; // ev_witness was already recorded for the resident witness (behind a device-side all-gather)
  // device group: this shard's own 1/count of the witness is in place (recorded behind its PCIe upload, before the all-gather);
  // with slice_aligned — the shard's point range IS that slice — its witness sort and accumulations wait for nothing else
  hipEvent_t ev_own_slice = nullptr;
  bool own_slice_event_set = false, slice_aligned = false;
  Groth16Timings last_tm = {0, 0, 0, 0}; // phase timings of the most recent prove (groth16_last_timings)
  MsmProfile prof[6] = {};               // A, B1, B2, C, H of the most recent prove + [5] the digit sort of the witness HEAD (ev[0] → ev[4]; L = 0 without one): this entry's own slots (the shards of a group may share a device)
  uint64_t last_use = 0;                 // CacheManager LRU clock
  TableBuild tb;                         // deferred fixed-base tables (single-device keys)
  ColdFeed* feed = nullptr;              // set for the ONE prove that runs while the key's sections are still arriving (cold pipeline)

  std::array<hipStream_t, 6> streams() const { return {s_qap, s_g1, s_g2, s_g3, s_g4, s_g5}; }
  ~ZKeyCache();
};

// digit width of the witness MSMs adapted to the witnesses seen (cache.cpp)
int witness_digit_target(const ZKeyCache* z, uint64_t entries);
int rebuild_witness_tables(ZKeyCache* z, int c_new);
// the same in the background (round 5): a worker builds the four tables beside the proves of the key, which go on with the tables
// they have, and a later prove adopts them (adopt_tables).  Returns at once; nothing happens when a build is already under way.
void start_witness_rebuild(ZKeyCache* z, int c_new);
// the policy that decides when either happens (cache.cpp); `sync`: re-build in this call instead of starting the worker
int follow_witness(ZKeyCache* z, bool sync);

// deferred tables: 1 = the key proves with its tables (or has none coming: classic layout for good), 0 = still building.
// `wait`: block until the build has ended.  Swaps complete tables in; the caller holds the manager's mutex (no prove in flight).
int adopt_tables(ZKeyCache* z, bool wait);

// CacheManager::compute — src/cache.rs:117-241, from a key that zkey_layout has read (a load, every shard of a device group and the
// cold prove parse once and hand the layout on).  A row of stages over one LoadCtx (cache.cpp): fill_header → open_streams →
// alloc_key_buffers (shard_ranges.h) → decide_layout → ingest (not when pipelined) → convert_bases → alloc_work_buffers →
// start_cold_upload / start_table_thread.  A PACKED key (L.packed set by zkez_layout; count = 1, cold = nullptr) runs ingest_packed in
// ingest's place: the packed sections go up into temporaries of the LoadCtx and the unpack kernels fill the buffers ingest fills.
// `defer_tables`: return once the key can prove in the classic layout and build
// the fixed-base tables on a worker thread (single-device keys; ICICLE_SNARK_DEFER_TABLES=0 builds them before returning)
// `cold` (single-device keys with deferred or no tables): return as soon as the buffers exist and an uploader task has been started —
// the sections, the CSR and the witness of `cold->wtns` arrive behind the stages of cold->feed; the caller waits for cold->task
// before it lets go of the zkey / witness memory.
struct ColdUpload {
  ColdFeed feed;
  HostTask task;                      // the uploader (a pooled worker; run inline when none can be had)
  // witness: standard-form values of the .wtns image the prove will run on
  const uint8_t* wtns_values = nullptr;
  size_t wtns_bytes = 0;
  // the two images when they are mapped files (staging workers pread() instead of copying out of the mapping); fd < 0: plain memory
  const void *zkey_base = nullptr, *wtns_base = nullptr;
  size_t zkey_len = 0, wtns_len = 0;
  int zkey_fd = -1, wtns_fd = -1;
  hipStream_t lanes[2] = {nullptr, nullptr};
  bool started = false;
};
void cold_upload_wait(ColdUpload* cu); // blocks until the uploader task has ended (no-op when it never started); returns its lanes to the pool
int build_cache(const ZkeyLayout& L, int device_id, int rank, int count, std::unique_ptr<ZKeyCache>& out, bool defer_tables = false, ColdUpload* cold = nullptr);
typedef CopyJob UploadJob;
int staged_upload(int device_id, const std::vector<UploadJob>& jobs, const hipStream_t* lanes_in = nullptr, int n_lanes = 0, StagedProgress* progress = nullptr);

// ---- lane tests' verdicts; packed points, packed coefficients and packed witnesses on a device (ptau_pack.hip, zkey_pack.hip,
// wtns_pack.hip; pack_device.h has what their kernels share)
// min over the faulty lanes of (element << 3 | kind) without a faulty lane; the text of a point's kind
constexpr unsigned long long NO_FAULT = ~0ull;
const char* const POINT_FAULT[4] = {"", "a coordinate is not below q", "the point is not on the curve", "the point is outside the subgroup"};
// What a pack / unpack launch leaves behind: min over the faulty lanes of (element << 3 | kind), NO_FAULT without one; their number.
struct PackTally {
  unsigned long long first, count;
};
// ONE launch, a lane per point, both buffers on the device, the faults into *d_tally (reset by the caller); nothing is synchronised.
// pack: n file-form points (64 bytes, g2: 128) → n packed words behind zkey_check29.h's lane test (g2: with the subgroup test);
// unpack: the reverse through point_pack29.h's full pk_unpack_g1 / pk_unpack_g2.  A faulty element leaves zeros.
int pack_on_device(hipStream_t st, const uint8_t* d_points, uint64_t n, bool g2, uint8_t* d_out, PackTally* d_tally);
int unpack_on_device(hipStream_t st, const uint8_t* d_words, uint64_t n, bool g2, uint8_t* d_out, PackTally* d_tally);
// one range of points on its way through the device, in either direction
struct PointRange {
  int section;
  bool g2;
  uint64_t n;
  const uint8_t* src; // host
  uint8_t* dst;       // host; set once the output's layout is known
  uint8_t *d_in, *d_out;
};
// every range with points: d_in and d_out from the session, src up (landed on return, its time added to *upload_ms), the ONE launch
// above on the session's stream 0 with d_tally[k] for range k (reset by the caller).  Nothing is synchronised.
int enqueue_point_ranges(vb::DeviceSession& ds, int dev, bool unpack, PointRange* ranges, size_t count, PackTally* d_tally, double* upload_ms);
// Packed coefficients (a ZkezCoefs that zkez_coefs_layout has passed) → n_coef file-form records of COEF_RECORD_BYTES at d_records:
// zkez_coefs_device_bytes is the room wanted at d_buf (a hipMalloc'd base), zkez_coefs_jobs appends the four uploads into it, and —
// once they have landed — zkez_coefs_decode zeroes the paddings and enqueues ONE launch on `st`, a 256-lane workgroup per block.
// Nothing is synchronised; *d_tally (reset by the caller) holds (coefficient << 3 | GROTH16_WTNZ_*).  A faulty lane writes a zero record.
size_t zkez_coefs_device_bytes(const ZkezCoefs& C);
void zkez_coefs_jobs(const ZkezCoefs& C, uint8_t* d_buf, std::vector<UploadJob>& jobs);
int zkez_coefs_decode(hipStream_t st, const ZkezCoefs& C, uint8_t* d_buf, uint32_t* d_records, PackTally* d_tally);
// ERR_FORMAT "<form>: section S, element E: <point kind>" / "<form>: coefficient E: <wtnz kind>" for a tally that holds a fault
int packed_point_fail(const char* form, int section, const PackTally& t);
int packed_coef_fail(const char* form, const PackTally& t);
// ERR_FORMAT "ptau: section S, element E: <point kind>": a faulty point of a .ptau, whichever tool met it
inline int ptau_point_fail(int section, uint64_t element, int kind)
{
  return fail(ERR_FORMAT, "ptau: section %d, element %llu: %s", section, (unsigned long long)element, POINT_FAULT[kind & 3]);
}
// where a faulty point lies, into whichever report it is: the reports share these names (fault_count is set where a report has it)
template <class Report>
void set_point_fault(Report* rep, int section, uint64_t element, int kind)
{
  rep->fault_section = section, rep->fault_index = element, rep->fault_kind = kind;
}

// ---- blinding and proof assembly (assemble.cpp)
// blinding terms that do not depend on the commitments: δ1·r, δ1·s, δ2·s, δ1·r·s (src/proof_helper.rs:280-283);
// groth16_prove_mem computes them on a host thread while the GPU works
struct Blinding {
  bn254_scalar_t r, s;
  bn254_projective_t d1r, d1s, d1rs;
  bn254_g2_projective_t d2s;
};
// The two scalar multiplications of the proof's C term that need a commitment — (A + α1 + δ1·r)·s and
// (B1 + β1 + δ1·s)·r, src/proof_helper.rs:284-287 — only need A and B1, which are complete milliseconds before H:
// the host threads that finish those two MSMs go on to compute them while the GPU still works (single-GPU prove only;
// a sharded prove has to sum the commitments of all ranks first).
struct EarlyTerms {
  const Blinding* bl = nullptr;
  std::atomic<bool> bl_ready{false};
  bn254_projective_t ta, tb;
  std::atomic<int> done{0};
  // pi_a and pi_b complete (blinded, affine, as the decimal strings of proof.json) as soon as A's and B2's tails have run —
  // milliseconds before H's: only pi_c is left for assemble_impl after the last kernel
  std::string a_dec[2], b_dec[4];
  std::atomic<bool> a_ready{false}, b_ready{false};
};
// pi_a = A + α1 + δ1·r / pi_b = B2 + β2 + δ2·s → affine → decimal strings (assemble.cpp)
void early_pi_a(const ZKeyCache* z, const Blinding& bl, const bn254_projective_t* a_plus_alpha_d1r, EarlyTerms* et);
void early_pi_b(const ZKeyCache* z, const Blinding& bl, const bn254_g2_projective_t* b2_sum, EarlyTerms* et);
int compute_blinding(const ZKeyCache* z, const uint8_t* r_in, const uint8_t* s_in, Blinding* b);
int assemble_impl(const ZKeyCache* z, const void* wtns, size_t wtns_len, const uint8_t* points, const Blinding& bl, char* proof_json, size_t proof_cap, char* public_json, size_t public_cap,
                  const EarlyTerms* et = nullptr);
// the same from the witness's first n_public + 1 values (32 bytes each, standard form) instead of a .wtns image
int assemble_values(const ZKeyCache* z, const uint8_t* values, const uint8_t* points, const Blinding& bl, char* proof_json, size_t proof_cap, char* public_json, size_t public_cap,
                    const EarlyTerms* et = nullptr);

// ---- one device (prover.cpp)
struct DeviceGroup; // multi.cpp

// ---- an .r1cs resident on one device (r1cs_check.hip), as groth16_zkey_verify_ptau (zkey_verify.hip) uses it
struct R1csShape {
  int dev;
  uint32_t n_wires, n_public, m;
};
} // namespace prover
} // namespace isnark
struct Groth16R1cs;
namespace isnark {
namespace prover {
R1csShape r1cs_shape(const Groth16R1cs* h);
std::mutex& r1cs_mutex(Groth16R1cs* h); // a handle serves one call at a time
// a_j = A_j·v, b_j = B_j·v, c_j = C_j·v for j < m to abc[j], abc[m + j], abc[2m + j] (standard form): the witness check's kernel
// with v (n_wires canonical standard-form values on the handle's device) in the witness's place; enqueued on `stream`
int r1cs_emit_abc(Groth16R1cs* h, const fe* d_v, fe* d_abc, hipStream_t stream);
// the handle's rows as groth16_zkey_new (zkey_new.hip) transposes them: rowptr[3m + 1] in terms (rows A_0 B_0 C_0 A_1 …), the wire
// and the Montgomery coefficient of each term.  Read-only, on the handle's device, valid while the caller holds r1cs_mutex.
struct R1csDeviceRows {
  const uint32_t *d_rowptr, *d_cols;
  const fe* d_vals;
  uint64_t n_terms;
};
R1csDeviceRows r1cs_device_rows(const Groth16R1cs* h);
} // namespace prover
} // namespace isnark

// The reference's CacheManager (src/cache.rs:110-115) maps "{zkey_path}_{device}" to a ZKeyCache.  Here an entry is either
// ONE device's cache or a GROUP of shard caches (one per device of a "HIP:a-b" device string) that prove together.
struct Groth16CacheManager {
  std::mutex mu;     // serialises cache builds and proves (one device pipeline per manager)
  std::mutex map_mu; // guards `cache` / `groups`; entries are shared_ptr so that an evict cannot free a key a prove still uses
  std::map<std::string, std::shared_ptr<isnark::prover::ZKeyCache>> cache;
  std::map<std::string, std::shared_ptr<isnark::prover::DeviceGroup>> groups;
  std::map<int, uint32_t> domain_n; // device → domain_size its NTT domain was last initialised for (get_cache, src/cache.rs:242-256)
  uint64_t clock = 0;               // LRU clock (last_use of the entries)
  uint64_t budget_bytes = 0;        // device-memory budget per device for cached keys (0 = none): least recently used keys are evicted
  std::thread warm;                 // prewarm_device on the device the manager was created for (joined by the first cache load and by free)
  ~Groth16CacheManager()
  {
    if (warm.joinable()) warm.join();
  }
};

namespace isnark {
namespace prover {
std::shared_ptr<ZKeyCache> find(Groth16CacheManager* cm, const char* key);
std::shared_ptr<DeviceGroup> find_group(Groth16CacheManager* cm, const char* key);
int set_active_device(int device_id);
int ensure_domain(Groth16CacheManager* cm, const ZKeyCache* z); // works on the calling thread's active device (= z->device_id)
int ensure_domain_for(Groth16CacheManager* cm, int device_id, uint32_t domain_size);
void evict_for_budget(Groth16CacheManager* cm, int device, uint64_t need);
uint64_t budget_room(Groth16CacheManager* cm, int device);
// the shard pipeline of one device; caller holds cm->mu.  wtns == NULL: the witness (and, with z->dist_ready, the Z rows) are resident
int shard_commitments(Groth16CacheManager* cm, ZKeyCache* z, const void* wtns, size_t wtns_len, uint8_t* out_points, Groth16Timings* tm, EarlyTerms* et);
// distributed front end, stages without the host synchronisation of the C API (the exchange is enqueued on z->s_qap)
int shard_upload_slice(ZKeyCache* z, const Wtns& w);
int shard_dist_stage1(Groth16CacheManager* cm, ZKeyCache* z);
int shard_dist_stage2(ZKeyCache* z);
bool shard_dist_supported(const ZKeyCache* z);

// ---- device groups (multi.cpp)
// "HIP", "HIP:3", "HIP:0-7", "HIP:0,2,5", "CUDA:0-3" (alias) → device ids (duplicates allowed: several shards on one device);
// a plain "HIP" / "CUDA" takes ICICLE_SNARK_DEVICES=<list> when set.  Returns 0 or an error code (text in last_error_text).
int parse_device_string(const char* device, std::vector<int>& ids);
int group_load(Groth16CacheManager* cm, const char* key, const uint8_t* zkey, size_t len, const std::vector<int>& devs);
int group_commitments(Groth16CacheManager* cm, DeviceGroup* g, const void* wtns, size_t wtns_len, uint8_t* out_points, Groth16Timings* tm);
const ZKeyCache* group_lead(const DeviceGroup* g);
void group_info(const DeviceGroup* g, Groth16CircuitInfo* info);
std::string group_describe(const DeviceGroup* g); // one line of JSON: shards, devices, transport, RCCL ranks (groth16_group_describe)
} // namespace prover
} // namespace isnark
