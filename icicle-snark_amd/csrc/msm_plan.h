// msm_plan.h — shared declarations of the MSM pipeline stages (sort plan, profile ring).
//
// The pipeline is split so that a caller holding several base sets for ONE scalar vector (Groth16:
// A, B1, B2 and C are all multiplied by the witness, src/proof_helper.rs:198-206) sorts the scalars'
// digits once and runs only the bucket stages per base set.
#pragma once
#include "common.h"
#include "ff.h"

namespace isnark {

constexpr uint32_t MSM_LARGE_CHUNK = 1024; // entries per work item of a large bucket (256 threads × 4 additions, then an 8-level tree; 4096 made the G2 chain 3× longer)

struct MsmGeom {
  int c, W;      // digit width and digits per scalar
  uint32_t NB;   // 2^(c-1): magnitudes of a signed digit (= buckets per window in the classic layout)
  uint32_t H[9]; // Σ_w 2^(c·w + c − 1)
  // Fixed-base TABLE mode (the prover's cached keys): the bases are stored as W rows 2^(c·w)·P_i, every digit of
  // every window then lands in ONE bucket set of NB buckets (bucket = |digit| − 1) and no Horner pass over windows
  // is left.  The number of mixed additions is still one per non-zero digit, but with a single bucket set the digit
  // can be 4 bits wider for the same number of buckets: 13 instead of 16 digits per 254-bit scalar (−19 % additions)
  // at the price of W× the base memory — 8 GB of the 288 GB at 1.6 M constraints.
  // Table mode narrows the TOP windows by one bit so that the W windows cover exactly 254 bits (c = 20: seven 20-bit and six
  // 19-bit windows instead of twelve full ones and a 14-bit top digit, whose 2^21 entries all fell into 12 K buckets — four times
  // the average load, the waves that defined the accumulation's length): windows w < wide are c bits wide at bit c·w, the others
  // c − 1 bits at c·wide + (c − 1)(w − wide).  Classic layout: only when the top digit would be 1–3 bits short (msm_geometry); its Horner tails double c or c − 1 times.
  int wide;
  int tab;       // 0 classic (bucket = w·NB + |d| − 1, entry = point index), 1 table mode (bucket = |d| − 1, entry = i | w << IB)
  int IB;        // table mode: bits of the point index inside an entry
  int Wb;        // bucket array viewed as Wb pseudo-windows of NBb buckets (classic: nbms × NB) for the reduction kernel
  uint32_t NBb;
  // Classic layout with precomputed bases (MSMConfig.precompute_factor = pf > 1, icicle/include/icicle/msm.h:23-27): the
  // caller's base array holds pf points per base, [pf·i + j] = 2^(j·c·nbms)·P_i (msm_precompute_bases), so window w adds
  // point j = w / nbms into the bucket set of window w mod nbms: nbms = ⌈W / pf⌉ bucket sets to reduce and a Horner tail
  // of nbms windows instead of W.  pf = 1: nbms = W.
  int pf, nbms;
};

// Result of the recode + counting-sort stage for one scalar vector (device arrays, workspace arena).
constexpr int MSM_TICKET_SLOTS = 8;
struct SortPlan {
  MsmGeom g;
  uint32_t L = 0, nbuckets = 0, large_thr = 0;
  uint32_t* ws = nullptr;      // base of the u32 workspace below
  uint32_t* counts = nullptr;  // [nbuckets] entries per bucket (bucket = w·NB + |digit| − 1)
  uint32_t* offsets = nullptr; // [nbuckets] exclusive prefix sum
  uint32_t* n_large = nullptr; // [0] number of large buckets, [1] total entries, [2] number of large work items
  uint32_t* tickets = nullptr; // [MSM_TICKET_SLOTS][64] zeroed by the sort: one counter per window for each bucket-stage run that uses this plan
  uint32_t* large_list = nullptr; // [nbuckets] ids of buckets with more than large_thr entries
  uint32_t* large_first = nullptr; // [nbuckets] first work item of each large bucket
  uint2* large_items = nullptr;   // [item_cap] (bucket, chunk) work items: a large bucket is cut into MSM_LARGE_CHUNK-entry chunks
  uint32_t item_cap = 0;
  uint32_t* order = nullptr;   // [nbuckets] bucket ids by decreasing entry count (wave-uniform trip counts)
  uint32_t* sorted = nullptr;  // [L·W] (index within the scalar vector) | sign << 31, grouped by bucket
  hipStream_t stream = nullptr;
  SortPlan() = default;
  SortPlan(const SortPlan&) = delete;
  SortPlan& operator=(const SortPlan&) = delete;
  ~SortPlan(); // = msm_sort_release(this): the workspace goes back to the arena on every path
};

// geometry for a length-L MSM (c_cfg > 0 forces the window size); tab != 0 asks for the table mode (falls back to
// the classic layout when the entry encoding would not fit; tab > 1 asks for the table mode with digits of `tab` bits)
// `bits` (MSMConfig.bitsize, msm.h:32-34): every scalar is < 2^bits — W = ⌊bits / c⌋ + 1 windows instead of ⌊254 / c⌋ + 1
// (0 = the scalar field's 254); `pf`: precompute factor of the base array (classic layout only).
MsmGeom msm_geometry(uint32_t L, int c_cfg, int tab = 0, int bits = 0, int pf = 1);
// recode → histogram → scan → scatter on stream s.  Workspace comes from the arena of stream s and is
// returned by msm_sort_release (which only marks it reusable by later work on that stream; idempotent, also
// run by ~SortPlan).
// `entries_hint` > 0: the number of non-zero digits the caller expects (a witness-light key adapted to its witnesses, prover.cpp):
// the large-bucket threshold is then 3 × that average instead of 3 × the dense one.
// `crowded`: the sort will run beside kernels that keep every SIMD's wave slots and registers nearly full (the bucket accumulations):
// its big kernels then use 256-thread workgroups, which find room where 512-thread ones wait for milliseconds (msm_sort.hip).
eIcicleError msm_sort_run(const bn254::fe* d_scalars, uint32_t L, int c_cfg, int large_bucket_factor, int scalars_mont, hipStream_t s, SortPlan* pl, int tab = 0, int bits = 0, int pf = 1,
                          uint64_t entries_hint = 0, bool crowded = false);
void msm_sort_release(SortPlan* pl);

// ring of the most recent MSM launches of this process: HIP events (recorded on the MSM's own stream,
// never synchronised here) + geometry, read back by icicle_snark_msm_profile() after the caller synced.
struct MsmProfile {
  hipEvent_t ev[5]; // start (sort), before accumulate, after accumulate, end, end of the sort (same stream as ev[0])
  bool has_sort_end;
  uint32_t L, nbuckets;
  int c, W, is_g2;
  bool valid;
  bool resolved; // ms[] holds the elapsed times already (a published copy: its events belong to somebody else)
  float ms[5];
};
constexpr int MSM_PROFILE_RING = 32;
MsmProfile* msm_profile_next();
// A caller with profile slots of its own (the prover: five per cached key, so that the shards of a device group that share a
// device do not recycle each other's slots mid-prove) publishes them, resolved to times, once its streams are synchronised.
void msm_profile_own_init(MsmProfile* p);    // creates the events on the active device (idempotent)
void msm_profile_own_destroy(MsmProfile* p);
void msm_profile_publish(const MsmProfile* p, int n);

// Bucket stages for one base set on stream s (may differ from the plan's stream; the caller orders them):
// accumulate (+ large buckets) → reduction.  Writes XYZZ partial sums (Montgomery form) to d_partials (device,
// caller-provided, ≥ msm_partials_bytes(): classic layout one sum per window; table mode the plain sum T and the t bit-plane
// sums S_j of the single bucket set; `d_points` is then the table with `points_form` = 2, rows of `row_len` points).  Entries whose scalar index is < skip_below
// are ignored and the base index is (scalar index − skip_below): lets the C MSM (witness[n_public+1..])
// share the witness sort.
// `points_form` below: 0 standard form, 1 Montgomery R = 2^256 (as stored in zkey files), 2 the internal encoding of the
// bucket kernels (packed canonical Montgomery R' = 2^261, ff29.h).  msm_*_points_to_internal converts a base array
// in place (once per key; the identity (0,0) is preserved) so that the hot loop loads points without a conversion.
eIcicleError msm_g1_points_to_internal(void* d_points, uint32_t n, int from_form, hipStream_t s);
eIcicleError msm_g2_points_to_internal(void* d_points, uint32_t n, int from_form, hipStream_t s);
// table mode (MsmGeom.tab): d_table = W rows of n points, row w = 2^(c·w)·P in the internal encoding (hipMalloc'ed,
// owned by the caller); `g` = msm_geometry(n_scalars, 0, 1) of the scalar vector the table will be used with.
eIcicleError msm_g1_build_table(const void* d_points, uint32_t n, int from_form, const MsmGeom& g, hipStream_t s, void** d_table);
eIcicleError msm_g2_build_table(const void* d_points, uint32_t n, int from_form, const MsmGeom& g, hipStream_t s, void** d_table);
// The same table built in slices of the base array (temporaries of a slice's size, no launch larger than the device holds at a
// time, `cancel` polled between slices): the deferred build of a cached key's tables on a low-priority stream beside the
// proves that already use the key (prover/cache.cpp).  Returns with stream s synchronised.
// bases per slice of the sliced build (ICICLE_SNARK_TABLE_SLICE_LOG overrides the default of 2^18 for G2, twice that for G1)
inline uint32_t table_slice_bases()
{
  static const int lg = env_int("ICICLE_SNARK_TABLE_SLICE_LOG", 18);
  return 1u << (lg < 12 ? 12 : lg > 22 ? 22 : lg);
}
eIcicleError msm_g1_build_table_sliced(const void* d_points, uint32_t n, int from_form, const MsmGeom& g, hipStream_t s, void** d_table, const std::atomic<bool>* cancel);
eIcicleError msm_g2_build_table_sliced(const void* d_points, uint32_t n, int from_form, const MsmGeom& g, hipStream_t s, void** d_table, const std::atomic<bool>* cancel);
// table mode: h_partials = [T | S_0 … S_{nbits−1}] (msm_partials_bytes gives nbits as *W)
void msm_g1_host_tail_tab(const void* h_partials, uint32_t nbits, bn254_projective_t* out);
void msm_g2_host_tail_tab(const void* h_partials, uint32_t nbits, bn254_g2_projective_t* out);
// The large-bucket kernels of a bucket stage on a SIDE stream, beside the accumulation instead of behind it (they write disjoint
// buckets): for uniform scalars their work lists are empty, but their 1024 + 256 workgroups still have to be dispatched one by one
// onto a GPU the accumulations keep full — 0.3–1.8 ms in which the MSM's chain did nothing (prover.cpp).  `fork` / `join`: events of
// the caller (disable-timing), recorded on s / on the side stream; the reduction behind the stage waits for `join`.
struct LargeSide {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
size_t msm_partials_bytes(const SortPlan* pl, bool g2, uint32_t* W, uint32_t* M);
// `ticket_slot` < MSM_TICKET_SLOTS: every run of the bucket stages on one plan needs its own (the runs may overlap in time)
eIcicleError msm_g1_partials(const SortPlan* pl, const void* d_points, int points_form, uint32_t skip_below, hipStream_t s, void* d_partials, MsmProfile* prof, uint32_t row_len = 1, int ticket_slot = 0, const LargeSide* side = nullptr);
eIcicleError msm_g2_partials(const SortPlan* pl, const void* d_points, int points_form, uint32_t skip_below, hipStream_t s, void* d_partials, MsmProfile* prof, uint32_t row_len = 1, int ticket_slot = 0);
// The two bucket stages separately, over a bucket array the caller owns (msm_bucket_bytes; workspace of ITS choice), so that
// several SEGMENTS of one scalar vector — each with its own sort plan of the same geometry — can be accumulated one after the
// other (`into` = continue the sums already in the array) before ONE reduction: the prover sorts and accumulates the head of a
// witness while its tail is still crossing PCIe (prover.cpp).  With segments, `d_points` and `skip_below` are the caller's to
// offset: entries index scalars relative to the segment's first element.
size_t msm_bucket_bytes(const SortPlan* pl, bool g2);
// `resident`: the accumulation kernel is launched with no more workgroups than the device holds at a time and strides over
// the buckets — its dispatch then never sits in a hardware pipe's way (see msm_accumulate_kernel).
eIcicleError msm_g1_accumulate(const SortPlan* pl, const void* d_points, int points_form, uint32_t skip_below, hipStream_t s, void* d_buckets, bool into, MsmProfile* prof, uint32_t row_len = 1, bool resident = false, const LargeSide* side = nullptr);
eIcicleError msm_g2_accumulate(const SortPlan* pl, const void* d_points, int points_form, uint32_t skip_below, hipStream_t s, void* d_buckets, bool into, MsmProfile* prof, uint32_t row_len = 1, bool resident = false, const LargeSide* side = nullptr);
eIcicleError msm_g1_reduce(const SortPlan* pl, hipStream_t s, const void* d_buckets, void* d_partials, int ticket_slot = 0);
eIcicleError msm_g2_reduce(const SortPlan* pl, hipStream_t s, const void* d_buckets, void* d_partials, int ticket_slot = 0);
// host-side tail: window sums (Σ of bpw partials) → Horner with c doublings → standard-form projective
void msm_g1_host_tail(const void* h_partials, uint32_t W, uint32_t bpw, int c, int wide, bn254_projective_t* out);
void msm_g2_host_tail(const void* h_partials, uint32_t W, uint32_t bpw, int c, int wide, bn254_g2_projective_t* out);

// G2 bucket accumulation, compiled with inlined Fq2 arithmetic (msm_g2_acc.hip)
void msm_g2_accumulate_launch(const SortPlan* pl, const void* d_points, int points_mont, uint32_t skip_below, uint32_t stride, hipStream_t s, void* buckets, int into, bool resident);

// ---- automatic fixed-base tables behind bn254_msm / bn254_g2_msm (runtime.cpp) -------------------------------------------------
// A caller that runs MSM after MSM over the SAME device-resident base array (the reference's host keeps its zkey points on the
// device, src/cache.rs:58-72) gets the prover's table mode without asking: the second MSM over (pointer, length, form) builds the
// table — W rows 2^(c·w)·P_i in the internal encoding — on the caller's stream, later ones use it (13 instead of 16 digits per
// scalar at 1.6 M points, one bucket set, no Horner pass).
// The reference reads the bases at call time (icicle/src/msm.cpp:12-32), so a table is only ever used for the bases' CURRENT
// contents, however the caller wrote them (round-3 verdict: write tracking of this library's own entry points alone is not that):
//   * every call that hits a table first sums a 64-bit position-dependent hash of the whole base array on the caller's stream
//     (one pass over L·64 / L·128 bytes: ≈ 30–60 µs at 1.6 M points) next to the sum stored when the table was built;
//   * a guarded refresh kernel follows in the same stream: it returns at once when the two sums agree and otherwise recomputes
//     every row of the table from the bases in place (slow — one inversion per row and base — but rare), after which the stored
//     sum is replaced.  No host synchronisation, no second pipeline: the MSM kernels behind it always see a table of the bases
//     as they are at that point of the stream;
//   * entry points of this library that write device memory still retire the tables they touch (note_device_write): that only
//     saves the refresh its work.
// A table in use by a call that is still enqueueing is pinned (base_table_unpin) — a concurrent retire parks it until then.
// ICICLE_SNARK_MSM_TABLES=0 switches the feature off, ICICLE_SNARK_MSM_TABLE_MB (default 16384) bounds the tables per device
// (least recently used first).
struct BaseTableRef {
  const void* table = nullptr;
  MsmGeom g;
  hipEvent_t built = nullptr;        // recorded behind the build on the building stream
  unsigned long long* sums = nullptr; // device: [0] hash sum of the bases the table was built from
  uint64_t id = 0;                    // pin to release with base_table_unpin once the call's kernels are enqueued (0: none)
  hipEvent_t used = nullptr;          // behind the last kernel of the previous call that used the table (any stream); nullptr: none yet
};
enum BaseTableState { BASE_TABLE_NONE = 0, BASE_TABLE_BUILD = 1, BASE_TABLE_HIT = 2 };
// NONE: run the classic layout (first sighting, not eligible, no memory); BUILD: the caller builds a table of geometry ref->g and
// hands it to base_table_publish (which pins it: ref->id); HIT: *ref is valid and pinned
BaseTableState base_table_lookup(const void* bases, size_t bytes, uint32_t n, bool g2, int form, size_t table_bytes, BaseTableRef* ref);
void base_table_publish(const void* bases, uint32_t n, bool g2, int form, void* table, size_t table_bytes, const MsmGeom& g, unsigned long long* sums, hipStream_t s, BaseTableRef* ref);
void base_table_unpin(uint64_t id, hipStream_t s); // s: the stream the call's kernels went to (its last-use mark is recorded there)

// exclusive prefix sum of m 32-bit counters on stream s (msm_sort.hip's three scan kernels); bsum: ≥ exclusive_scan_u32_scratch_words(m) words
hipError_t exclusive_scan_u32(const uint32_t* in, uint32_t m, uint32_t* out, uint32_t* bsum, hipStream_t s);
size_t exclusive_scan_u32_scratch_words(uint32_t m);

bool ext_get_int(const ConfigExtension* ext, const char* key, int* out);
bool ext_get_bool(const ConfigExtension* ext, const char* key, bool* out);

} // namespace isnark
