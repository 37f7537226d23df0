/*
 * groth16_prover.h — C API of the prover host that ships inside libicicle_snark_hip.so.
 *
 * The reference's host is Rust (src/lib.rs, src/proof_helper.rs, src/cache.rs); no Rust toolchain
 * exists in this build environment, so the same host logic is provided in C++ behind this C API,
 * with the reference's names and argument meaning:
 *
 *   groth16_prove(witness, zkey, proof, public, device, &mut CacheManager)   — src/lib.rs:33-61
 *   CacheManager::{compute, get_cache, insert_cache, contains}                — src/cache.rs:110-262
 *
 * File formats are snarkjs `.zkey` / `.wtns` in, `proof.json` / `public.json` out
 * (src/file_wrapper.rs:45-113, src/zkey.rs:47-85, src/conversions.rs:30-56).
 * All functions return 0 on success, an eIcicleError code (> 0) for device errors and a negative
 * value for I/O / format errors; groth16_last_error() gives the text.  Nothing unwinds across the ABI.
 */
#ifndef GROTH16_PROVER_H
#define GROTH16_PROVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct Groth16CacheManager Groth16CacheManager;

/* CacheManager::default() / drop — src/cache.rs:110-115 */
Groth16CacheManager* groth16_cache_manager_new(void);
void groth16_cache_manager_free(Groth16CacheManager* cm);
/* Optional: create on `device_id`, on a helper thread, what the first cache load of a process would otherwise pay for inside
 * its first prove (six streams with their DMA queues: 48 ms measured, the pinned staging pool).  groth16_cache_manager_new
 * does this by itself when a device has been made current before it (icicle_set_device); the REPL calls it at start-up.
 * ICICLE_SNARK_PREWARM=0 switches it off. */
void groth16_cache_manager_prewarm(Groth16CacheManager* cm, int device_id);

/* groth16_prove — src/lib.rs:33-61.  `device` is the reference's free-form device string (the reference passes the type
 * and always uses id 0, src/lib.rs:25-31); this library registers "HIP" (and the alias "CUDA"); anything else, including
 * "CPU", is an error — there is no CPU fallback.  The string may name the devices to prove on:
 *     "HIP"  (device 0, or the list in ICICLE_SNARK_DEVICES)   "HIP:2"   "HIP:0-7"   "HIP:0,2,4,6"
 * More than one device = ONE prove sharded over a device group inside this process: point-range shards of
 * the A, B1, B2, C bases, residue-class shards of H, the QAP front end distributed, device-side exchanges over xGMI.  A
 * device may be named several times ("HIP:0,0,0,0": four shards on GPU 0 — how a 1-GPU machine exercises the path).
 * Blinding factors r, s are drawn at random (default build of the reference). */
int groth16_prove(const char* witness_path, const char* zkey_path, const char* proof_path, const char* public_path,
                  const char* device, Groth16CacheManager* cm);

/* ---- finer-grained entry points used by bench.py / tests (same pipeline, memory in / memory out) ---- */

/* Build (or find) the device-resident cache for a zkey image held in memory (CacheManager::compute,
 * src/cache.rs:117-241).  `key` plays the role of "{zkey_path}_{device}" (src/lib.rs:44).
 * shard_rank / shard_count: this process keeps only the points [rank·L/count, (rank+1)·L/count) of each of
 * the five MSM bases (multi-GPU point-range sharding); 0 / 1 for a single GPU. */
int groth16_cache_load(Groth16CacheManager* cm, const char* key, const void* zkey, size_t zkey_len, int device_id,
                       int shard_rank, int shard_count);
int groth16_cache_load_file(Groth16CacheManager* cm, const char* key, const char* zkey_path, int device_id,
                            int shard_rank, int shard_count);
/* A single-device key is usable as soon as its sections are on the device: the first proofs run the classic bucket layout
 * while a worker thread builds the key's fixed-base tables (13 instead of 16 digits per scalar; 0.26 s of GPU work at 1.6 M
 * constraints) on a low-priority stream, and the first prove that finds them complete adopts them.  Proofs are identical
 * either way.  Returns 1 when the key proves in its final layout, 0 while the build is under way, negative on error;
 * wait != 0 blocks until the build has ended.  ICICLE_SNARK_DEFER_TABLES=0 builds the tables inside groth16_cache_load. */
int groth16_cache_tables_ready(Groth16CacheManager* cm, const char* key, int wait);
/* The same key over a GROUP of devices (what groth16_prove builds for "HIP:a-b"): shard k of n_devices lives on
 * device_ids[k].  Every entry point that takes a key (groth16_commitments, groth16_prove_mem, groth16_prove_resident,
 * groth16_cache_info, groth16_last_timings, groth16_cache_evict) then works on the group: groth16_commitments returns the
 * SUM of the shards' commitments. */
int groth16_cache_load_devices(Groth16CacheManager* cm, const char* key, const void* zkey, size_t zkey_len, const int* device_ids,
                               int n_devices);
/* device string → ids ("HIP:0-7" → 0 … 7): returns how many devices it names (`ids` receives the first `cap`), or a
 * negative error code.  Needs no GPU. */
int groth16_parse_device(const char* device, int* ids, int cap);
/* Device-memory budget for the cached keys of ONE device (bytes; 0 = unlimited, the reference's behaviour — its
 * CacheManager never evicts, src/cache.rs:110-114).  Before a new key is built, the least recently used single-device
 * keys of that device are evicted until the new entry fits.  ICICLE_SNARK_CACHE_BUDGET_MB sets the initial value. */
void groth16_cache_set_budget(Groth16CacheManager* cm, uint64_t bytes_per_device);
int groth16_cache_contains(const Groth16CacheManager* cm, const char* key);
void groth16_cache_evict(Groth16CacheManager* cm, const char* key);

/* The five commitments of groth16_commitments (src/proof_helper.rs:172-241) for this process's shard,
 * as standard-form projective points in the order A (G1, 96 B), B1 (G1, 96 B), B2 (G2, 192 B),
 * C (G1, 96 B), H (G1, 96 B)  — 576 bytes.  Includes construct_r1cs (src/proof_helper.rs:31-170).
 * wtns == NULL re-uses the witness uploaded by the previous call for this key (inputs already resident in
 * HBM — what bench.py times); otherwise the witness is staged through pinned memory and uploaded first. */
#define GROTH16_COMMITMENTS_BYTES 576
typedef struct {
  double h2d_ms;       /* witness upload */
  double qap_ms;       /* construct_r1cs on the device (sparse mat-vec, 2 batched NTTs, pointwise) */
  double msm_ms;       /* the five MSMs (two streams) */
  double total_ms;     /* wall clock of the call */
} Groth16Timings;
int groth16_commitments(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len,
                        uint8_t out_points[GROTH16_COMMITMENTS_BYTES], Groth16Timings* timings /* may be NULL */);

/* Multi-GPU witness distribution.  Every rank of a sharded key needs the whole witness on its device (its MSM range, and
 * the rows of the QAP front end it evaluates read arbitrary wires).  Instead of shard_count full uploads over PCIe, rank r
 * uploads elements [r·slice, min(n_vars, (r+1)·slice)), slice = ⌈n_vars / shard_count⌉, to their place in its device
 * witness buffer; the caller completes the buffer with an IN-PLACE all-gather of `slice_bytes` bytes per rank over
 * `*d_witness` (world × slice_bytes bytes; RCCL over xGMI: icicle_snark_rccl_allgather_device) and then calls
 * groth16_witness_ready, after which groth16_commitments / groth16_dist_stage1 take wtns = NULL. */
int groth16_upload_witness_slice(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len, void** d_witness, uint64_t* slice_bytes);
int groth16_witness_ready(Groth16CacheManager* cm, const char* key);

/* Distributed QAP front end for 2, 4 or 8 shards (H sharded by residue class; HISTORY.md §5, tests/dist_qap_model.py):
 * instead of replicating the spmv and the inverse transform on every rank, each rank transforms 1/count of the rows and
 * two all-to-alls move the blocks.  Sequence per prove, on every rank:
 *     groth16_dist_stage1(wtns)  →  all-to-all(send, recv)  →  groth16_dist_stage2()  →  all-to-all(send, recv)
 *     →  groth16_dist_exchange_done()  →  groth16_commitments(wtns = NULL)
 *                                                  (finishes with the size-n/count forward transform and the five MSMs)
 * The buffers are device memory owned by the cache entry: 3 rows of row_bytes; the chunk a rank exchanges with `peer` for
 * row `q` sits at q·row_bytes + peer·chunk_bytes in BOTH the send and the receive buffer.  groth16_dist_supported tells
 * whether the entry can take this path (otherwise groth16_commitments alone does everything, replicated). */
int groth16_dist_supported(Groth16CacheManager* cm, const char* key);
int groth16_dist_stage1(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len, void** d_send,
                        void** d_recv, uint32_t* rows, uint64_t* row_bytes, uint64_t* chunk_bytes);
int groth16_dist_stage2(Groth16CacheManager* cm, const char* key, void** d_send, void** d_recv);
/* The caller confirms that the second all-to-all has DELIVERED into *d_recv of groth16_dist_stage2.  Only after this call
 * does groth16_commitments(wtns = NULL) finish from those rows; without it (an exchange that failed, a retry) the
 * commitments call recomputes the whole front end itself, replicated.  A new witness clears the confirmation. */
int groth16_dist_exchange_done(Groth16CacheManager* cm, const char* key);

/* Element-wise group sum of `count` commitment blocks (gathered from the shards): out = Σ_k blocks[k]. */
int groth16_sum_commitments(const uint8_t* blocks, int count, uint8_t out_points[GROTH16_COMMITMENTS_BYTES]);

/* Tail of groth16_prove_helper (src/proof_helper.rs:274-316): blinding with (r, s) — 32-byte little-endian
 * standard-form scalars; NULL draws them at random; r = s = 1 reproduces the `no-randomness` feature —
 * affine conversion and JSON rendering.  Outputs are NUL-terminated pretty-printed JSON texts identical
 * in layout to serde_json::to_writer_pretty.  Returns the needed size (incl. NUL) if a buffer is too small. */
int groth16_assemble_proof(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len,
                           const uint8_t points[GROTH16_COMMITMENTS_BYTES], const uint8_t* r, const uint8_t* s,
                           char* proof_json, size_t proof_cap, char* public_json, size_t public_cap);

/* One-GPU convenience: commitments + assemble. */
int groth16_prove_mem(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len, const uint8_t* r,
                      const uint8_t* s, char* proof_json, size_t proof_cap, char* public_json, size_t public_cap,
                      Groth16Timings* timings);

/* Same, but with wtns_resident != 0 the witness uploaded by an earlier call is re-used on the device (the bytes are
 * still needed for the public signals): "inputs already resident in HBM", what bench.py times. */
int groth16_prove_resident(Groth16CacheManager* cm, const char* key, const void* wtns, size_t wtns_len, int wtns_resident,
                           const uint8_t* r, const uint8_t* s, char* proof_json, size_t proof_cap, char* public_json,
                           size_t public_cap, Groth16Timings* timings);

/* sizes of the cached circuit */
typedef struct {
  uint32_t n_vars, n_public, domain_size, n_coef;
  uint64_t device_bytes;
  uint32_t b_bases;  /* bases the two B MSMs run over (= the wires of this shard; kept for layout compatibility) */
  uint32_t shards;   /* device group: number of shards (device_bytes and b_bases are sums over them); else 0 */
} Groth16CircuitInfo;
int groth16_cache_info(const Groth16CacheManager* cm, const char* key, Groth16CircuitInfo* info);
/* the same for a caller that passes sizeof(its Groth16CircuitInfo): fields beyond info_size are not written, so a binary
 * built against an older, shorter struct keeps working when the struct grows */
int groth16_cache_info_sized(const Groth16CacheManager* cm, const char* key, void* info, size_t info_size);

/* What the key runs on, as one line of JSON — for a device group {"shards": G, "devices": [...], "distinct_devices": k,
 * "transport": "pull" | "memcpy" | "rccl", "peer_access": bool, "rccl_ranks": n (0 unless the rccl transport moves the
 * exchanges), "distributed_front_end": bool, "transport_forced_by_env": bool}; a single-device key answers "shards": 0.
 * Returns 0, or the size needed (incl. NUL) when `cap` is too small.  bench.py prints it with every multi-GPU line. */
int groth16_group_describe(const Groth16CacheManager* cm, const char* key, char* out, size_t cap);

/* phase timings (HIP events) of the most recent prove of `key` through ANY entry point — groth16_prove returns none,
 * like the reference's; bench.py reads them here.  ICICLE_SNARK_QUIET=1 suppresses groth16_prove's "proof took: …" line
 * (src/lib.rs:58) for callers whose stdout is machine-read. */
int groth16_last_timings(Groth16CacheManager* cm, const char* key, Groth16Timings* timings);

const char* groth16_last_error(void);

/* groth16_verify — src/lib.rs:63-82 with groth16_verify_helper (src/proof_helper.rs:319-372) and the snarkjs
 * verification_key.json reader (src/cache.rs:74-108).  Checks e(−A,B)·e(IC₀+Σ pubᵢ·ICᵢ₊₁, γ₂)·e(C,δ₂)·e(α₁,β₂) = 1
 * with four host pairings.  groth16_verify (paths): 0 = accepted, 1 = "Verification failed" (the reference
 * asserts), negative = I/O or format error.  groth16_verify_json (texts): 1 = accepted, 0 = rejected, negative =
 * format error.  No device is needed. */
int groth16_verify(const char* proof_path, const char* public_path, const char* vk_path);
int groth16_verify_json(const char* proof_json, const char* public_json, const char* vk_json);
const char* groth16_verify_last_error(void);

/* groth16_verify_batch — verify n proofs against ONE verification key on one GPU.
 * verdicts[i] = exactly what groth16_verify_json(proof_jsons[i], public_jsons[i], vk_json) returns: 1 accepted,
 * 0 rejected, negative = that item's format error (same codes).  device: "HIP", "CUDA" or "HIP:k" (one device; a list
 * is an error).  Returns 0 when every item was judged, whatever the verdicts; < 0 for a malformed vk or a null argument
 * (text in groth16_verify_last_error()); > 0 (eIcicleError) for a bad device string or a device failure.  n = 0
 * succeeds and writes nothing.  The JSON texts are parsed on the host (≤ 16 threads); the pi_b subgroup test, the
 * public-input sum, the multi-Miller loop and the final exponentiation run on the device, one lane per proof. */
int groth16_verify_batch(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json,
                         const char* device, int32_t* verdicts);
/* host parse time (vk and items) and device time (HIP events, uploads to verdicts) of this thread's last batch, ms */
void groth16_verify_batch_last_timings(double* parse_ms, double* device_ms);

/* groth16_verify_batch_combined — the same batch decided by ONE randomised pairing equation when every proof is valid.
 * Arguments, return codes, error texts, the n = 0 behaviour and the meaning of verdicts[i] are groth16_verify_batch's; items the
 * parser refuses keep their negative code and take part in nothing.  For coefficients z_i derived from the seed, the remaining
 * ("live") items are checked together:
 *     Π_i e(−z_i·A_i, B_i) · e(Σ_i z_i·cpub_i, γ₂) · e(Σ_i z_i·C_i, δ₂) · e((Σ_i z_i)·α₁, β₂) = 1
 * after a subgroup test of every pi_b (an endomorphism test: one 63-bit multiplication).  If all of that holds, every live item
 * gets 1 and *path = 1.  On any subgroup failure or a failed equation *path = 0 and the live items go through
 * groth16_verify_batch's per-item device stage.  So the verdicts always equal groth16_verify_batch's, with one exception: an
 * invalid item is accepted with probability ≤ 2^-127 per call, over the seed.  A valid proof is never rejected.  *path is 1 too
 * when no item is live (nothing was left to decide); `path` may be NULL.
 * Coefficients: z_i = the first 16 bytes of SHA-256(seed ‖ LE64(i)) read as a little-endian integer (the low 128 bits of the
 * digest taken as a little-endian number); 0 is replaced by 1.  i is the index in the caller's arrays, so chunking and parse
 * errors do not shift them.  seed32 == NULL draws 32 bytes from the operating system (getrandom, else /dev/urandom); when
 * that fails the call returns −3 — it never falls back to a constant.
 * THE SEED MUST BE SECRET AND FRESH: whoever knows the seed before choosing the proofs can build invalid proofs whose errors
 * cancel in the equation, which voids the guarantee.  Pass a seed only for reproducible tests; use NULL otherwise.
 * groth16_verify_batch_last_timings afterwards: the parse time, and as device time the wall time from the end of the parse
 * to the verdicts (lanes, product, MSM, the host tail, and the fallback when it ran). */
int groth16_verify_batch_combined(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json,
                                  const char* device, const uint8_t* seed32 /* NULL = OS randomness */, int32_t* verdicts,
                                  int32_t* path /* may be NULL */);
/* out16[16·k …] = z_{first + k} (16 bytes, little endian) for k < count, as derived above.  Needs no GPU. */
void groth16_verify_combined_coefficients(const uint8_t seed32[32], uint64_t first, uint64_t count, uint8_t* out16);

/* A set of verification keys, prepared once and kept on one device, for groth16_verify_batch_mixed.
 * groth16_vkset_new: every key goes through the key checks of groth16_verify_json (the host subgroup tests included), on the
 * library's worker threads.  A refused key gives −2 with the text "key <index>: <the key's error>" for the lowest such index; a
 * null argument (vk_jsons, one of its entries, device, out) gives −3.  Both are decided BEFORE any device is touched.  device:
 * "HIP", "CUDA" or "HIP:k" — one device, to which the set is bound; > 0 (eIcicleError) for a bad device string or a device failure.
 * On the device the set keeps, in standard form with (0, 0) the identity: every key's IC (concatenated) and α₁, and β₂, γ₂, δ₂ as
 * affine points.  n_keys = 0 is accepted.  A mutex in the set serialises the calls made on it; groth16_vkset_free releases
 * everything (the set must not be used afterwards).
 * groth16_vkset_info: key = −1 returns the number of keys; otherwise 0 with *n_public = that key's nPublic, −3 for a null set or a
 * key index outside the set. */
typedef struct Groth16VkSet Groth16VkSet;
int groth16_vkset_new(const char* const* vk_jsons, int n_keys, const char* device, Groth16VkSet** out);
int groth16_vkset_info(const Groth16VkSet* set, int key, uint32_t* n_public);   /* key = -1: returns n_keys */
void groth16_vkset_free(Groth16VkSet* set);

/* groth16_verify_batch_mixed — n proofs of MANY keys, interleaved, in one call: item i is a proof under key key_of[i] of the set.
 * verdicts[i] = what groth16_verify_batch returns for item i under that key (1 accepted, 0 rejected, negative = the item's format
 * error), with the one exception of the combined call: an invalid item is accepted with probability ≤ 2^-127.  An item whose
 * key_of is outside the set gets −2 (text in groth16_verify_last_error()) and disturbs nothing else.  n = 0 succeeds.
 * With z_i = groth16_verify_batch_combined's coefficients (same rule, i = the index in the caller's arrays), the live items are
 * checked together:
 *     Π_i e(−z_i·A_i, B_i) · Π_k [ e((Σ_{i∈k} z_i)·α₁,k, β₂,k) · e(S_pub,k, γ₂,k) · e(Σ_{i∈k} z_i·C_i, δ₂,k) ] = 1
 * S_pub,k = Σ_j u_j,k·IC_j,k, u_0,k = Σ_{i∈k} z_i, u_{j+1,k} = Σ_{i∈k} z_i·s_ij — with one key, groth16_verify_batch_combined's
 * equation.  The lanes run over all live items at once whatever their keys, the 3·K sums are one segmented multi-scalar sum, the
 * 3·K fixed-G2 Miller loops one launch.  If every pi_b passes the subgroup test and the equation holds, every live item gets 1
 * and report->path = 1 (also when no item is live).  Otherwise path = 0 and the keys are decided one by one from the values
 * already on the device: a key whose own equation (its items' factors and its three pairs) holds and whose items all passed the
 * subgroup test has its items accepted; only the items of the other keys (report->keys_fallback of them, out of
 * report->keys_live keys with a live item) go through groth16_verify_batch's per-item stage, one pass per such key.
 * An invalid item is accepted with probability ≤ 2^-127 per call on the global equation, and per key on the per-key equations,
 * over the seed.  THE SEED MUST BE SECRET AND FRESH, as for groth16_verify_batch_combined: pass NULL outside tests.
 * Not done: bisection inside a failing key (its items all take the per-item stage), several lanes per proof, more than one GPU,
 * proofs in any other form than the JSON texts; the command-line worker has no command for it.
 * Returns 0 when every item was judged; −3 for a null argument (report may be NULL) or no randomness; > 0 for a device failure.
 * report: parse_ms = the host parse, device_ms = the wall time from there to the verdicts. */
typedef struct { int32_t path; uint32_t keys_live, keys_fallback; double parse_ms, device_ms; } Groth16MixedReport;
int groth16_verify_batch_mixed(Groth16VkSet* set, const char* const* proof_jsons, const char* const* public_jsons,
                               const int32_t* key_of, int n, const uint8_t* seed32 /* NULL = OS randomness */,
                               int32_t* verdicts, Groth16MixedReport* report);

/* groth16_zkey_check — is this proving key sound?  Opt-in: groth16_cache_load* and the proves trust the key they are given.
 * Every point of sections 3 (IC), 5 (A), 6 (B1), 7 (B2), 8 (C), 9 (H) and of the header is tested on one GPU, one lane per point,
 * in the file's Montgomery form; section 4 gets the loader's range check plus value < r; then three pair checks.
 * kinds of fault, in the order in which one element is tested: */
#define GROTH16_ZKEY_NONCANONICAL   1  /* a coordinate's 256-bit residue is >= q */
#define GROTH16_ZKEY_OFF_CURVE      2  /* not the identity (0,0) and not on y^2 = x^3 + 3 (G1) / x^3 + 3/xi (G2) */
#define GROTH16_ZKEY_OFF_SUBGROUP   3  /* G2 only: on the twist, outside the order-r subgroup */
#define GROTH16_ZKEY_IDENTITY       4  /* header points only: alpha1, beta1, beta2, gamma2, delta1, delta2 must not be the identity */
#define GROTH16_ZKEY_PAIR_MISMATCH  5  /* beta1/beta2, delta1/delta2, or section 6 against section 7 */
#define GROTH16_ZKEY_COEFFICIENT    6  /* section 4: matrix, constraint or wire out of range, or value >= r */

typedef struct {
  int32_t  kind;          /* 0 = sound, else the kind of the FIRST fault */
  int32_t  section;       /* zkey section id of the first fault: 2 (header), 3, 4, 5, 6, 7, 8, 9 */
  uint64_t index;         /* lowest element index at fault in that section; for the header the position 0..5 in file order;
                             UINT64_MAX for a section-6/7 mismatch, which the randomised check does not localise */
  uint64_t faults[10];    /* faults[s] = elements at fault in section s (membership kinds 1-4 and 6); a mismatch counts 1 in faults[2] or faults[6] */
  double   upload_ms, device_ms, pairing_ms;
} Groth16ZkeyReport;

typedef struct {
  uint32_t slice_points;  /* points per upload slice; 0 = the default */
  const uint8_t* seed32;  /* NULL = 32 bytes from getrandom / /dev/urandom, as groth16_verify_batch_combined */
} Groth16ZkeyCheckOptions;

/* "First" means: sections in ascending id, within a section the lowest index, within an element the kinds in the order 1, 2, 3
 * (4 for a header point).  faults[] is complete for every section whatever came first.
 * Pair checks (kind 5) run only when the sections they read have no membership fault.  The header pairs hold when
 * e(beta1, G2) = e(G1, beta2) and e(delta1, G2) = e(G1, delta2) by the host pairing (index 1 and 4: the G1 member's slot).
 * Sections 6 and 7 hold when S1 = Σ z_i·B1_i and S2 = Σ z_i·B2_i satisfy e(S1, G2) = e(G1, S2), z_i =
 * groth16_verify_combined_coefficients(seed, i) and the sums from the library's MSMs over 128-bit scalars: with every B2_i in G2,
 * a key with some B1_i that is not the G1 image of its B2_i passes with probability <= 2^-127 over the seed, WHICH MUST BE SECRET
 * AND FRESH (opt->seed32 is for reproducible tests; NULL draws from the operating system, and the call returns -3 when that fails).
 * What the check does NOT show: that the key belongs to a given circuit or ceremony, or any relation between A, C, H and IC —
 * groth16_r1cs_match_zkey compares section 4 with an .r1cs, and groth16_zkey_verify_ptau the point sections with the .r1cs and
 * the .ptau, as `snarkjs zkey verify` does.
 * device as groth16_verify_batch ("HIP", "CUDA", "HIP:k").  opt may be NULL.  The call holds no cache entry and needs no
 * Groth16CacheManager; the calling thread's device is what it was afterwards.  report->upload_ms: the host to device copies of the
 * sections, device_ms: the wall time of the device part (buffers, uploads, kernels, MSMs), pairing_ms: the host pairings (the
 * header's four run on a worker thread beside the device part).  ICICLE_SNARK_TRACE_ZKEY_CHECK=1 prints the stage times on stderr.
 * 1 sound, 0 at least one fault (report says which), < 0 an error (groth16_last_error): the loader's own codes for format (-2),
 * I/O (-1) and argument (-3) errors, and -5 for a device failure, whose positive eIcicleError would read as a verdict here. */
int groth16_zkey_check(const void* zkey, size_t len, const char* device, const Groth16ZkeyCheckOptions* opt, Groth16ZkeyReport* report);
int groth16_zkey_check_file(const char* zkey_path, const char* device, const Groth16ZkeyCheckOptions* opt, Groth16ZkeyReport* report);

/* snarkjs verification_key.json text of the key (protocol, curve "bn128", nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, IC;
 * projective third coordinates as snarkjs writes them).  Reads the header and section 3 as they are — groth16_zkey_check is what
 * tests them.  Host only: never initialises a GPU.  Returns the length needed including the terminator (call with cap = 0 to
 * size; `out` is written only when cap is at least that), < 0 on a format error (groth16_last_error). */
int64_t groth16_zkey_export_vk(const void* zkey, size_t len, char* out, size_t cap);

/* An .r1cs (iden3 binary format, as circom and snarkjs write it) read once and kept on one GPU: the circuit's A, B and C as rows
 * of (wire, coefficient) terms.  Sections are found by id in any order, unknown ids (3: the wire -> label map, 4 and 5: custom
 * gates) are ignored, a missing or duplicated section 1 or 2 is a format error; n_public = nPubOut + nPubIn.
 * groth16_r1cs_info is the host half alone — container, header, and ONE pass over section 2's count words that checks that every
 * count keeps the walk inside the section, that the walk consumes it exactly and that the term total fits 32 bits.  It never
 * initialises a GPU.  groth16_r1cs_load then uploads the section in slices and a kernel unpacks the 36-byte records into aligned
 * (wire, Montgomery coefficient) arrays, testing wire < nWires and coefficient < r first; a bad record fails the load with -2
 * and a text naming the lowest constraint at fault, its matrix and the kind.  A handle exists only when every wire id is in range.
 * SAFETY: no byte of a hostile or truncated file can make a kernel read outside its buffers — the host walk bounds every record
 * before anything is uploaded, and the fill kernel bounds every wire id before anything gathers with it.
 * device as groth16_verify_batch ("HIP", "CUDA", "HIP:k"; a list is an error).  -1 I/O, -2 format, -3 argument, -5 device failure
 * (groth16_last_error).  The calling thread's device is afterwards what it was before.  A handle serves one call at a time (calls
 * on one handle are serialised); groth16_r1cs_free(NULL) does nothing. */
typedef struct Groth16R1cs Groth16R1cs;
typedef struct {
  uint32_t n_wires, n_public, n_constraints;
  uint64_t n_terms;        /* non-zero entries of A, B and C together */
  uint64_t device_bytes;   /* what the handle keeps on the device (0 from groth16_r1cs_info) */
  double   walk_ms;        /* the host pass over the count words */
  double   upload_ms;      /* host to device copies of section 2 (0 from groth16_r1cs_info) */
  double   device_ms;      /* wall time of the device part: buffers, uploads, the fill kernel */
} Groth16R1csInfo;
int  groth16_r1cs_info(const void* r1cs, size_t len, Groth16R1csInfo* info);
int  groth16_r1cs_load(const void* r1cs, size_t len, const char* device, Groth16R1cs** out);
int  groth16_r1cs_load_file(const char* path, const char* device, Groth16R1cs** out); /* maps the file */
int  groth16_r1cs_get_info(const Groth16R1cs* h, Groth16R1csInfo* info); /* what the load measured */
void groth16_r1cs_free(Groth16R1cs* h);

/* groth16_witness_check — does this witness satisfy this circuit?  Exact, on the GPU; what `snarkjs wtns check` answers.
 * Opt-in: the proves do not run it (their QAP front end takes A∘B for the third row, so an unsatisfying witness yields a proof
 * that fails verification and nothing says why).  kinds of fault, in the order of testing: */
#define GROTH16_WTNS_NONCANONICAL 1   /* a witness value >= r; index = the lowest such wire */
#define GROTH16_WTNS_ONE          2   /* wire 0 is not 1; index = 0 */
#define GROTH16_WTNS_CONSTRAINT   3   /* (A_j·w)(B_j·w) != C_j·w; index = the lowest such j */
typedef struct {
  int32_t  kind;           /* 0 = satisfied, else the kind of the FIRST fault */
  uint64_t index;
  uint64_t noncanonical;   /* witness values >= r */
  uint64_t failed;         /* violated constraints, all of them; 0 when noncanonical != 0: the constraints are evaluated only
                              over canonical values, which the field routines' bounds assume */
  double   upload_ms, device_ms; /* the witness's host to device copy; wall time of the device part (upload and both kernels) */
} Groth16WitnessReport;
/* The .wtns is parsed as the proves parse it; a witness count other than nWires is -3.  An empty linear combination evaluates
 * to 0, a wire named twice in one sums.  Only the tallies come back from the device.  1 satisfied, 0 not (report says why),
 * < 0 an error with the loader's codes. */
int groth16_witness_check(Groth16R1cs* h, const void* wtns, size_t wtns_len, Groth16WitnessReport* report);
int groth16_witness_check_file(Groth16R1cs* h, const char* wtns_path, Groth16WitnessReport* report);

/* groth16_r1cs_match_zkey — does this proving key carry this circuit's A and B?  kinds of fault, in the order of reporting: */
#define GROTH16_MATCH_SIZES 1   /* index: 0 n_vars vs nWires, 1 n_public vs nPubOut + nPubIn, 2 domain_size */
#define GROTH16_MATCH_ROW_A 2   /* index = the lowest row of the domain whose A differs */
#define GROTH16_MATCH_ROW_B 3
typedef struct {
  int32_t  kind;           /* 0 = match, else the kind of the FIRST fault: sizes, then A, then B */
  uint64_t index;
  uint64_t rows_a, rows_b; /* rows that differ, all of them (0 after a sizes fault: nothing was compared) */
  double   device_ms;      /* wall time of the device part: buffers, uploads, kernels */
} Groth16R1csMatchReport;
/* Sizes first, on the host: n_vars = nWires, n_public = nPubOut + nPubIn, and domain_size the smallest power of two
 * >= mConstraints + n_public + 1 (snarkjs' rule).  Then both sides are evaluated at ONE vector z of nWires coefficients, z_i =
 * groth16_verify_combined_coefficients(seed, i): the circuit's rows A_j·z and B_j·z by the witness check's kernel, the key's
 * section 4 by the prover's own CSR build and sparse product with z in the witness's place.  Row j of the key's A must equal
 * A_j·z for j < m, z_{j-m} for m <= j <= m + n_public (the rows snarkjs adds to bind the public signals) and 0 above; row j of its
 * B must equal B_j·z for j < m and 0 above.  A row whose coefficients differ from the circuit's is a non-zero linear form in the
 * z_i, zero for at most one value of one z_i: it is accepted with probability <= 2^-127 over the seed, WHICH MUST BE SECRET AND
 * FRESH (seed32 is for reproducible tests; NULL draws from the operating system, and the call returns -3 when that fails).  The
 * comparison does not depend on the order of section 4's records or on records of one entry that sum.
 * What it does NOT show: anything about C, which section 4 does not hold; and that the point sections 3 and 5 to 9 belong to
 * these matrices — both are groth16_zkey_verify_ptau's, which needs the .ptau.  Section 4's values are taken as the prover takes them —
 * groth16_zkey_check is what tests value < r.
 * 1 match, 0 not (report says where), < 0 an error with the loader's codes (-2 also for a section-4 record out of range). */
int groth16_r1cs_match_zkey(Groth16R1cs* h, const void* zkey, size_t len, const uint8_t* seed32 /* NULL = OS randomness */,
                            Groth16R1csMatchReport* report);

/* A prepared .ptau (snarkjs' powers-of-tau container after `powersoftau prepare phase2`), as groth16_zkey_verify_ptau reads it:
 * magic "ptau", version 1; section 1 = {n8 = 32, q, power, ceremonyPower}; sections 4, 5, 6 = [alpha*tau^i]1, [beta*tau^i]1, [beta]2;
 * sections 12, 13, 14, 15 = [L_j(tau)]1, [L_j(tau)]2, [alpha*L_j(tau)]1, [beta*L_j(tau)]1 with one block per power p = 0, 1, ... of
 * 2^p elements beginning at element 2^p - 1 (section 12 goes on to power + 1).  Points are uncompressed, affine, Montgomery form.
 * groth16_ptau_info reads container and header: -2 for a malformed file, with a text of its own when sections 12 to 15 are
 * missing (the file has not been prepared for phase 2).  domain_power >= 0 also asks whether the file serves a key of domain
 * 2^domain_power: -3 when power is below it (both numbers in the text), -2 when a block the verify would read — block k of
 * sections 12 to 15, block k + 1 of section 12 — does not lie inside its section.  Nothing more is demanded of the lengths.
 * Host only: never initialises a GPU. */
typedef struct {
  uint32_t power, ceremony_power;
  uint64_t section_bytes[16];  /* payload bytes per section id; 0 = absent */
} Groth16PtauInfo;
int groth16_ptau_info(const void* ptau, size_t len, int32_t domain_power /* -1: none */, Groth16PtauInfo* info);

/* groth16_zkey_verify_ptau — is this proving key the Groth16 key of THIS circuit over THIS ceremony?  What `snarkjs zkey verify
 * circuit.r1cs pot.ptau key.zkey` answers for the point sections, on the GPU.  Opt-in, like the other checks.
 * Notation: nc constraints, m wires, npub public signals, n = 2^k the domain; L_j the Lagrange basis of the size-n domain, L'_j
 * that of the size-2n domain; tau, alpha, beta the ptau's; gamma2, delta2 the key header's.  From a seed, z_s =
 * groth16_verify_combined_coefficients(seed, s) for s < m and y_i = ...(seed, m + i) for i < n; z^pub is z with the private wires
 * (s > npub) zeroed, z^priv = z - z^pub.  For a vector v, a(v)_j = A_j*v for j < nc, v_{j-nc} on the public-binding rows
 * nc <= j <= nc + npub, 0 above; b(v)_j = B_j*v and c(v)_j = C_j*v for j < nc, 0 above.  kinds of fault, in the order of testing: */
#define GROTH16_VERIFY_SIZES   1   /* index: 0 n_vars vs nWires, 1 n_public, 2 domain_size (as groth16_r1cs_match_zkey) */
#define GROTH16_VERIFY_KEY     2   /* groth16_zkey_check finds a fault: report->key says which; no equation was evaluated (but see below) */
#define GROTH16_VERIFY_HEADER  3   /* index: 0 alpha1 != section 4 element 0, 1 beta1 != section 5 element 0, 2 beta2 != section 6 */
#define GROTH16_VERIFY_A       4   /* sum_s z_s*A_s (section 5)   !=  sum_j a(z)_j*[L_j]1                    in G1 */
#define GROTH16_VERIFY_B1      5   /* sum_s z_s*B1_s (section 6)  !=  sum_j b(z)_j*[L_j]1                    in G1 */
#define GROTH16_VERIFY_B2      6   /* sum_s z_s*B2_s (section 7)  !=  sum_j b(z)_j*[L_j]2                    in G2 */
#define GROTH16_VERIFY_IC      7   /* e(sum_{s<=npub} z_s*IC_s, gamma2) != e(T(z^pub), G2),
                                      T(v) = sum_j ( a(v)_j*[beta*L_j]1 + b(v)_j*[alpha*L_j]1 + c(v)_j*[L_j]1 ) */
#define GROTH16_VERIFY_C       8   /* e(sum_{s>npub} z_s*C_{s-npub-1}, delta2) != e(T(z^priv), G2) */
#define GROTH16_VERIFY_H       9   /* e(sum_i y_i*H_i, delta2) != e(sum_i y_i*[L'_{2i+1}]1, G2)   (section 12, block k + 1, odd elements) */
typedef struct {
  int32_t  kind;           /* 0 = the key verifies, else the kind of the FIRST fault in the order above */
  uint64_t index;          /* for SIZES and HEADER only */
  uint32_t failed_mask;    /* bit (kind - GROTH16_VERIFY_HEADER) for HEADER, A, B1, B2, IC, C, H: every equation that fails,
                              whatever failed first (0 after SIZES or KEY: nothing was evaluated) */
  Groth16ZkeyReport key;   /* groth16_zkey_check's report on the key (zeroed after a SIZES fault) */
  double   upload_ms, device_ms, pairing_ms; /* this call's own uploads; wall time of its device part (buffers, uploads, kernels,
                                                MSMs); the six host pairings — the embedded report has the key check's */
} Groth16ZkeyVerifyReport;
/* The left sides are the library's MSMs over 128-bit scalars, the right sides full-width MSMs over the ptau's block for n; A, B1
 * and B2 are compared as points, IC, C and H by two host pairings each; the identity on both sides holds, on one side fails (a
 * circuit without private wires has an empty section 8, and C holds).  The H row is snarkjs' H from the odd Lagrange points of
 * the doubled domain; this library's synthesised keys use the same basis (L_i(tau/g)*(tau^n - 1)/(-2*delta) = L'_{2i+1}(tau)/delta).
 * SOUNDNESS.  Every equation is a linear form in the z_s or the y_i; a section that differs from the true one in any element is
 * accepted with probability <= 2^-127 per equation, so < 2^-124 for the call, over the seed, WHICH MUST BE SECRET AND FRESH
 * (seed32 is for reproducible tests; NULL draws from the operating system, and the call returns -3 when that fails).  The
 * argument needs every key point on its curve and every B2_s in the subgroup, so groth16_zkey_check runs first, with the same
 * seed, and the verdict is 1 only when it says sound; delta1/delta2 and beta1/beta2 are its pair tests.  One fault of its does
 * not end the call: a mismatch of section 6 against section 7 as the key's only fault leaves every point where the sums are
 * defined, so the equations run and B1 or B2 names the section that is not the circuit's (report->key still shows the
 * mismatch; should both hold nonetheless, the kind is KEY).  The ptau ranges that are
 * read get the same lane tests (coordinates < q, on the curve, section 13 in the subgroup); a ptau point that fails is a format
 * error (-2) naming section and element.  HEADER compares the stored Montgomery words, which the key check has found canonical.
 * What it does NOT show: anything about the .ptau itself, which is taken as given (groth16_ptau_verify, below, is what judges it);
 * the phase-2 contribution chain of section 10 and snarkjs' circuit hash; WHICH element of a section is wrong (a failing
 * equation is not localised); section 4, which remains groth16_r1cs_match_zkey's.
 * The key's sections go up twice — once inside the key check, once for the MSMs — so that the key check stays what it is.
 * report->upload_ms etc. as groth16_zkey_check.  ICICLE_SNARK_TRACE_ZKEY_VERIFY=1 prints the stage times on stderr.
 * 1 verifies, 0 not (report says why), < 0 an error (groth16_last_error): -1 I/O, -2 format (either file), -3 argument (also a
 * ptau whose power is below the domain's), -5 device failure.  The _file variant maps both files and uploads only the ranges
 * it reads: a power-22 .ptau is several GB. */
int groth16_zkey_verify_ptau(Groth16R1cs* h, const void* zkey, size_t zkey_len, const void* ptau, size_t ptau_len,
                             const uint8_t* seed32 /* NULL = OS randomness */, Groth16ZkeyVerifyReport* report);
int groth16_zkey_verify_ptau_file(Groth16R1cs* h, const char* zkey_path, const char* ptau_path, const uint8_t* seed32,
                                  Groth16ZkeyVerifyReport* report);

/* groth16_zkey_new — the Groth16 proving key of THIS circuit over THIS ceremony, before any phase-2 contribution: what `snarkjs
 * zkey new circuit.r1cs pot.ptau out.zkey` writes, made on the GPU.  Opt-in; nothing else in the library calls it.
 * WHAT IT IS NOT: a key to prove with in production.  Its gamma and delta are 1 (gamma2 = delta2 = G2, delta1 = G1): whoever knows
 * that can forge proofs, until a phase-2 contribution has replaced delta: groth16_zkey_contribute, below, applies one and
 * groth16_zkey_contributions audits the chain.  The call builds and does not verify — the .ptau is taken
 * as given; groth16_zkey_check, groth16_r1cs_match_zkey and groth16_zkey_verify_ptau are what judge the result.
 * Notation as above: nc constraints, m wires, npub public signals, n = 2^k the smallest power of two >= nc + npub + 1.  For a wire s
 *   A_s  = sum_j A[j,s]*[L_j]1 (+ [L_{nc+s}]1 for s <= npub: the rows snarkjs adds to bind the public signals)
 *   B1_s = sum_j B[j,s]*[L_j]1,   B2_s = sum_j B[j,s]*[L_j]2
 *   comb_s = sum_j ( A[j,s]*[beta*L_j]1 + B[j,s]*[alpha*L_j]1 + C[j,s]*[L_j]1 ) (+ [beta*L_{nc+s}]1 for s <= npub)
 * THE FILE: sections 1 to 10 in this order.  2: n8, q, n8, r, m, npub, n, then alpha1 = ptau section 4 element 0, beta1 = section 5
 * element 0, beta2 = section 6 (the stored words, copied), gamma2 = G2, delta1 = G1, delta2 = G2.  3: comb_s for s <= npub.  4: a
 * count and one record {matrix, row, wire, value*R^2 mod r} per term of A and of B as the .r1cs lists them — zero coefficients and
 * repeated wires kept — constraint by constraint, A's terms then B's, then the npub + 1 binding records (0, nc + s, s, 1).  5, 6,
 * 7: A, B1, B2.  8: comb_s for s > npub (empty for a circuit without private wires).  9: [L'_{2i+1}]1, i < n — section 12, block
 * k + 1, odd elements.  10: a zero contribution count; snarkjs' 64-byte circuit hash is NOT written.  Points are affine,
 * Montgomery form, the identity (0, 0); a wire that appears in no matrix is all-zero bytes.
 * groth16_zkey_new_size is the host half: the file's size and section 4's record count (terms of A + terms of B + npub + 1) from
 * the .r1cs alone, with groth16_r1cs_info's walk and its codes.  It never initialises a GPU.
 * The .ptau is read as groth16_zkey_verify_ptau reads it: block k of sections 12 to 15 and block k + 1 of section 12 go up and
 * through the lane tests before anything reads them.  A column of more than heavy_column_terms terms (the constant wire can sit in
 * every constraint) is cut into items that a workgroup each sums; the result does not depend on the threshold. */
typedef struct {
  uint32_t heavy_column_terms;   /* 0 = the default */
} Groth16ZkeyNewOptions;
typedef struct {
  uint32_t n_vars, n_public, domain;
  uint64_t n_coeffs, zkey_bytes;           /* section 4's records; the file (also when cap was too small) */
  uint32_t longest_column;                  /* terms of the longest (matrix, wire) column, binding rows included */
  uint32_t heavy_columns, heavy_items;      /* sums that were cut, and the items they were cut into */
  double   upload_ms, device_ms, download_ms, write_ms; /* the ptau ranges' copies; wall time of the device part up to the last
                                               kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16ZkeyNewReport;
/* 0 built; -1 I/O; -2 format: a ptau that is not prepared for phase 2, or a ptau point of a range that is read failing its lane
 * test (the text names section, block and element); -3 argument: a ptau whose power is below the domain's (both numbers in the
 * text), or cap too small (report->zkey_bytes still says what is needed); -5 device failure (groth16_last_error).  The _file
 * variant maps the .ptau and uploads only the ranges it reads, writes to a temporary beside zkey_path and renames it: a failed
 * call leaves no file there.  The calling thread's device is what it was afterwards; calls on one handle are serialised.
 * ICICLE_SNARK_TRACE_ZKEY_NEW=1 prints the stage times on stderr. */
int groth16_zkey_new_size(const void* r1cs, size_t len, uint64_t* zkey_bytes, uint64_t* n_coeffs);
int groth16_zkey_new(Groth16R1cs* h, const void* ptau, size_t ptau_len, void* zkey_out, size_t cap, const Groth16ZkeyNewOptions* opt,
                     Groth16ZkeyNewReport* report);
int groth16_zkey_new_file(Groth16R1cs* h, const char* ptau_path, const char* zkey_path, const Groth16ZkeyNewOptions* opt,
                          Groth16ZkeyNewReport* report);

/* groth16_setup — the Groth16 proving key of a loaded circuit made DIRECTLY from toxic waste (tau, alpha, beta, gamma, delta) on
 * one GPU, without any .ptau: what arkworks' generate_random_parameters, gnark's groth16.Setup, bellman and `snarkjs groth16 setup`
 * offer.  Opt-in; nothing else in the library calls it.  For development, CI, benchmarks on one's own circuit, and deployments where
 * prover and verifier are one party.
 * WHAT IT IS NOT: **whoever ran the call can forge proofs for the key.**  The five scalars existed in that process's memory; they
 * are wiped on the host (explicit_bzero) and every device buffer that held a scalar derived from them is overwritten before it is
 * freed, which is best effort — registers, spills and the operating system's copies are out of reach.  groth16_zkey_contribute
 * afterwards protects only delta; tau, alpha and beta stay known to the runner.  A key for third parties comes from the ceremony
 * chain (ptau-new -> ptau-contribute -> ptau-prepare -> zkey-new -> zkey-contribute).
 * THE KEY: the layout, the sizes and section 4 are groth16_zkey_new's (groth16_zkey_new_size gives the size), byte for byte what
 * synth.setup writes for the same five scalars; with gamma = delta = 1 it is groth16_zkey_new's key over a .ptau of the same tau,
 * alpha, beta.  With n the domain, w its root of unity, g the root of order 2n and L_j(x) = w^j (x^n - 1) / (n (x - w^j)):
 *   a_s = sum_j A[j,s]*L_j(tau) (+ L_{nc+s}(tau) for s <= npub), b_s, c_s likewise from B and C;  A_s = [a_s]1, B1_s = [b_s]1,
 *   B2_s = [b_s]2;  comb_s = beta*a_s + alpha*b_s + c_s;  IC_s = [comb_s/gamma]1 (s <= npub), C_s = [comb_s/delta]1 (s > npub);
 *   H_j = [L_j(tau/g) * (tau^n - 1) / (-2 delta)]1;  the header holds [alpha]1 [beta]1 [beta]2 [gamma]2 [delta]1 [delta]2.
 * A wire in no matrix, or whose column cancels, is the identity: all-zero bytes.  Section 10 has a zero count, so
 * groth16_zkey_contributions answers as it does for any key with delta != 1 and no record.
 * toxic160: tau, alpha, beta, gamma, delta as five 32-byte little-endian standard-form scalars — for tests and reproducible
 * benchmarks.  NULL: the operating system's randomness, redrawn until valid.  groth16_setup_toxic_check (host only, never
 * initialises a GPU) returns 0, or the kind of the first fault: GROTH16_TOXIC_RANGE a scalar >= r, GROTH16_TOXIC_ZERO a zero among
 * the five, GROTH16_TOXIC_DOMAIN tau^(2n) = 1 for n = 2^domain_power — tau in the domain or in its coset g*domain, where a Lagrange
 * denominator vanishes (-3: a null pointer or domain_power > 27).  groth16_setup runs it before any device work: a fault is -2 with
 * a message naming the scalar and the kind, nothing is written and the caller's buffer is untouched.
 * A column of more than heavy_column_terms terms is cut into items that a workgroup each sums in Fr; field addition is exact, so no
 * byte depends on the threshold.
 * WHAT IT DOES NOT DO: read a zkez or any packed input; use more than one GPU; write a .ptau; write snarkjs' circuit hash. */
enum { GROTH16_TOXIC_RANGE = 1, GROTH16_TOXIC_ZERO = 2, GROTH16_TOXIC_DOMAIN = 3 };
typedef struct {
  uint32_t heavy_column_terms;   /* 0 = the default */
} Groth16SetupOptions;
typedef struct {
  uint32_t n_vars, n_public, domain;
  uint64_t n_coeffs, zkey_bytes;           /* section 4's records; the file (also when cap was too small) */
  uint32_t longest_column;                  /* terms of the longest (matrix, wire) column, binding rows included */
  uint32_t heavy_columns, heavy_items;      /* columns that were cut, and the items they were cut into */
  double   upload_ms, device_ms, download_ms, write_ms; /* the tables' copies; wall time of the device part up to the last
                                               kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
  double   lagrange_ms, columns_ms, g1_ms, g2_ms;       /* device time by stage: the Lagrange rows; the column sums and outputs;
                                               the fixed-base multiplications of the G1 array; of the G2 array (beside G1's) */
} Groth16SetupReport;
/* 0 built; -1 I/O; -2 the toxic waste (above); -3 argument: a null handle or report, a domain above 2^27, or cap too small
 * (report->zkey_bytes still says what is needed); -5 device failure (groth16_last_error).  The _file variant writes to a temporary
 * beside zkey_path and renames it: a failed call leaves no file there.  The calling thread's device is what it was afterwards;
 * calls on one handle are serialised.  ICICLE_SNARK_TRACE_ZKEY_SETUP=1 prints the stage times on stderr. */
int groth16_setup_toxic_check(const uint8_t toxic160[160], uint32_t domain_power);
int groth16_setup(Groth16R1cs* h, const uint8_t* toxic160, void* zkey_out, size_t cap, const Groth16SetupOptions* opt,
                  Groth16SetupReport* report);
int groth16_setup_file(Groth16R1cs* h, const uint8_t* toxic160, const char* zkey_path, const Groth16SetupOptions* opt,
                       Groth16SetupReport* report);

/* groth16_zkey_contribute — one phase-2 contribution applied to a proving key on the GPU: what makes groth16_zkey_new's key a key
 * to prove with.  Opt-in; nothing else in the library calls it.  The contributor's secret is delta' in [1, r):
 *   header   delta1 <- delta'*delta1, delta2 <- delta'*delta2; everything else of section 2 stays byte for byte
 *   8, 9     every point of C and of H becomes delta'^-1 * P — ONE scalar for |8| + |9| points: zc_scale_g1_kernel, a lane per point
 *   10       one record appended (the section is created behind the last one when the key has none)
 *   1, 3, 4, 5, 6, 7 and any other section: copied, in the input's order.
 * The identity stays all-zero bytes and affine Montgomery bytes are canonical, so the result is a function of (key, delta') alone.
 * Every point of 8 and 9 passes the key check's lane test (coordinates < q, on the curve) before any arithmetic sees it; a
 * point that fails is -2 with a text naming section, index and kind, and nothing is written.  The header's delta1 and delta2 get
 * the same tests on the host (delta2: in the subgroup), and an identity delta is refused (-2).
 * SECTION 10 — THIS LIBRARY'S OWN LAYOUT.  snarkjs' record needs BLAKE2b, its ChaCha-seeded hash-to-G2 and its circuit hash; what
 * is written here is instead: u32 count, then count records
 *   after1   64 B   delta1 after this contribution (affine, Montgomery form, as the header)
 *   R        64 B   the commitment k*before1, same form
 *   z        32 B   the response, standard form little-endian, < r
 *   name_len u32    <= 255
 *   name     name_len bytes
 * with TAG = "icicle-snark zkey contribution v1" (ASCII, no terminator); before1 of record 1 = the header's delta1 at the time of
 * contributing, of record i = record i-1's after1; h_0 = SHA-256(TAG || section 2 bytes [0, 468) || section 3) — everything up to
 * and including gamma2, and IC: what no contribution changes; e_i = SHA-256(h_{i-1} || before1 || after1 || R || name_len || name),
 * h_i = e_i; the challenge c_i = the first 16 bytes of e_i, little-endian, 0 replaced by 1; z = k + c*delta' mod r (Schnorr), which
 * a verifier checks as z*before1 = R + c*after1.  A KEY CONTRIBUTED HERE CONTINUES ITS CEREMONY HERE: snarkjs reads sections 2 to 9
 * to prove and to export the vk, which are unaffected, but its `zkey verify` and `zkey contribute` do not read this section 10.
 * SECRETS, from the caller's 32 bytes (secret32 = NULL: the operating system's).  W(x) = SHA-256(x || 0x00) || SHA-256(x || 0x01) read
 * as a 512-bit big-endian integer, mod r.  delta' = W(secret || TAG) unless opt->fixed_delta (32 bytes, standard form little-endian,
 * 0 < . < r: for tests and reproducible runs) gives it; k = W(secret || delta' as 32 B LE || h_{i-1} || before1), so one secret used
 * on two keys does not leak delta'.  A zero delta' or k is -3.  The host copies of secret, delta', delta'^-1, k and the digit masks
 * are wiped (explicit_bzero) before the call returns — best effort: the masks also travel to the device as kernel arguments, and
 * the kernel's duration depends on them.
 * The output's size is known before any device work: the input, plus the record (164 + name bytes), plus 12 when section 10 was
 * absent; cap is tested first, and a short cap is -3 with report->zkey_bytes set and nothing written.
 * 0 done; -1 I/O; -2 format: a malformed key, a faulty point of section 8 or 9, a malformed section 10 (or one whose last after1 is
 * not the header's delta1); -3 argument: a name over 255 bytes, a bad fixed_delta, cap too small, equal paths; -5 device failure
 * (groth16_last_error).  The _file variant maps the input, writes a temporary beside out_path and renames it: a failed call leaves
 * nothing.  The calling thread's device is what it was afterwards.  ICICLE_SNARK_TRACE_ZKEY_CONTRIBUTE=1 prints the stage times. */
typedef struct {
  const uint8_t* fixed_delta;   /* NULL, or delta' itself: 32 bytes, standard form little-endian, 0 < delta' < r */
} Groth16ZkeyContributeOptions;
typedef struct {
  uint32_t contribution;        /* this record's number: 1 for the first */
  uint64_t points_c, points_h;  /* points of section 8 and of section 9 */
  uint64_t zkey_bytes;          /* the output (also when cap was too small) */
  int32_t  fault_section, fault_kind;   /* after a faulty point: 8 or 9, and GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE */
  uint64_t fault_index, faults;         /* the first such point's index in its section; how many there are */
  double   upload_ms, device_ms, download_ms, write_ms; /* the sections' copies up; wall time of the device part up to the last
                                   kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16ZkeyContributeReport;
int groth16_zkey_contribute(const void* zkey, size_t len, const uint8_t* secret32 /* NULL = OS randomness */, const char* name,
                            void* out, size_t cap, const char* device, const Groth16ZkeyContributeOptions* opt,
                            Groth16ZkeyContributeReport* report);
int groth16_zkey_contribute_file(const char* zkey_path, const char* out_path, const uint8_t* secret32, const char* name,
                                 const char* device, const Groth16ZkeyContributeOptions* opt, Groth16ZkeyContributeReport* report);

/* groth16_zkey_contributions — is section 10 a chain of valid contributions that ends in this key's delta?  Host only: never
 * initialises a GPU.  A key without section 10 counts as zero records.  kinds of fault, in the order of testing: */
#define GROTH16_CONTRIB_SECTION 1   /* the count or a record does not fit the section (or section 10 is duplicated); index = the record, 0 for the count */
#define GROTH16_CONTRIB_POINT   2   /* a record's after1 or R has a coordinate >= q or is off the curve, or after1 is the identity */
#define GROTH16_CONTRIB_POK     3   /* z >= r, or z*before1 != R + c*after1.  Record 1 is checked against before1 = G1: a chain that did
                                       not start from groth16_zkey_new's delta = 1 fails here at index 1 */
#define GROTH16_CONTRIB_HEADER  4   /* the last after1 is not the header's delta1; or count = 0 and delta1 != G1 */
#define GROTH16_CONTRIB_PAIR    5   /* e(delta1, G2) != e(G1, delta2) */
typedef struct {
  uint32_t count;            /* records in section 10 (0 after a SECTION fault of the count) */
  int32_t  kind;             /* 0 = the chain holds, else the kind of the FIRST fault */
  uint32_t index;            /* the record at fault, 1 for the first; 0 for HEADER, PAIR and the count */
} Groth16ContributionsReport;
typedef struct {
  uint8_t after1[64];        /* as the record holds it */
  char    name[256];         /* zero-terminated */
} Groth16ContributionInfo;
/* infos (may be NULL) receives after1 and the name of the first min(count, infos_cap) records whose bounds hold.
 * What it does NOT show: that sections 8 and 9 follow delta2 — that C and H really were scaled.  That is
 * groth16_zkey_verify_ptau's, which pairs both against the header's delta2; run both.
 * 1 the chain holds, 0 not (report says where), < 0 an error (-2: the key's container or header is malformed). */
int groth16_zkey_contributions(const void* zkey, size_t len, Groth16ContributionsReport* report, Groth16ContributionInfo* infos,
                               size_t infos_cap);

/* groth16_ptau_prepare — sections 12 to 15 of a powers-of-tau file from its sections 2 to 5, on the GPU: what `snarkjs powersoftau
 * prepare phase2` makes, the first link of ptau-prepare -> zkey-new -> zkey-contribute -> zkey-verify -> prove -> verify.  Opt-in.
 * THE INPUT is an UNPREPARED file, what a ceremony ends with: magic "ptau", version 1; section 1 = {n8 = 32, q, power <= 28,
 * ceremonyPower}; section 2 = [tau^i]1 for i < 2^(power+1) - 1; sections 3, 4, 5 = [tau^i]2, [alpha*tau^i]1, [beta*tau^i]1 for
 * i < 2^power; section 6 = [beta]2; section 7 = the contributions (not read) — each once, with exactly these element counts (-2
 * naming the section and both sizes otherwise).  A file that has one of 12 to 15 is -2 with a text of its own ("already prepared").
 * THE OUTPUT is the input byte for byte — sections 1 to 7 and whatever else it holds — with the header's section count four
 * higher and sections 12, 13, 14, 15 appended in this order.  Points stay uncompressed, affine, Montgomery form, the identity all
 * zero; affine bytes are canonical, so the output is a function of the input alone.
 * DEFINITION.  w_p = the root of unity of order 2^p that bn254_get_root_of_unity(2^p) returns.  Block p of a section begins at
 * element 2^p - 1 and its element j < 2^p is
 *     (1/2^p) * sum_{i < 2^p} w_p^(-i*j) * S_i
 * with S_i element i of the source section: 2 -> 12, 3 -> 13, 4 -> 14, 5 -> 15.  Blocks run p = 0 ... power; section 12 has one
 * more, p = power + 1.  For the sources as above this is [L_j(tau)]1, [L_j(tau)]2, [alpha*L_j(tau)]1, [beta*L_j(tau)]1 of the
 * size-2^p domain, what groth16_ptau_info describes.
 * SECTION 12's LAST BLOCK.  Section 2 holds 2^(power+1) - 1 powers, one fewer than that block's transform takes: its last input
 * S_(2N-1), N = 2^power, is THE IDENTITY — the transform of the zero-extended vector, which is what snarkjs does.  With L'_j the
 * Lagrange basis of the size-2N domain and w' = w_(power+1) the block therefore holds
 *     L'_j(tau) - tau^(2N-1) * w'^(-j*(2N-1)) / (2N)      and not L'_j(tau),
 * which a writer that knows tau (this library's test synthesiser) puts there.  Both give valid keys: the block is only read for a
 * circuit whose domain is 2^power, as the H basis [L'_(2i+1)]1; the quotient polynomial has degree <= 2N - 2, its coefficient of
 * x^(2N-1) is zero, and sum_j p(w'^j) * block_j = p(tau) for every p of degree <= 2N - 2.  groth16_zkey_verify_ptau compares H
 * against whatever block the file holds.  A power of 28 is -3: that block would need a root of order 2^29.
 * Every point of sections 2 to 5 passes the key check's lane test before any arithmetic sees it (coordinates < q, on the curve,
 * section 3 in the subgroup; section 6 on the host); a point that fails is -2 with a text naming section, element and kind, the
 * report says the same, *out_len is 0 and the _file entry leaves no file.  Sections are tested as they are reached: the caller's
 * buffer may by then hold earlier sections; nothing of it is valid unless the call returns 1.
 * The transform runs block by block, section by section, decimation in time with affine points between the levels: one lane per
 * butterfly, T = w*Q by a signed-digit walk with a twiddle per lane, then P + T and P - T; every degenerate case (an identity
 * input, T = +-P, w = 1) is exact.  One path for every level: there is no switch point between kernels, so no such argument.
 * groth16_ptau_prepared_size is the host half: the output's size from the input's container alone.  Never initialises a GPU.
 * What it does NOT do: check its source's powers against one another or its records (groth16_ptau_verify and
 * groth16_ptau_contributions do: run them first), apply phase-1 contributions (a beacon is one: groth16_ptau_beacon), use more than one GPU.  No file written by snarkjs exists offline: reader and writer share the layout stated here.
 * 1 prepared; -1 I/O; -2 format; -3 argument: cap too small (report->ptau_bytes says what is needed, nothing is written), power 28,
 * equal paths, a device string that does not name one HIP device; -5 device failure (groth16_last_error).  The _file variant maps
 * the input, writes a temporary beside out_path and renames it: a failed call leaves nothing.  The calling thread's device is what
 * it was afterwards.  ICICLE_SNARK_TRACE_PTAU_PREPARE=1 prints the stage times on stderr. */
typedef struct {
  uint32_t power;
  uint64_t points[4];           /* points of sections 12, 13, 14, 15 */
  uint64_t ptau_bytes;          /* the output (also when cap was too small) */
  int32_t  fault_section, fault_kind;   /* after a faulty point: 2 to 6, and GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP */
  uint64_t fault_index;                 /* the lowest faulty element of that section */
  double   upload_ms, device_ms, download_ms, write_ms; /* the sources' and the twiddles' copies up; wall time of the device part
                                   without the downloads; the blocks' copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16PtauPrepareReport;
int groth16_ptau_prepared_size(const void* ptau, size_t len, uint64_t* ptau_bytes);
int groth16_ptau_prepare(const void* ptau, size_t len, void* out, size_t cap, uint64_t* out_len, const char* device,
                         Groth16PtauPrepareReport* report);
int groth16_ptau_prepare_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPrepareReport* report);

/* groth16_ptau_new, groth16_ptau_contribute, groth16_ptau_contributions — start a powers-of-tau ceremony, extend it by one
 * participant on the GPU, and audit its record chain on the host: the links before groth16_ptau_prepare.  Opt-in.
 * groth16_ptau_new writes the UNPREPARED file of tau = alpha = beta = 1 (the layout groth16_ptau_prepare states): section 1 with
 * power = ceremonyPower = `power`, 2^(power+1) - 1 copies of G1 as section 2, 2^power copies of G2 as 3, 2^power copies of G1 as 4
 * and as 5, G2 as 6, and a zero count as section 7.  Host only: never initialises a GPU.  groth16_ptau_new_size is its size.  A
 * power above 27 is -3 (groth16_ptau_prepare's own limit); cap is tested before anything is written (-3, *out_len = the bytes needed).
 * A CONTRIBUTION of the secrets tau', alpha', beta' in [1, r) to an unprepared file of N = 2^power:
 *   2        P_i <- tau'^i * P_i, i < 2N - 1         3 (G2)   P_i <- tau'^i * P_i, i < N
 *   4        P_i <- alpha' * tau'^i * P_i, i < N     5        P_i <- beta' * tau'^i * P_i, i < N
 *   6        beta' * P (on the host)                 7        one record appended
 * Section 1 and any unknown section stay byte for byte; sections keep the input's order.  Points leave in the file's form — affine,
 * canonical Montgomery bytes, the identity all zero — so the result is a function of (file, tau', alpha', beta') alone: a file of
 * (tau, alpha, beta) becomes the file of (tau*tau', alpha*alpha', beta*beta').  A prepared file (one of sections 12 to 15) is -2
 * with the unprepared reader's text: contribute first, prepare last.
 * Every point of sections 2 to 5 goes up and through the lane tests (coordinates < q, on the curve, section 3 in the subgroup;
 * section 6 on the host) and every verdict is read before the first scale kernel is launched: a fault is -2 "ptau: section S,
 * element E: kind" naming the lowest faulty element of the first faulty section (6 first), the report says the same, nothing is
 * written.  Then one launch per section, a lane per point: the lane's scalar s = c * tau'^i (c = 1, 1, alpha', beta') is computed
 * ON THE DEVICE from two small tables the host uploads, lo[j] = tau'^j (j < 2^k) and hi_c[m] = c * tau'^(m * 2^k), k = (power + 2)/2,
 * as hi_c[i >> k] * lo[i mod 2^k]; then its non-adjacent form and a signed-digit walk of 256 steps.  No table of 2N powers exists.
 * SECTION 7 — THIS LIBRARY'S OWN LAYOUT, as section 10 of a key contributed here is and for the same reason: snarkjs' record needs
 * BLAKE2b and its hash-to-G2.  What is written is instead: u32 count, then count records of
 *   tau1 64 B, alpha1 64 B, beta1 64 B, tau2 128 B, beta2 128 B    [tau]1 [alpha]1 [beta]1 [tau]2 [beta]2 AFTER this contribution
 *   R_tau 64 B, R_alpha 64 B, R_beta 64 B                          the commitments k_x * before.x1
 *   z_tau 32 B, z_alpha 32 B, z_beta 32 B                          the responses, standard form little-endian, < r
 *   name_len u32 <= 255, name
 * (points affine, Montgomery form) with TAG = "icicle-snark ptau contribution v1" (ASCII, no terminator); `before` of record 1 =
 * (G1, G1, G1), of record i = record i-1's (tau1, alpha1, beta1); h_0 = SHA-256(TAG || section 1's payload); e_i = SHA-256(h_{i-1}
 * || before's three points || the five after points || R_tau || R_alpha || R_beta || name_len || name), h_i = e_i; the challenge
 * c_i = the first 16 bytes of e_i, little-endian, 0 replaced by 1.  One challenge serves three Schnorr proofs with independent
 * nonces: z_x = k_x + c * x' mod r, checked as z_x * before.x1 = R_x + c * after.x1 for x in {tau, alpha, beta}.  The after points
 * are x' times what the FILE holds (section 2 element 1, section 3 element 1, section 4 element 0, section 5 element 0, section 6;
 * at power 0, which holds no power of tau, the last record's tau1 and tau2 or the generators), so a chain over a file that did not
 * start at groth16_ptau_new's fails the audit at record 1.  A FILE CONTRIBUTED HERE CONTINUES ITS CEREMONY HERE: snarkjs reads
 * sections 1 to 6 and 12 to 15 to build keys, which are what they would be, but its `powersoftau verify` and `contribute` do not
 * read this section 7.
 * SECRETS, from the caller's 32 bytes (secret32 = NULL: the operating system's), with groth16_zkey_contribute's W: x' = W(secret ||
 * TAG || label_x), one-byte labels 1, 2, 3 for tau, alpha, beta, unless opt->fixed_tau / fixed_alpha / fixed_beta (32 bytes,
 * standard form little-endian, 0 < . < r: for tests and reproducible runs) gives it; k_x = W(secret || x' as 32 B LE || h_{i-1} ||
 * before.x1 || label_x).  A zero secret or nonce is -3.  The host copies live in one struct that is wiped (explicit_bzero) on every
 * way out, and the device tables are overwritten before they are freed — BEST EFFORT: the compiler may keep copies, the lanes'
 * scalars live in registers and scratch of the device, and a kernel's duration depends on their digits.
 * The output's size is known before any device work: the input plus the record (740 + name bytes).  cap is tested first; a short
 * cap is -3 with report->ptau_bytes set and nothing written.  A section 7 that is malformed, or whose last record is not what the
 * file holds (the HEADER rule below), is -2; earlier proofs are not re-run.
 * 0 done; -1 I/O; -2 format; -3 argument: a name over 255 bytes, a bad fixed secret, cap too small, equal paths (by name or by
 * inode), a device string that does not name one HIP device; -5 device failure (groth16_last_error).  The _file variants write a
 * temporary beside out_path and rename it: a failed call leaves nothing.  The calling thread's device is what it was afterwards.
 * ICICLE_SNARK_TRACE_PTAU_CONTRIBUTE=1 prints the stage times on stderr.
 * What none of this does: check that a file's powers are CONSISTENT WITH ONE ANOTHER — the audit ties the records to element 1 and
 * element 0 of the sections and to section 6, NOT the other 2N - 2 powers: that is groth16_ptau_verify's same-ratio test over all
 * points, below; read or write snarkjs' record format; use more than one GPU; decompose the scalars (GLV). */
int groth16_ptau_new_size(uint32_t power, uint64_t* ptau_bytes);
int groth16_ptau_new(uint32_t power, void* out, size_t cap, uint64_t* out_len);
int groth16_ptau_new_file(uint32_t power, const char* out_path);
typedef struct {
  const uint8_t* fixed_tau;     /* NULL, or tau' itself: 32 bytes, standard form little-endian, 0 < tau' < r */
  const uint8_t* fixed_alpha;   /* the same for alpha' */
  const uint8_t* fixed_beta;    /* the same for beta' */
} Groth16PtauContributeOptions;
typedef struct {
  uint32_t contribution;        /* this record's number: 1 for the first */
  uint32_t power;
  uint64_t points[4];           /* points of sections 2, 3, 4, 5 */
  uint64_t ptau_bytes;          /* the output (also when cap was too small) */
  int32_t  fault_section, fault_kind;   /* after a faulty point: 2 to 6, and GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP */
  uint64_t fault_index;                 /* the lowest faulty element of that section */
  double   upload_ms, device_ms, download_ms, write_ms; /* the sections' and the tables' copies up; wall time of the device part up
                                   to the last kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16PtauContributeReport;
int groth16_ptau_contribute(const void* ptau, size_t len, const uint8_t* secret32 /* NULL = OS randomness */, const char* name,
                            void* out, size_t cap, const char* device, const Groth16PtauContributeOptions* opt,
                            Groth16PtauContributeReport* report);
int groth16_ptau_contribute_file(const char* in_path, const char* out_path, const uint8_t* secret32, const char* name,
                                 const char* device, const Groth16PtauContributeOptions* opt, Groth16PtauContributeReport* report);

/* groth16_ptau_contributions — is section 7 of an unprepared file a chain of valid contributions that ends in what the file holds?
 * Host only: never initialises a GPU.  The kinds are GROTH16_CONTRIB_*, tested in THIS order, the first fault reported:
 *   SECTION  the count or a record does not fit the section; index = the record, 0 for the count
 *   then record by record (index = the record, 1 for the first):
 *   POINT    one of a record's eight points has a coordinate >= q or is off the curve, tau2 or beta2 is outside the subgroup, or
 *            one of the five after points is the identity
 *   POK      a z >= r, or one of the three equations fails
 *   BEACON   (a record that states a beacon only: the beacon block below) over the work bound, or not the recomputed beacon's
 *   PAIR     e(tau1, G2) != e(G1, tau2), or e(beta1, G2) != e(G1, beta2)
 *   and at the end
 *   HEADER   (index 0) the last record's alpha1, beta1, beta2 are not section 4 element 0, section 5 element 0 and section 6, or —
 *            at power >= 1 — its tau1 and tau2 are not element 1 of sections 2 and 3 (at power 0 the file holds no power of tau:
 *            only the pairing ties tau1 to tau2); with count = 0 the generators are compared against those same elements.
 * What it does NOT show: THAT THE OTHER 2N - 2 POWERS FOLLOW — that every point of sections 2 to 5 really was scaled by the power
 * it should have been.  That is a same-ratio test over all points: groth16_ptau_verify, below.  Run both.
 * 1 the chain holds, 0 not (report says where), < 0 an error (-2: the container is malformed, or the file is prepared). */
typedef struct {
  uint32_t count;            /* records in section 7 (0 after a SECTION fault of the count) */
  int32_t  kind;             /* 0 = the chain holds, else the kind of the FIRST fault */
  uint32_t index;            /* the record at fault, 1 for the first; 0 for HEADER and the count */
} Groth16PtauContributionsReport;
typedef struct {
  uint8_t tau1[64], alpha1[64], beta1[64], tau2[128], beta2[128];   /* as the record holds them */
  char    name[256];                                                /* zero-terminated */
} Groth16PtauContributionInfo;
/* infos (may be NULL) receives the points and the name of the first min(count, infos_cap) records whose bounds hold. */
int groth16_ptau_contributions(const void* ptau, size_t len, Groth16PtauContributionsReport* report,
                               Groth16PtauContributionInfo* infos, size_t infos_cap);

/* groth16_ptau_beacon, groth16_zkey_beacon, groth16_beacon_digest, groth16_ptau_beacons, groth16_zkey_beacons — THE RANDOM BEACON:
 * the last step of each ceremony phase, what `snarkjs powersoftau beacon` and `snarkjs zkey beacon` apply.  Opt-in.  DESIGN.md 7o.
 * A beacon is a contribution whose secret is PUBLIC: beacon_hash, 32 bytes nobody could have known before the last participant
 * finished (a block hash, a drand round), stretched by 2^iter_exp sequential hashes so that the last participant cannot choose
 * their share after seeing the outcome: d_0 = beacon_hash, d_(j+1) = SHA-256(d_j), digest = d at j = 2^iter_exp (iter_exp = 0 is
 * ONE hash).  groth16_beacon_digest computes it, on the host; iter_exp above GROTH16_BEACON_ITER_EXP_MAX is -3.
 * THE SECRETS are groth16_ptau_contribute's / groth16_zkey_contribute's with secret := digest and nothing else changed: the same W,
 * tags, labels and nonces.  So the points a beacon writes are, byte for byte, what the contribute call with secret32 = digest
 * writes (sections 2 to 6 of a .ptau; the header and sections 8 and 9 of a .zkey) by the same kernels; only the record differs.
 * THE RECORD is a record of its section (7 or 10) with two differences: BIT 31 of the stored name_len word is set (the name's
 * length is the low bits, still <= 255), and 36 bytes follow the name: beacon_hash (32 B), iter_exp (u32 LE).  e_i hashes the
 * name_len word AS STORED, the name, then those 36 bytes: the beacon's parameters are bound into the chain.  Any other bit above
 * bit 8 of name_len, or a trailer cut short, is a SECTION fault.  A file without beacon records reads and audits as before; a build
 * of this library from before beacons answers SECTION for a file with one (name_len > 255) — the right answer for a reader that
 * cannot audit it.  Contributions may follow a beacon, as in snarkjs: groth16_*_contribute appends behind beacon records.
 * THE AUDIT (groth16_ptau_contributions, groth16_zkey_contributions) tests a flagged record for the new kind BEACON right after its
 * POK has passed (so: SECTION, then per record POINT, POK, BEACON, and for a .ptau PAIR; HEADER and the key's PAIR at the end):
 *   iter_exp > GROTH16_BEACON_ITER_EXP_MAX; or the running total of 2^iter_exp over the file's beacon records, this one included,
 *   exceeds 2^25 (the index is the record that crosses) — both BEFORE any hashing: a hostile file cannot buy more work; or
 *   the record is not the beacon's: with the digest and the secrets recomputed, after.x1 != x' * before.x1 in canonical affine
 *   bytes for one of tau1, alpha1, beta1 (.ptau) or for after1 (.zkey), or a recomputed secret is zero.  The G2 side stays PAIR's.
 * A proof of knowledge of any OTHER x, however honest, is therefore BEACON.  groth16_*_beacons list the flagged records among
 * those the audit lists (the records whose bounds hold; after a SECTION fault the ones BEFORE the record at fault, so an index
 * here is always an entry of the audit's infos): the return value is their number, infos (may be NULL) receives the first
 * min(that, cap).  Host only, bounds only: they verify nothing.  < 0: the container is malformed (-2).
 * groth16_*_beacon[_file] are groth16_*_contribute[_file] in everything else: the lane tests before any arithmetic, cap tested first
 * against a size known before any device work (the contribution's plus 36), the temporary file and the rename, nothing left by a
 * failed call, -2 for a truncated or prepared .ptau or a stale chain, the reports.  There are no fixed_* options.  iter_exp above
 * GROTH16_BEACON_ITER_EXP_MAX, or a null beacon_hash, is -3 before any work.
 * What none of this does: read or write snarkjs' beacon record (its format needs BLAKE2b and hash-to-G2); take numIterationsExp
 * above 24 (snarkjs allows up to 63); exist as a command of the `prove` worker (its -contributions and ptau-verify commands do
 * audit and list beacon records); use more than one GPU. */
#define GROTH16_CONTRIB_BEACON  6   /* a beacon record's iter_exp or the file's beacon work is over the bound, or the record is not the beacon's */
#define GROTH16_BEACON_ITER_EXP_MAX 24
typedef struct {
  uint32_t index;            /* the record, 1 for the first */
  uint8_t  hash[32];         /* beacon_hash as the record holds it */
  uint32_t iter_exp;
} Groth16BeaconInfo;
int groth16_beacon_digest(const uint8_t hash[32], uint32_t iter_exp, uint8_t out[32]);
int groth16_ptau_beacon(const void* ptau, size_t len, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name,
                        void* out, size_t cap, const char* device, Groth16PtauContributeReport* report);
int groth16_ptau_beacon_file(const char* in_path, const char* out_path, const uint8_t beacon_hash[32], uint32_t iter_exp,
                             const char* name, const char* device, Groth16PtauContributeReport* report);
int groth16_zkey_beacon(const void* zkey, size_t len, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name,
                        void* out, size_t cap, const char* device, Groth16ZkeyContributeReport* report);
int groth16_zkey_beacon_file(const char* zkey_path, const char* out_path, const uint8_t beacon_hash[32], uint32_t iter_exp,
                             const char* name, const char* device, Groth16ZkeyContributeReport* report);
int groth16_ptau_beacons(const void* ptau, size_t len, Groth16BeaconInfo* infos, size_t cap);
int groth16_zkey_beacons(const void* zkey, size_t len, Groth16BeaconInfo* infos, size_t cap);

/* groth16_ptau_verify — two questions about one .ptau, UNPREPARED OR PREPARED, answered on the GPU: are sections 2 to 6 the powers of
 * one (tau, alpha, beta), and — when sections 12 to 15 are present — are they the inverse transforms of 2 to 5 that
 * groth16_ptau_prepare and snarkjs write?  What `snarkjs powersoftau verify` shows about the points.  Opt-in.
 * THE CONTAINER: sections 1 to 7 with the unprepared layout's exact element counts (groth16_ptau_prepare states them), and of 12 to 15
 * none or all four, each with exactly the bytes prepare writes; anything else is -2.  A power above 27 is -3.
 * POINTS — A VERDICT, NOT AN ERROR.  Every point of 2 to 5 and 12 to 15 goes through the lane tests of the other key tools
 * (coordinates < q, on the curve, sections 3 and 13 in the subgroup; section 6 on the host).  A point that fails gives 0 with kind
 * POINT and fault_section, fault_index (the lowest faulty element of that section), fault_kind = GROTH16_ZKEY_NONCANONICAL /
 * _OFF_CURVE / _OFF_SUBGROUP.  AN IDENTITY IN SECTIONS 2 TO 6 is a fault of its own, kind IDENTITY (fault_kind 0): tau, alpha, beta
 * are not 0, and e(O, .) = 1 would satisfy every equation below.  Identities in 12 to 15 are legitimate (tau inside a domain).
 * Sections are tested in the order 6, then pair by pair 2, 12, 3, 13, 4, 14, 5, 15, within a section POINT before IDENTITY; the first
 * fault ends the call, no sum has read the faulty section, and failed_mask is 0: it then says nothing about the equations.
 * EQUATIONS ON 2 TO 6, one bit of failed_mask each (bit = kind - 1), all evaluated whatever failed first; kind is the lowest.  N =
 * 2^power, P_i section 2, Q_i section 3, tau1 = P_1, tau2 = Q_1, rho_i = the 128-bit coefficient i of the seed (SHA-256(seed ||
 * LE64(i)), first 16 bytes little-endian, 0 -> 1), one vector for the four sections:
 *   bit 0 GENERATORS  P_0 = G1 and Q_0 = G2, as stored words
 *   bit 1 TAU_PAIR    e(P_1, G2) = e(G1, Q_1)                                              (power >= 1)
 *   bit 2 BETA_PAIR   e(section 5 [0], G2) = e(G1, section 6)
 *   bit 3 TAU_G1      L = sum_{i < 2N-2} rho_i P_i, R = sum rho_i P_(i+1):  e(L, tau2) = e(R, G2)
 *   bit 4 TAU_G2      L = sum_{i < N-1} rho_i Q_i, R = sum rho_i Q_(i+1):   e(tau1, L) = e(G1, R)
 *   bit 5 ALPHA_TAU   as bit 3 over section 4 (N points)
 *   bit 6 BETA_TAU    as bit 3 over section 5
 * Bit 4 needs tau in G1.  While TAU_PAIR holds that is tau1, as written.  When TAU_PAIR fails, tau1 does not stand for tau2, and bit 4
 * is evaluated as e(R', L) = e(L', R) with (L', R') the two sums of the first of sections 2, 4, 5 whose own bit holds — that bit IS
 * R' = tau2 L' — so that a wrong P_1 is named TAU_PAIR + TAU_G1 and not also TAU_G2; when none holds, nothing in the file stands for
 * tau2 in G1 and bit 4 is set.  Every ratio is thereby measured against tau2 = Q_1, as the tests' exact model does.
 * At power 0 bits 1 and 3 to 6 have nothing to sum and hold.  What ties element 0 of sections 4 and 5, and tau1 and tau2, to the
 * contributors is groth16_ptau_contributions' HEADER rule; this call does NOT run that audit (a file written by a model that knows
 * tau has no records).  Run both.
 * EQUATIONS ON 12 TO 15, bits 7 to 10, kinds LAGRANGE_12 to LAGRANGE_15, when the sections are present.  Block p of a section starts
 * at element 2^p - 1 and must be (1/2^p) sum_i w_p^(-ij) S_i over its source S (2 -> 12, 3 -> 13, 4 -> 14, 5 -> 15; section 12's
 * block power + 1 with the identity as its last input).  The library's NTT is not used — its domain is process-wide state of the
 * cache manager — but one full-width MSM on each side with scalars every lane computes for itself:
 *   x     = SHA-256(seed || "icicle-snark ptau verify v1" || LE32(c)) as a big-endian integer mod r, for the first c = 0, 1, ... with
 *           x != 0 and x^(2^(power+1)) != 1;  y = 1/x
 *   mu_p  = the 128-bit coefficient 2^32 + p of the seed, p <= power + 1;  W = w_(power+1);  pmax = power + 1 for 12, power for 13 to 15
 *   left  element e of the prepared section, p = floor(log2(e + 1)), j = e + 1 - 2^p:
 *           lambda_e = mu_p (x^(2^p) - 1) / (x - W^(j 2^(power+1-p)))
 *   right element i of the source, q = the least p with 2^p > i:
 *           d_i = y^(i+1) T[q],  T[q] = sum_{p=q}^{pmax} mu_p x^(2^p)
 *   sum_e lambda_e B_e = sum_{i < min(|S|, 2^pmax)} d_i S_i, compared as points (section 13 in G2).
 * It holds because f(X) = sum_i x^(n-1-i) X^i = (x^n - X^n)/(x - X) has f(w^j) = (x^n - 1)/(x - w^j), and a block that is the inverse
 * transform of S gives sum_j f(w^j) B_j = sum_i x^(n-1-i) S_i.  The mu_p are needed: with equal multipliers an error in one block is
 * cancelled exactly by chosen errors in the next.  ONLY THE FORM PREPARE AND SNARKJS WRITE IS ACCEPTED: a section 12 whose last block
 * is the untruncated L'_j(tau) (a writer that knows tau) fails LAGRANGE_12.
 * SOUNDNESS.  A file that fails an equation in truth is accepted with probability <= 2^-127 per equation of bits 3 to 6 (in rho),
 * and per Lagrange equation <= 2^(power+1)/r per block (in x) plus 2^-127 (in mu) — IF THE SEED IS SECRET AND FRESH: whoever knows the
 * seed before writing the file can make a false file pass.  seed32 = NULL draws it from the operating system; a fixed seed is for
 * tests and reproducible runs.
 * The file is worked through pair by pair — (2, 12), (3, 13), (4, 14), (5, 15): up, lane tests, sums, freed — so no more than one
 * pair is resident.  The _file entry maps the file.  No fixed-base table is built, the NTT domain is not touched, the calling thread's
 * device is what it was afterwards.  ICICLE_SNARK_TRACE_PTAU_VERIFY=1 prints the stage times on stderr.
 * What it does NOT show: WHO CONTRIBUTED (groth16_ptau_contributions' answer, beacon records included: run both); snarkjs' section-7 format; a file
 * truncated by a prefix copy (other counts: -2, or LAGRANGE_12; groth16_ptau_truncate's files have this layout and are judged as
 * any other); more than one GPU; WHICH element of a failing equation is wrong.
 * 1 both questions hold; 0 not (report says what); -1 I/O; -2 a malformed container; -3 argument: power above 27, a device string
 * that does not name one HIP device; -5 device failure (groth16_last_error). */
#define GROTH16_PTAU_VERIFY_GENERATORS  1
#define GROTH16_PTAU_VERIFY_TAU_PAIR    2
#define GROTH16_PTAU_VERIFY_BETA_PAIR   3
#define GROTH16_PTAU_VERIFY_TAU_G1      4
#define GROTH16_PTAU_VERIFY_TAU_G2      5
#define GROTH16_PTAU_VERIFY_ALPHA_TAU   6
#define GROTH16_PTAU_VERIFY_BETA_TAU    7
#define GROTH16_PTAU_VERIFY_LAGRANGE_12 8   /* 9, 10, 11: LAGRANGE_13, _14, _15 */
#define GROTH16_PTAU_VERIFY_LAGRANGE_13 9
#define GROTH16_PTAU_VERIFY_LAGRANGE_14 10
#define GROTH16_PTAU_VERIFY_LAGRANGE_15 11
#define GROTH16_PTAU_VERIFY_POINT       12  /* a point failed its lane test: fault_section, fault_index, fault_kind */
#define GROTH16_PTAU_VERIFY_IDENTITY    13  /* an identity in sections 2 to 6: fault_section, fault_index */
typedef struct {
  uint32_t power;
  int32_t  prepared;            /* 1: sections 12 to 15 are present and were checked */
  int32_t  kind;                /* 0 = both questions hold, else the FIRST failing kind (the lowest bit of failed_mask, or POINT / IDENTITY) */
  uint32_t failed_mask;         /* bit (kind - 1) per failing equation; 0 after POINT / IDENTITY */
  int32_t  fault_section, fault_kind;   /* POINT, IDENTITY: the section; POINT: GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP */
  uint64_t fault_index;                 /* the lowest faulty element of that section */
  uint64_t points[8];           /* points of sections 2, 3, 4, 5, 12, 13, 14, 15 (the last four 0 for an unprepared file) */
  double   upload_ms, device_ms, pairing_ms; /* the sections', coefficients' and tables' copies up; wall time of the device part
                                   without them; the host's pairings and comparisons */
} Groth16PtauVerifyReport;
int groth16_ptau_verify(const void* ptau, size_t len, const uint8_t* seed32 /* NULL = OS randomness */, const char* device,
                        Groth16PtauVerifyReport* report);
int groth16_ptau_verify_file(const char* path, const uint8_t* seed32, const char* device, Groth16PtauVerifyReport* report);

/* groth16_ptau_pack, groth16_ptau_unpack — a powers-of-tau file in HALF THE BYTES and back, on the GPU: every point stored as x and
 * one bit of y, what a ceremony's participants download and upload and its coordinator stores.  groth16_points_pack / _unpack are
 * the same over a plain buffer of points.  Opt-in.
 * THE PACKED POINT.  A point of a .ptau is affine, canonical Montgomery form (R = 2^256), little-endian, the identity all zero.
 *   G1, 32 bytes   x exactly as the file holds it.  q < 2^254, so bits 254 and 255 are free: bit 7 of byte 31 = sign(y), bit 6 of
 *                  byte 31 = the identity flag.  The identity is the flag alone: 00 ... 00 40.
 *   G2, 64 bytes   x as the file holds it, c0 then c1; the same two flag bits in byte 63.  c0 carries no flags.
 *   sign(y) in Fq  = 1 iff the STANDARD-form integer of y is above (q - 1)/2 (not defined on the Montgomery representative);
 *   sign(y) in Fq2 = the sign of y.c1 when y.c1 != 0, else the sign of y.c0.
 * pack and unpack are inverse bijections between sound file-form points and valid packed words, so both directions are functions of
 * their input alone.  UNPACKING a word tests, in this order: the flags (an identity flag with any other bit set, the sign bit
 * included: NONCANONICAL); x < q as an integer (NONCANONICAL); the root of x^3 + 3, on the twist x^3 + 3/xi — none: OFF_CURVE — as
 * a^((q+1)/4) in Fq and by the complex method in Fq2 (two such exponentiations, no inversion), each ending in a squaring that is
 * compared with a, so no path can emit a wrong point; a root of 0 with the sign bit set (NONCANONICAL); then negates to match the sign
 * bit; G2 only, the subgroup test of the other key tools (OFF_SUBGROUP).  The root doubles as the on-curve test.  PACKING runs the
 * lane test of the other key tools first (coordinates < q, on the curve, G2 in the subgroup), so a file packed here always unpacks.
 * The kinds are GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP.
 * THE RAW ENTRIES take n points (64 or 128 bytes each; g2 != 0: G2) or n packed words (32 or 64 bytes) in host memory and write the
 * other form to `out`; n = 0 is valid.  A faulty element is -2 "points: element E: kind" with fault_index the LOWEST faulty element,
 * fault_kind its kind and fault_count how many there are; nothing is written.
 * THE PACKED CONTAINER has the section table of a .ptau under magic "ptaz", version 1: no reader of a .ptau takes it for one (-2,
 * as any foreign magic), and the packed reader takes no .ptau.  Section 1, section 7 and any unknown section are byte for byte the
 * .ptau's, the sections keep their order, and the point sections hold exactly (N = 2^power)
 *   2: (2N - 1) * 32    3: N * 64    4, 5: N * 32    6: 64    and of a prepared file also
 *   12: (4N - 1) * 32   13: (2N - 1) * 64   14, 15: (2N - 1) * 32
 * bytes — of 12 to 15 none or all four; anything else is -2 naming the section and both sizes.  groth16_ptau_pack reads a .ptau in
 * either form as groth16_ptau_verify does (the same container rules, power <= 27).  The host bounds every section before a byte
 * goes up: no content of a file can make a kernel read outside its buffers.
 * Section 6 goes through the same lane code on the host; sections 2 to 5 and 12 to 15 go up and through one launch each, a lane per
 * point.  ALL verdicts are read before anything is written: a faulty point is -2 "ptau: section S, element E: kind" — section 6
 * first, then the lowest faulty section, its lowest faulty element, fault_count that section's faulty elements — and nothing is
 * written.  The output's size is known from the container alone: groth16_ptau_packed_size / groth16_ptau_unpacked_size give it from
 * (power, prepared, the input's bytes) on the host, -3 for a power above 27 or an input shorter than its point sections; cap is
 * tested before any device work (-3, report->out_bytes says what is needed).
 * 0 done; -1 I/O; -2 format or a faulty point; -3 argument: cap too small, equal paths (by name or by inode), a power above 27, a
 * device string that does not name one HIP device; -5 device failure (groth16_last_error).  The _file entries map the input, write a
 * temporary beside out_path and rename it: a failed call leaves nothing.  The calling thread's device is what it was afterwards.
 * ICICLE_SNARK_TRACE_PTAU_PACK=1 prints the stage times on stderr.
 * What it does NOT do: let groth16_ptau_contribute, _verify, _prepare or groth16_zkey_new read a packed file (unpack first; the
 * device side of unpack leaves file-form points in a device buffer, so a later reader needs no host round trip); .zkey files (the
 * raw entries take their points); bellman's or snarkjs' challenge / response formats; more than one GPU; a power above 27; judge the
 * points' RELATIONS (groth16_ptau_verify and groth16_ptau_contributions do, on the unpacked file). */
typedef struct {
  uint64_t n;
  int32_t  fault_kind;          /* after a faulty element: GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP */
  uint64_t fault_index;         /* the lowest faulty element */
  uint64_t fault_count;         /* how many elements are faulty */
  double   upload_ms, device_ms, download_ms;
} Groth16PointsPackReport;
int groth16_points_pack(const void* points, uint64_t n, int g2, void* out, const char* device, Groth16PointsPackReport* report);
int groth16_points_unpack(const void* packed, uint64_t n, int g2, void* out, const char* device, Groth16PointsPackReport* report);
typedef struct {
  uint32_t power;
  int32_t  prepared;            /* 1: sections 12 to 15 are present */
  uint64_t points[2];           /* G1 points, G2 points (section 6 included) */
  uint64_t in_bytes, out_bytes; /* the input; the output (also when cap was too small) */
  int32_t  fault_section, fault_kind;   /* after a faulty point: the section, and GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP */
  uint64_t fault_index;                 /* the lowest faulty element of that section */
  uint64_t fault_count;                 /* that section's faulty elements */
  double   upload_ms, device_ms, download_ms, write_ms; /* the sections' copies up; wall time of the device part without them, up to
                                   the last kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16PtauPackReport;
int groth16_ptau_packed_size(uint32_t power, int prepared, uint64_t ptau_bytes, uint64_t* packed_bytes);
int groth16_ptau_unpacked_size(uint32_t power, int prepared, uint64_t packed_bytes, uint64_t* ptau_bytes);
int groth16_ptau_pack(const void* ptau, size_t len, void* out, size_t cap, const char* device, Groth16PtauPackReport* report);
int groth16_ptau_pack_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPackReport* report);
int groth16_ptau_unpack(const void* packed, size_t len, void* out, size_t cap, const char* device, Groth16PtauPackReport* report);
int groth16_ptau_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPackReport* report);

/* groth16_ptau_truncate — a powers-of-tau file of power P cut down to the file of power p <= P, what `snarkjs powersoftau truncate`
 * is for: a ceremony is run once at a large power and each circuit is served the file of its own.  Opt-in.
 * truncate(F, p) is defined for a .ptau F of power P <= 27, UNPREPARED (sections 1 to 7) or PREPARED (1 to 7 and 12 to 15, the
 * container rules of groth16_ptau_verify), and 0 <= p <= P.  Sections keep F's order; any section this library does not know is
 * copied byte for byte.  With n' = 2^p:
 *   1            power <- p, ceremonyPower unchanged           (p = P: the output is F byte for byte)
 *   2            the first 2n' - 1 points                      3, 4, 5      the first n' points
 *   6, 7         byte for byte
 *   13, 14, 15   the first 2n' - 1 points: blocks 0 to p       12           blocks 0 to p byte for byte, then block p + 1 FIXED UP
 * THE FIX-UP.  Block p + 1 of F's section 12 (p < P) is the full transform of size 2n' — all 2n' powers exist in F — while a file of
 * power p defines it over the zero-extended vector, section 2 holding only 2n' - 1 powers, and groth16_ptau_verify accepts only that
 * form (LAGRANGE_12).  A prefix copy would fail this library's own verifier.  With Q = element 2n' - 1 of F's section 2, the one
 * input the small file no longer holds, and w' the root of order 2n':
 *   B'_j = B_j - (w'^j / 2n') * Q,   j < 2n'        (the scalar of input 2n' - 1 is w'^(-j(2n' - 1)) / 2n' = w'^j / 2n')
 * so that truncate(prepare(U), p) = prepare(truncate(U, p)) BYTE FOR BYTE for every unprepared U.  No fix-up when p = P.
 * ON THE GPU: 2n' lanes, each with a full-width scalar of its own — computed in the lane from two small public tables, lo[i] = w'^i
 * and hi[m] = w'^(m 2^k) / 2n', k = (p + 2) / 2 — times THE SAME point Q.  A common base needs no doublings: the host builds 816
 * signed-window multiples d * 32^w * Q (d = 1 to 16, w < 51; width 5) as affine points, a workgroup of 256 lanes stages them in
 * 52 224 bytes of LDS (three workgroups a CU), and a lane recodes its scalar into 51 signed digits and adds one row per non-zero
 * digit, y negated for a negative one: AT MOST 51 MIXED ADDITIONS A LANE for the product and one for B_j - T, against the 256
 * doublings and 85 additions of the per-lane-base walk.  Exact in every degenerate case: B_j the identity, T = B_j (the all-zero
 * identity), T = -B_j (a doubling), a partial sum that meets a row or its negative.  Q the identity: nothing to subtract, the block
 * is copied and no device is opened.
 * LANE TESTS FIRST: Q (on the host) and every point of block p + 1 (on the device) go through the lane test of the other tools
 * (coordinates < q, on the curve) before any arithmetic: a fault is -2 "ptau: section S, element E: kind" — Q first, then the lowest
 * faulty element of the block, fault_count how many of the block are faulty — and nothing is written.  THE COPIED PREFIXES ARE NOT
 * TESTED: they are the input's bytes, and groth16_ptau_verify judges a file.  Only block p + 1 and the tables go up.  AN UNPREPARED
 * INPUT, OR p = P, NEVER INITIALISES A GPU (the device string is still parsed).
 * THE CHAIN.  h_0 of section 7's chain hashes section 1's payload, which holds `power`.  For a file with power < ceremonyPower —
 * only a truncation makes one — h_0 is computed over the payload with the power field REPLACED BY ceremonyPower: the payload of the
 * file the records were made for.  For power >= ceremonyPower the hashed bytes are what they were.  groth16_ptau_contributions
 * therefore audits a truncated unprepared file with the records and the verdict of the full one: the HEADER rule's elements
 * (element 1 of sections 2 and 3, element 0 of 4 and 5, section 6) survive, and at p = 0 the power-0 rule applies.  It does NOT
 * show that power was not lowered by hand: a file cut by other means with the same bytes IS this file.  groth16_ptau_contribute
 * refuses a file with power < ceremonyPower (-2: contribute to the full file, then truncate), before any device work.
 * groth16_ptau_truncated_size gives the output's size on the host.  cap is tested before any device work (-3, report->out_bytes says
 * what is needed).  0 done; -1 I/O; -2 format (a packed "ptaz" file: the reader's text; unpack first) or a faulty point; -3 argument:
 * power above the file's, cap too small, equal paths (by name or by inode), a device string that does not name one HIP device; -5
 * device failure (groth16_last_error).  The _file entry maps the input, writes a temporary beside out_path and renames it: a failed
 * call leaves nothing.  The calling thread's device is what it was afterwards.  ICICLE_SNARK_TRACE_PTAU_TRUNCATE=1 prints the stage
 * times on stderr.
 * What it does NOT do: read a packed (ptaz) file; RAISE a power; read or write snarkjs' section-7 format; use
 * more than one GPU; test the copied prefixes. */
typedef struct {
  uint32_t power_in, power_out;
  int32_t  prepared;            /* 1: sections 12 to 15 are present */
  uint64_t points_fixed;        /* elements of section 12's block power_out + 1 that went through the fix-up (0: none needed) */
  uint64_t in_bytes, out_bytes; /* the input; the output (also when cap was too small) */
  int32_t  fault_section, fault_kind;   /* after a faulty point: 2 or 12, and GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE */
  uint64_t fault_index;                 /* the lowest faulty element of that section */
  uint64_t fault_count;                 /* the block's faulty elements (1 for Q) */
  double   upload_ms, device_ms, download_ms, write_ms; /* the block's and the tables' copies up; wall time of the device part
                                   without them and without the host's copy of the container, which runs beside the kernels: what
                                   the device adds to the call; the block's copy down; msync and rename (_file) */
} Groth16PtauTruncateReport;
int groth16_ptau_truncated_size(const void* ptau, size_t len, uint32_t power, uint64_t* bytes);
int groth16_ptau_truncate(const void* ptau, size_t len, uint32_t power, void* out, size_t cap, const char* device,
                          Groth16PtauTruncateReport* report);
int groth16_ptau_truncate_file(const char* in_path, const char* out_path, uint32_t power, const char* device,
                               Groth16PtauTruncateReport* report);

/* groth16_wtns_pack, groth16_wtns_unpack, groth16_prove_packed, groth16_witness_check_packed — a witness with a code byte per value
 * and only the value's significant bytes ("wtnz"), packed on the host of the witness generator and decoded on the GPU straight into
 * the place the prove reads it from.  A witness is the one file a proving service moves per proof, and most of its 32 bytes a wire
 * are zero: a bit wire costs 1 byte, a full-width value 33.  Opt-in: nothing that takes a .wtns takes this, and the reverse.
 * THE VALUE.  v in standard form, 0 <= v < r, as a .wtns holds it; bytes(x) = the significant bytes of x, bytes(0) = 0.  The first
 * rule that applies:   v = 0: code 0x00, no payload   |   v = 1: code 0x40, no payload   |   m = r - v with bytes(m) < bytes(v): code
 * 0x80 | bytes(m) (0x81 ... 0x9f), payload m in bytes(m) little-endian bytes   |   else code bytes(v) (0x01 ... 0x20), payload v in
 * bytes(v) little-endian bytes.  Every other code byte is undefined.  The encoding is unique: pack and unpack are inverse bijections
 * and both are functions of their input alone.
 * THE CONTAINER is an iden3 section table under magic "wtnz", version 1, each section once, in any order (pack writes 1, 2, 3, 4):
 *   1  a .wtns header byte for byte: n8 = 32, q (= r of BN254, 32 bytes), n_witness (u32) — 40 bytes
 *   2  the codes, one byte per value: n_witness bytes
 *   3  the directory: ceil(n_witness / 256) + 1 little-endian u64; entry b = the offset in section 4 where the payload of block b
 *      (values 256 b ... 256 b + 255) begins; entry 0 is 0, the last entry is section 4's size
 *   4  the payload: the values' significant bytes in order
 * THE HOST bounds everything before a byte goes up: the section sizes against n_witness; the directory beginning at 0, never
 * decreasing, ending at section 4's size, no block spanning more than 256 * 32 = 8192 bytes (-2, each with a text of its own).  No
 * content of a file can then make the kernel read outside its buffers.
 * A DECODER refuses a value with one of the kinds below (-2 "wtnz: element E: kind"): fault_index is the LOWEST faulty element,
 * fault_kind its kind, fault_count how many there are, and nothing is written. */
#define GROTH16_WTNZ_CODE         1   /* an undefined code byte */
#define GROTH16_WTNZ_NONCANONICAL 2   /* a payload whose top byte is 0; code 0x01 with payload 01; a 32-byte positive form whose negated form is shorter */
#define GROTH16_WTNZ_RANGE        3   /* 32 bytes that are not below r */
#define GROTH16_WTNZ_DIRECTORY    4   /* a block's 256 lengths (an undefined code counts 0) do not sum to its directory span: named at the
                                         block's first element, and the only fault such a block reports */
typedef struct {
  uint32_t n_witness;
  uint64_t in_bytes, out_bytes;  /* the input; the output (also when cap was too small) */
  int32_t  fault_kind;           /* GROTH16_WTNZ_*; pack: GROTH16_WTNZ_RANGE for a .wtns value >= r */
  uint64_t fault_index;          /* the lowest faulty element */
  uint64_t fault_count;          /* how many elements are faulty */
  double   upload_ms, kernel_ms, device_ms, download_ms, write_ms; /* groth16_wtns_unpack: sections 2 to 4 up; the decode kernel alone
                                    (events); wall time of the device part without the upload; the values down; msync and rename (_file) */
} Groth16WtnsPackReport;
/* HOST ONLY — the five entries below never initialise a GPU: the witness generator's host has none.
 * groth16_wtns_packed_size: the bytes of the packed form of a .wtns image.  groth16_wtns_pack: a .wtns (as every .wtns reader here
 * takes it) to its packed form; a value >= r is -2 "wtns: element E is not below r" with report->fault_index = E.
 * groth16_wtns_unpack_host: the .wtns a packed witness came from, byte for byte when the .wtns had nothing but its sections 1 and 2;
 * faults as above.  cap is tested before anything is written (-3, report->out_bytes says what is needed).  The _file entries map the
 * input, write a temporary beside out_path and rename it: a failed call leaves nothing.
 * What they do NOT do: keep a .wtns' other sections or its version (the output is version 2, sections 1 and 2); check the witness
 * against a circuit; compress (a dense witness GROWS by one byte a value and the directory). */
int groth16_wtns_packed_size(const void* wtns, size_t len, uint64_t* packed_bytes);
int groth16_wtns_pack(const void* wtns, size_t len, void* out, size_t cap, Groth16WtnsPackReport* report);
int groth16_wtns_pack_file(const char* in_path, const char* out_path, Groth16WtnsPackReport* report);
int groth16_wtns_unpack_host(const void* packed, size_t len, void* out, size_t cap, Groth16WtnsPackReport* report);
int groth16_wtns_unpack_host_file(const char* in_path, const char* out_path, Groth16WtnsPackReport* report);
/* groth16_wtns_unpack — the same on one HIP device: sections 2 to 4 go up, ONE launch decodes them — a 256-lane workgroup per block,
 * a lane per value — and the values come down.  All verdicts are read before anything is written.  -3 also for a device string that
 * does not name one HIP device, -5 a device failure.  The calling thread's device is what it was afterwards.
 * What it does NOT do: pack on the GPU; keep anything resident (groth16_prove_packed does). */
int groth16_wtns_unpack(const void* packed, size_t len, void* out, size_t cap, const char* device, Groth16WtnsPackReport* report);
int groth16_wtns_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16WtnsPackReport* report);
/* groth16_prove_packed — groth16_prove_mem from a packed witness: groth16_prove_mem's two tests of a witness with their messages
 * (curve, length), sections 2 to 4 up, the decode into the key's resident witness buffer on the key's stream, and on a clean tally
 * the resident prove (groth16_prove_resident's path) — decode and commitments under one hold of the manager's mutex, so no other
 * thread's prove lands between them.  The public signals are decoded on the host from the first n_public + 1 values.  Afterwards the
 * witness is resident as after groth16_prove_mem.  On a fault (-2, as above) NO witness is resident and nothing is proved.
 * -1 ... -5 as groth16_prove_mem.  What it does NOT do: device groups and shards (-3 with a message: single-device keys only);
 * overlap the upload with the head of the prove as groth16_prove_mem does for large witnesses; pack on the GPU. */
int groth16_prove_packed(Groth16CacheManager* cm, const char* key, const void* wtnz, size_t len, const uint8_t* r, const uint8_t* s,
                         char* proof_json, size_t proof_cap, char* public_json, size_t public_cap, Groth16Timings* timings);
/* groth16_prove_packed_files — groth16_prove with a packed witness, file to file, the cache key "<zkey_path>_<device>" as there.  A
 * key the manager does not hold is loaded through groth16_cache_load_file first.  What it does NOT do: groth16_prove's cold-path
 * overlap — the key's upload and the first proof run one after the other; more than one device (-3). */
int groth16_prove_packed_files(const char* witness_path, const char* zkey_path, const char* proof_path, const char* public_path,
                               const char* device, Groth16CacheManager* cm);
/* groth16_witness_check_packed — groth16_witness_check with the decode in front, on the handle's device: verdict and report are those
 * of the unpacked witness (upload_ms is the packed sections').  A faulty packed witness is -2 as above: no verdict.
 * What it does NOT do: anything groth16_witness_check does not. */
int groth16_witness_check_packed(Groth16R1cs* h, const void* wtnz, size_t len, Groth16WitnessReport* report);
int groth16_witness_check_packed_file(Groth16R1cs* h, const char* wtnz_path, Groth16WitnessReport* report);

/* groth16_zkey_pack, groth16_zkey_unpack, groth16_cache_load_packed, groth16_prove_zkez_files — a proving key PACKED ("zkez") and
 * back, and a load that takes the packed key and never holds the unpacked one on the host.  The .zkey is the largest file that
 * reaches a prover: its points are stored as x and one bit of y (the packed point of groth16_ptau_pack above, unchanged: half the
 * bytes), its coefficients as a code byte and the significant bytes of the value (the value code of groth16_wtns_pack above,
 * unchanged).  Opt-in: nothing that takes a .zkey takes this, and the reverse.
 * THE CODED VALUE.  Section 4 of a .zkey holds a coefficient as file_value = v * R^2 mod r, R = 2^256.  The value coded is the
 * standard-form coefficient v = file_value * R^-2 mod r — in a real key almost always 1 or r - 1, one code byte or two.  Packing
 * demands file_value < r (a value not below r is the fault RANGE); v -> v * R^2 mod r is a bijection on [0, r) and the value code is
 * one between [0, r) and its valid (code, payload) pairs, so pack and unpack are inverse byte for byte and both are functions of
 * their input alone.
 * THE CONTAINER is the .zkey's section table under magic "zkez", version 1, the sections in the input's order: no reader of a .zkey
 * takes it for one (-2, as any foreign magic), and the packed reader takes no .zkey.
 *   1, 2, 10 and any unknown section   byte for byte the .zkey's (the header and its six points are NOT packed)
 *   3, 5, 6, 8, 9 (G1), 7 (G2)         exactly half the bytes: each point its packed word, the identity 00 ... 00 40
 *   4   u32 declared_count (the .zkey's first four bytes, verbatim; no loader reads it) | u32 n_coef | u64 payload_bytes |
 *       n_coef * 12 bytes, the {m, c, s} triples as they stand | n_coef code bytes | the directory, ceil(n_coef / 256) + 1
 *       little-endian u64: entry b = where the payload of block b (coefficients 256 b ... 256 b + 255) begins, entry 0 = 0, the last
 *       entry = payload_bytes | the payload: the values' significant bytes in order
 * THE HOST bounds everything before a byte goes up: sections 1 and 2 by the rules of every .zkey reader here; every point section's
 * exact packed size (-2 naming the section and both sizes); section 4's size against the sum of its parts; the directory beginning at
 * 0, never decreasing, no block spanning more than 8192 bytes, ending at payload_bytes (-2, each with a text of its own).  No content
 * of a file can then make a kernel read outside its buffers.  groth16_zkey_pack reads the key as groth16_zkey_check does (section 3
 * included): a key that reader refuses is refused with its message.
 * THE DEVICE runs one launch per point section — packing behind the lane test of the other key tools (section 7 with the subgroup
 * test), so a file packed here always unpacks; unpacking through the full test of groth16_ptau_unpack, section 7's subgroup test
 * included — and for section 4 two kernels to pack (code and block sums; then, behind the host's directory, the payload) and one to
 * unpack, a 256-lane workgroup per block.
 * FAULTS are -2 and name the lowest faulty section, then its lowest faulty element; fault_count is that section's; nothing is written
 * and nothing is cached:
 *   "zkez: section S, element E: <point kind>"   GROTH16_ZKEY_NONCANONICAL / _OFF_CURVE / _OFF_SUBGROUP
 *   "zkez: coefficient E: <kind>"                fault_section = 4 and GROTH16_WTNZ_CODE / _NONCANONICAL / _RANGE / _DIRECTORY
 *   packing: "zkey: section S, element E: <point kind>" and "zkey: coefficient E: not below r" (GROTH16_WTNZ_RANGE)
 * SIZES.  groth16_zkey_unpacked_size is exact from the packed container; groth16_zkey_packed_bound is the upper bound from the .zkey's
 * container, every value at 32 bytes; both run the reader's tests and need no GPU.  The packed size itself is known only after the
 * first coefficient kernel: the buffer entry tests cap then (-3, report->out_bytes says what is needed).
 * 0 done; -1 I/O; -2 format or a fault; -3 argument: cap too small, equal paths (by name or by inode), a device string that does not
 * name one HIP device; -5 device failure.  The _file entries map the input, write a temporary beside out_path and rename it: a
 * failed call leaves nothing.  ICICLE_SNARK_TRACE_ZKEY_PACK=1 prints the stage times on stderr.
 * What it does NOT do: compress the {m, c, s} triples; pack section 2 or section 10; let groth16_zkey_check, _verify_ptau,
 * _contribute, groth16_r1cs_match_zkey, groth16_cache_load or groth16_prove read a packed key (unpack first, or load it packed);
 * overlap the packed load with a first proof; skip section 7's subgroup test on load; serve shards or device groups. */
typedef struct {
  uint32_t n_vars, n_public, domain, n_coef;
  uint64_t points[2];             /* G1 points, G2 points of sections 3 and 5 to 9 */
  uint64_t in_bytes, out_bytes;   /* the input; the output (also when cap was too small) */
  uint64_t point_bytes, coef_bytes; /* of the PACKED form: the point sections; section 4 */
  int32_t  fault_section, fault_kind; /* the section; a point's GROTH16_ZKEY_*, in section 4 GROTH16_WTNZ_* */
  uint64_t fault_index;           /* the lowest faulty element of that section */
  uint64_t fault_count;           /* that section's faulty elements */
  double   upload_ms, device_ms, download_ms, write_ms; /* the sections' copies up; wall time of the device part without them, up to
                                     the last kernel; the copies into the buffer or the mapped file; msync and rename (_file) */
} Groth16ZkeyPackReport;
int groth16_zkey_unpacked_size(const void* zkez, size_t len, uint64_t* zkey_bytes);
int groth16_zkey_packed_bound(const void* zkey, size_t len, uint64_t* packed_bytes);
int groth16_zkey_pack(const void* zkey, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyPackReport* report);
int groth16_zkey_pack_file(const char* in_path, const char* out_path, const char* device, Groth16ZkeyPackReport* report);
int groth16_zkey_unpack(const void* zkez, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyPackReport* report);
int groth16_zkey_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16ZkeyPackReport* report);
/* THE RAW CODEC, as groth16_points_pack is to the point sections: n records of 44 bytes {m, c, s, value} in host memory to the body
 * of a packed section 4 (declared_count = n) and back; n = 0 is valid (a body of 24 bytes).  pack: cap is tested once the size is
 * known (-3, out_bytes says what is needed; zkez bound: 24 + 45 n + 8 ceil(n / 256) bytes); unpack: the body passes the reader's
 * tests of section 4 first and `out` takes n * 44 bytes.  Faults as above, "zkey: coefficient E: not below r" / "zkez: coefficient
 * E: <kind>"; nothing is written. */
typedef struct {
  uint64_t n;
  uint64_t in_bytes, out_bytes;
  int32_t  fault_kind;          /* GROTH16_WTNZ_* */
  uint64_t fault_index;         /* the lowest faulty coefficient */
  uint64_t fault_count;         /* how many are faulty */
  double   upload_ms, device_ms, download_ms;
} Groth16ZkeyCoefsReport;
int groth16_zkey_coefs_pack(const void* records, uint64_t n, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* report);
int groth16_zkey_coefs_unpack(const void* body, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* report);
/* groth16_cache_load_packed — groth16_cache_load from a packed key, on ONE device: the packed point sections and section 4 go up, the
 * unpack kernels write file-form points and records straight into the buffers the loader has always filled, every verdict is read,
 * and the rest of the load — the CSR build, the bases' conversion, the deferred tables — runs unchanged on what it has always been
 * given.  The entry is the one groth16_cache_load of the unpacked key builds; the budget is charged the UNPACKED size.  A fault is
 * -2 as above and nothing is cached.  A key the manager already holds under `key` is 0 at once.  Warm, this load is SLOWER than
 * groth16_cache_load_file of the same key (the roots cost more than the halved upload saves; README has the figures): what the
 * format buys is bytes stored and moved.  The arguments are groth16_cache_load's; anything but shard 0 of 1 is -3 with a message.
 * What it does NOT do: shards and device groups; overlap with a first proof. */
int groth16_cache_load_packed(Groth16CacheManager* cm, const char* key, const void* zkez, size_t len, int device_id, int shard_rank,
                              int shard_count);
int groth16_cache_load_packed_file(Groth16CacheManager* cm, const char* key, const char* zkez_path, int device_id, int shard_rank,
                                   int shard_count);
/* groth16_prove_zkez_files — groth16_prove with a packed key, file to file, the cache key "<zkez_path>_<device>".  A key the manager
 * does not hold is loaded through groth16_cache_load_packed_file first; then groth16_prove_mem's path runs.  What it does NOT do:
 * groth16_prove's cold-path overlap; more than one device (-3). */
int groth16_prove_zkez_files(const char* witness_path, const char* zkez_path, const char* proof_path, const char* public_path,
                             const char* device, Groth16CacheManager* cm);

#ifdef __cplusplus
}
#endif
#endif
