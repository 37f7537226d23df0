// ptau_contribute.hip — groth16_ptau_new: the starting file of a powers-of-tau ceremony; groth16_ptau_contribute: one participant's
// secrets (τ′, α′, β′) applied to every point of an unprepared file; groth16_ptau_contributions: the host's audit of the chain section
// 7 records.  include/groth16_prover.h has the contract and section 7's layout; DESIGN.md §7h.  groth16_ptau_beacon is the same call
// with the secret replaced by the beacon's public digest and the record's tail added (§7o): no stage of it is written twice.
//
//   host, first  the container (ptau_unprepared_layout), section 7's bounds and its last record against the file, the output's size
//                against the room, section 6 through the lane test; τ′, α′, β′ and the three nonces (transcript.h has the hashes, the
//                record walk and the proof of knowledge, one text with groth16_zkey_contribute's); the tables lo[j] = τ′^j and
//                hi_c[m] = c·τ′^(m·2^k) for c ∈ {1, α′, β′} (device_call.h's split_power_tables over ptau_contribute29.h), Montgomery
//                form, on the worker pool.
//   device       sections 2 … 5 go up and stay; each through ptau_ranges.h's lane test (section 3 with the subgroup test), and all four
//                verdicts are read before any arithmetic sees a point.  Then per section ONE launch of pc_scale_kernel, a lane per
//                point: s = from_mont(hi_c[i ≫ k]·lo[i mod 2^k]) = c·τ′^i, its non-adjacent form, pp29::pp_scale's walk — a full-width
//                scalar per lane that no table of 2N entries holds.  point_form.h's to_file_form writes the section back over its
//                source in the file's form, the identity all zero.
//   host, beside the record — eight G1 and two G2 multiplications by zc_mul_affine, on points the verdicts have passed — section 6 and
//                the sections that are copied, while the kernels run.  Nothing is written before the verdicts are in.
//   The device tables are overwritten before they are freed, the host's secrets wiped on every way out: best effort.
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "point_form.h"
#include "prover_internal.h"
#include "ptau_contribute29.h"
#include "ptau_ranges.h"
#include "transcript.h"
#include "verify_batch.h"

using namespace bn254;
using namespace isnark::transcript;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;
using pv::Group;

constexpr int PC_WG = 64;
const char TAG[] = "icicle-snark ptau contribution v1";
constexpr size_t TAG_LEN = sizeof TAG - 1;
constexpr uint32_t NEW_POWER_MAX = 27; // groth16_ptau_prepare's limit
// a record: the five `after` points, the three commitments, the three responses, the name
constexpr size_t TAU1 = 0, ALPHA1 = 64, BETA1 = 128, TAU2 = 192, BETA2 = 320, AFTER_BYTES = 448, R_TAU = 448, Z_TAU = 640, NAME_LEN = 736, RECORD_FIXED = 740;
constexpr size_t BEFORE_BYTES = 192; // (tau1, alpha1, beta1): the first three points of a record

// One lane per point of a section (pts[i], i < n): (c·τ′^i)·P as Montgomery projective, the identity (0, 1, 0).  lo[j] = τ′^j for
// j < 2^k and hi[m] = c·τ′^(m·2^k) for m ≤ (n − 1) ≫ k, Montgomery form: the host sizes hi for 2^(power+1) indices, n is at most
// 2^(power+1) − 1.  The points have passed their lane test.
template <class C>
__global__ __launch_bounds__(PC_WG) void pc_scale_kernel(const typename C::A* __restrict__ pts, uint64_t n, const fe* __restrict__ lo, const fe* __restrict__ hi, uint32_t k,
                                                         typename C::P* __restrict__ out)
{
  typedef CurveL<typename Group<C>::F> CL;
  const uint64_t i = (uint64_t)blockIdx.x * PC_WG + threadIdx.x;
  if (i >= n) return;
  const typename C::A p = pts[i];
  out[i] = C::x_to_projective(CL::x_store(pc29::pc_lane<typename Group<C>::F>(p, ld(hi + (i >> k)), ld(lo + (i & (((uint64_t)1 << k) - 1))))));
}

// ---- section 7 (the scalars, the record walk and the proof of knowledge are transcript.h's)
// h₀: what no contribution changes.  A file with power < ceremonyPower (groth16_ptau_truncate's) hashes section 1 as the file the
// records were made for held it: the power field replaced by ceremonyPower.  Every other file hashes its own bytes.
void chain_start(const pv::PtauLayout& L, uint8_t h[32])
{
  std::vector<uint8_t> m;
  append(m, TAG, TAG_LEN);
  append(m, L.sec[1]->p, (size_t)L.sec[1]->size);
  if (L.power < L.ceremony_power) memcpy(m.data() + TAG_LEN + 36, &L.ceremony_power, 4); // (ptau_header: the payload has 44 bytes)
  isnark::sha256(m.data(), m.size(), h);
}
// e_i = SHA-256(h_{i−1} ‖ before ‖ the five after points ‖ R_tau ‖ R_alpha ‖ R_beta ‖ name_len as stored ‖ name ‖ a beacon's trailer)
// → h (in place); c: its first 16 bytes, little-endian, 0 → 1.  The responses are not hashed.
void chain_step(uint8_t h[32], const uint8_t* before, const Record& r, fe* c)
{
  std::vector<uint8_t> m;
  append(m, h, 32);
  append(m, before, BEFORE_BYTES);
  append(m, r.p, Z_TAU);
  append(m, r.p + NAME_LEN, hashed_tail(r));
  hash_step(m, h, c);
}

// the five points a record must end in, as the file holds them now: [τ]₁ [α]₁ [β]₁ [τ]₂ [β]₂ in a record's order.  At power 0 the
// file holds no power of τ: have_tau is false and the two τ entries are left alone.
struct Held {
  uint8_t b[AFTER_BYTES];
  bool have_tau;
};
Held held_points(const pv::PtauLayout& L)
{
  Held h;
  memset(h.b, 0, sizeof h.b);
  h.have_tau = L.power >= 1;
  if (h.have_tau) {
    memcpy(h.b + TAU1, L.sec[2]->p + 64, 64);
    memcpy(h.b + TAU2, L.sec[3]->p + 128, 128);
  }
  memcpy(h.b + ALPHA1, L.sec[4]->p, 64);
  memcpy(h.b + BETA1, L.sec[5]->p, 64);
  memcpy(h.b + BETA2, L.sec[6]->p, 128);
  return h;
}
// the HEADER rule: `after` (a record's first 448 bytes, or the generators) against the file
bool header_holds(const Held& f, const uint8_t* after)
{
  if (f.have_tau && (memcmp(after + TAU1, f.b + TAU1, 64) != 0 || memcmp(after + TAU2, f.b + TAU2, 128) != 0)) return false;
  return memcmp(after + ALPHA1, f.b + ALPHA1, 64) == 0 && memcmp(after + BETA1, f.b + BETA1, 64) == 0 && memcmp(after + BETA2, f.b + BETA2, 128) == 0;
}
// (G₁, G₁, G₁, G₂, G₂): record 0
void generators(uint8_t out[AFTER_BYTES])
{
  const G1::A g1 = vb::g1_generator_mont();
  const G2::A g2 = vb::g2_generator_mont();
  for (size_t off : {TAU1, ALPHA1, BETA1}) memcpy(out + off, &g1, 64);
  for (size_t off : {TAU2, BETA2}) memcpy(out + off, &g2, 128);
}

// x′ = W(seed ‖ TAG ‖ label) → *x, standard form, for `which` = 0, 1, 2 (τ, α, β: labels 1, 2, 3); false when it is zero
bool derive_secret(const uint8_t seed[32], int which, fe* x)
{
  const uint8_t label = (uint8_t)(which + 1);
  std::vector<uint8_t> m;
  append(m, seed, 32);
  append(m, TAG, TAG_LEN);
  append(m, &label, 1);
  *x = wide_hash(m);
  return !Fr::is_zero(*x);
}
// BEACON's last question (transcript.h's beacon_work_allowed has passed): with the digest and τ′, α′, β′ recomputed, is
// after.x1 = x′·before.x1 in the file's canonical affine bytes for tau1, alpha1, beta1?
bool record_is_the_beacons(const Record& r, const uint8_t* before)
{
  uint8_t digest[32];
  beacon_digest(r.trailer, beacon_iter_exp(r), digest);
  for (int x = 0; x < 3; x++) {
    fe s;
    if (!derive_secret(digest, x, &s)) return false;
    const G1::A want = zc29::zc_mul_affine<G1, G1L>(point_at<G1::A>(before + 64 * x), s);
    if (memcmp(&want, r.p + 64 * x, 64) != 0) return false;
  }
  return true;
}

// everything secret of one call; wiped on every way out (best effort: the compiler may have kept copies in registers or spills)
struct Secrets {
  uint8_t seed[32];
  fe x[3], k[3];          // τ′, α′, β′ and their nonces, standard form
  std::vector<fe> tables; // lo ‖ hi_1 ‖ hi_α′ ‖ hi_β′, Montgomery form
  ~Secrets()
  {
    if (!tables.empty()) explicit_bzero(tables.data(), tables.size() * sizeof(fe));
    explicit_bzero(seed, sizeof seed);
    explicit_bzero(x, sizeof x);
    explicit_bzero(k, sizeof k);
  }
};
// the device's copy of the tables: overwritten on every way out, before the session frees it
struct TableWipe {
  fe* d = nullptr;
  size_t bytes = 0;
  hipStream_t st = nullptr;
  ~TableWipe()
  {
    if (d && hipMemsetAsync(d, 0, bytes, st) == hipSuccess) (void)hipStreamSynchronize(st);
  }
};

using pv::Sink;
using pv::TempOutput;

// ---- groth16_ptau_new
int new_size(uint32_t power, uint64_t* bytes)
{
  if (power > NEW_POWER_MAX) return pv::fail(pv::ERR_ARG, "ptau: power %u is above %u, the highest groth16_ptau_prepare takes", power, NEW_POWER_MAX);
  const uint64_t N = (uint64_t)1 << power;
  *bytes = 12 + (12 + 44) + (12 + (2 * N - 1) * 64) + (12 + N * 128) + 2 * (12 + N * 64) + (12 + 128) + (12 + 4);
  return 0;
}
void new_write(uint32_t power, uint8_t* w)
{
  const uint64_t N = (uint64_t)1 << power;
  const G1::A g1 = vb::g1_generator_mont();
  const G2::A g2 = vb::g2_generator_mont();
  auto section = [&](uint32_t id, uint64_t size) { pv::put_section(w, id, size); };
  // count copies of one point from w on, on the worker pool
  auto fill = [&](const void* pt, size_t elem, uint64_t count) {
    uint8_t* const base = w;
    isnark::run_ranges((size_t)count, 1 << 16, [&](int, size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; i++) memcpy(base + i * elem, pt, elem);
    });
    w += count * elem;
  };
  const uint32_t n8 = 32, zero = 0;
  pv::put_container_head(w, "ptau", 1, 7);
  section(1, 44);
  const fe q = Fq::modulus();
  memcpy(w, &n8, 4);
  memcpy(w + 4, q.l, 32);
  memcpy(w + 36, &power, 4);
  memcpy(w + 40, &power, 4);
  w += 44;
  section(2, (2 * N - 1) * 64);
  fill(&g1, 64, 2 * N - 1);
  section(3, N * 128);
  fill(&g2, 128, N);
  for (uint32_t id : {4u, 5u}) {
    section(id, N * 64);
    fill(&g1, 64, N);
  }
  section(6, 128);
  fill(&g2, 128, 1);
  section(7, 4);
  memcpy(w, &zero, 4);
}

// ---- groth16_ptau_contribute
struct Buffers {
  uint8_t* sec[4] = {nullptr, nullptr, nullptr, nullptr}; // sections 2 … 5: the source, then the result in the file's form
  uint8_t *proj = nullptr, *scratch = nullptr;
  fe* tables = nullptr;
  unsigned long long* first = nullptr; // [4]
};

template <class C>
int scale_section(hipStream_t st, const Buffers& b, int k4, uint64_t n, const fe* d_lo, const fe* d_hi, uint32_t kbits)
{
  typedef typename C::A A;
  typedef typename C::P P;
  A* const d_a = (A*)b.sec[k4];
  P* const d_p = (P*)b.proj;
  DEV_LAUNCH("scale kernel launch", (pc_scale_kernel<C>), dim3((uint32_t)((n + PC_WG - 1) / PC_WG)), dim3(PC_WG), st, (const A*)d_a, n, d_lo, d_hi, kbits, d_p);
  return pv::to_file_form<C>(st, d_p, n, d_a, (typename Group<C>::Fo::T*)b.scratch);
}

// beacon: null for a participant's contribution; else secret32 is not read — the secret is the beacon's digest — and opt is null
int contribute_impl(const uint8_t* data, size_t len, const uint8_t* secret32, const char* name, const char* device, const Groth16PtauContributeOptions* opt,
                    Groth16PtauContributeReport* rep, const Sink& sink, const Beacon* beacon = nullptr)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (beacon && !beacon->hash) return pv::fail(pv::ERR_ARG, "null beacon hash");
  if (beacon && beacon->iter_exp > BEACON_ITER_EXP_MAX) return pv::fail(pv::ERR_ARG, "beacon: iter_exp %u is above %u", beacon->iter_exp, BEACON_ITER_EXP_MAX);
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  if (!name) name = "";
  const size_t name_len = strlen(name);
  if (name_len > NAME_BYTES_MAX) return pv::fail(pv::ERR_ARG, "the contributor's name has %zu bytes, a record holds %u", name_len, NAME_BYTES_MAX);
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  if (int rc = pv::ptau_unprepared_layout(data, len, secs, &L)) return rc;
  const uint32_t power = L.power;
  if (power < L.ceremony_power)
    return pv::fail(pv::ERR_FORMAT, "ptau: power %u is below the ceremony's %u: the file is a truncation; contribute to the full file, then truncate", power, L.ceremony_power);
  const uint64_t N = (uint64_t)1 << power;
  const uint64_t counts[4] = {2 * N - 1, N, N, N};
  std::vector<Record> recs;
  uint32_t count, bad;
  if (walk_records(L.sec[7], RECORD_FIXED, NAME_LEN, recs, &count, &bad)) return pv::fail(pv::ERR_FORMAT, "ptau: section 7 is malformed at record %u of %u", bad, count);
  const Held held = held_points(L);
  if (count && !header_holds(held, recs.back().p)) return pv::fail(pv::ERR_FORMAT, "ptau: section 7's last record is not what sections 2 to 6 hold");

  // the output's size, before anything else is done
  const uint64_t rec_bytes = RECORD_FIXED + tail_bytes(name_len, beacon), total = (uint64_t)len + rec_bytes;
  rep->contribution = count + 1;
  rep->power = power;
  for (int k4 = 0; k4 < 4; k4++) rep->points[k4] = counts[k4];
  rep->ptau_bytes = total;
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;
  auto fault = [&](int section, uint64_t element, int kind) {
    pv::set_point_fault(rep, section, element, kind);
    return pv::ptau_point_fail(section, element, kind);
  };
  const G2::A beta2_in = point_at<G2::A>(L.sec[6]->p);
  if (const int kind = classify(beta2_in)) return fault(6, 0, kind);

  // what the record starts from.  before: (tau1, alpha1, beta1) of the last record, or the generators; cur: what x′ multiplies — the
  // file's points, which the HEADER rule has just tied to the last record where the file has them
  uint8_t gens[AFTER_BYTES], cur[AFTER_BYTES];
  generators(gens);
  const uint8_t* const before = count ? recs.back().p : gens;
  memcpy(cur, before, AFTER_BYTES);
  if (held.have_tau) memcpy(cur + TAU1, held.b + TAU1, 64), memcpy(cur + TAU2, held.b + TAU2, 128);
  memcpy(cur + ALPHA1, held.b + ALPHA1, 64);
  memcpy(cur + BETA1, held.b + BETA1, 64);
  memcpy(cur + BETA2, held.b + BETA2, 128);
  // (power 0 behind earlier records: their τ points are the only ones no section holds, so no lane test below sees them)
  if (!held.have_tau && count && (classify(point_at<G1::A>(cur + TAU1)) || classify(point_at<G2::A>(cur + TAU2))))
    return pv::fail(pv::ERR_FORMAT, "ptau: section 7's last record holds a tau point that is not on its curve or in its subgroup");

  // ---- τ′, α′, β′, the nonces
  Secrets S;
  uint8_t digest[32];
  if (beacon) beacon_digest(beacon->hash, beacon->iter_exp, digest), secret32 = digest; // (public: nothing of it needs wiping)
  if (int rc = pv::seed_or_random(secret32, S.seed)) return rc;
  static const char* const NAMES[3] = {"tau", "alpha", "beta"};
  const uint8_t* const fixed[3] = {opt ? opt->fixed_tau : nullptr, opt ? opt->fixed_alpha : nullptr, opt ? opt->fixed_beta : nullptr};
  for (int x = 0; x < 3; x++) {
    if (fixed[x]) {
      memcpy(S.x[x].l, fixed[x], 32);
      if (!Fr::is_canonical(S.x[x]) || Fr::is_zero(S.x[x])) return pv::fail(pv::ERR_ARG, "fixed_%s is not in [1, r)", NAMES[x]);
    } else if (!derive_secret(S.seed, x, &S.x[x])) {
      return pv::fail(pv::ERR_ARG, "the secret gives %s' = 0", NAMES[x]);
    }
  }
  // h_{i−1} over the records there are, as groth16_ptau_contributions hashes them
  uint8_t h[32];
  chain_start(L, h);
  for (uint32_t i = 0; i < count; i++) {
    fe c;
    chain_step(h, i ? recs[i - 1].p : gens, recs[i], &c);
  }
  for (int x = 0; x < 3; x++) {
    const uint8_t label = (uint8_t)(x + 1);
    std::vector<uint8_t> m;
    append(m, S.seed, 32);
    append(m, S.x[x].l, 32);
    append(m, h, 32);
    append(m, before + 64 * x, 64);
    append(m, &label, 1);
    S.k[x] = wide_hash(m);
    if (Fr::is_zero(S.k[x])) return pv::fail(pv::ERR_ARG, "the secret gives the nonce 0");
  }

  pv::StageTrace trace("ptau-contribute", "ICICLE_SNARK_TRACE_PTAU_CONTRIBUTE");
  // ---- the tables: lo[j] = τ′^j, j < 2^k; hi_c[m] = c·τ′^(m·2^k), m < 2^(power+1−k): every index below 2^(power+1) has its two entries
  const uint32_t kbits = pc29::pc_table_bits(power);
  const size_t n_lo = (size_t)1 << kbits, n_hi = (size_t)1 << (power + 1 - kbits);
  S.tables.resize(n_lo + 3 * n_hi);
  {
    fe starts_m[3] = {Fr::to_mont(Fr::one_std()), Fr::to_mont(S.x[1]), Fr::to_mont(S.x[2])};
    pv::split_power_tables(Fr::to_mont(S.x[0]), kbits, n_hi, starts_m, 3, S.tables.data());
    explicit_bzero(starts_m, sizeof starts_m);
  }
  trace.lap("layout, secrets, tables");

  // ---- sections 2 … 5 up, and through the lane tests before anything else reads them
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  Buffers b;
  static_assert(sizeof(G2::A) == 2 * sizeof(G1::A) && sizeof(G2::P) == 2 * sizeof(G1::P), "a G2 section of 2^power points fills the buffers of a G1 section of 2^(power+1)");
  const size_t top = (size_t)(2 * N);
  for (int k4 = 0; k4 < 4; k4++) b.sec[k4] = ds.buf.alloc<uint8_t>((size_t)L.sec[2 + k4]->size);
  b.proj = ds.buf.alloc<uint8_t>(top * sizeof(G1::P));
  b.scratch = ds.buf.alloc<uint8_t>(top * sizeof(fe));
  b.tables = ds.buf.alloc<fe>(S.tables.size());
  b.first = ds.buf.alloc<unsigned long long>(4);
  if (!b.sec[0] || !b.sec[1] || !b.sec[2] || !b.sec[3] || !b.proj || !b.scratch || !b.tables || !b.first) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  TableWipe wipe; // (declared behind the session: it runs before the session drains and frees)
  wipe.d = b.tables, wipe.bytes = S.tables.size() * sizeof(fe), wipe.st = st;
  DEV_TRY("hipMemset", hipMemsetAsync(b.first, 0xff, 4 * sizeof *b.first, st));
  for (int k4 = 0; k4 < 4; k4++) {
    if (int rc = pv::timed_upload(dev, b.sec[k4], L.sec[2 + k4]->p, (size_t)L.sec[2 + k4]->size, &rep->upload_ms)) return rc;
    if (int rc = enqueue_lane_test(st, k4 == 1, b.sec[k4], counts[k4], b.first + k4)) return rc;
  }
  if (int rc = pv::timed_upload(dev, b.tables, S.tables.data(), S.tables.size() * sizeof(fe), &rep->upload_ms)) return rc;
  unsigned long long first[4] = {NO_FAULT, NO_FAULT, NO_FAULT, NO_FAULT};
  DEV_TRY("download", hipMemcpyAsync(first, b.first, sizeof first, hipMemcpyDeviceToHost, st));
  DEV_TRY("lane tests", hipStreamSynchronize(st));
  trace.lap("sections up, lane tests");
  for (int k4 = 0; k4 < 4; k4++)
    if (first[k4] != NO_FAULT) return fault(2 + k4, first[k4] >> 3, (int)(first[k4] & 7));

  // ---- one scale launch per section, each followed by the way back to the file's form
  for (int k4 = 0; k4 < 4; k4++) {
    const fe *d_lo = b.tables, *d_hi = b.tables + n_lo + (k4 < 2 ? 0 : k4 - 1) * n_hi; // sections 2, 3: c = 1; 4: α′; 5: β′
    if (int rc = k4 == 1 ? scale_section<G2>(st, b, k4, counts[k4], d_lo, d_hi, kbits) : scale_section<G1>(st, b, k4, counts[k4], d_lo, d_hi, kbits)) return rc;
  }

  // ---- meanwhile: the record, section 6, and every section that is copied
  std::vector<uint8_t> record(rec_bytes);
  G2::A beta2_out;
  {
    uint8_t* const r = record.data();
    static const size_t G1_OFF[3] = {TAU1, ALPHA1, BETA1};
    for (int x = 0; x < 3; x++) {
      const G1::A after = zc29::zc_mul_affine<G1, G1L>(point_at<G1::A>(cur + G1_OFF[x]), S.x[x]);
      const G1::A commitment = zc29::zc_mul_affine<G1, G1L>(point_at<G1::A>(before + G1_OFF[x]), S.k[x]);
      memcpy(r + G1_OFF[x], &after, 64);
      memcpy(r + R_TAU + 64 * x, &commitment, 64);
    }
    const G2::A tau2 = zc29::zc_mul_affine<G2, G2L>(point_at<G2::A>(cur + TAU2), S.x[0]);
    beta2_out = zc29::zc_mul_affine<G2, G2L>(beta2_in, S.x[2]);
    memcpy(r + TAU2, &tau2, 128);
    memcpy(r + BETA2, &beta2_out, 128);
    const Record rec = put_tail(r, NAME_LEN, name, name_len, beacon);
    fe c;
    chain_step(h, before, rec, &c);
    for (int x = 0; x < 3; x++) {
      const fe z = schnorr_response(S.k[x], c, S.x[x]);
      memcpy(r + Z_TAU + 32 * x, z.l, 32);
    }
  }
  uint8_t* w = out;
  uint8_t* out_sec[4] = {nullptr, nullptr, nullptr, nullptr};
  memcpy(w, data, 12);
  w += 12;
  for (const pv::SectionEntry& e : pv::sections_in_order(data)) {
    const uint64_t size = e.id == 7 ? e.size + rec_bytes : e.size;
    pv::put_section(w, e.id, size);
    if (e.id >= 2 && e.id <= 5) out_sec[e.id - 2] = w;
    else if (e.id == 6) memcpy(w, &beta2_out, 128);
    else memcpy(w, e.p, (size_t)e.size);
    if (e.id == 7) {
      const uint32_t now = count + 1;
      memcpy(w, &now, 4);
      memcpy(w + e.size, record.data(), (size_t)rec_bytes);
    }
    w += size;
  }
  trace.lap("record, copied sections");

  DEV_TRY("scale kernels", hipStreamSynchronize(st));
  rep->device_ms = pv::ms_since(t_dev);
  trace.lap("kernels done");
  const auto t_down = std::chrono::steady_clock::now();
  isnark::CopyJob jobs[4];
  for (int k4 = 0; k4 < 4; k4++) jobs[k4] = {out_sec[k4], b.sec[k4], (size_t)L.sec[2 + k4]->size};
  DEV_TRY("device to host download", isnark::staged_copy(dev, jobs, 4, false));
  rep->download_ms = pv::ms_since(t_down);
  trace.lap("sections downloaded");
  return 0;
}

} // namespace

ISNARK_API int groth16_ptau_new_size(uint32_t power, uint64_t* ptau_bytes)
{
  if (!ptau_bytes) return pv::fail(pv::ERR_ARG, "null output");
  *ptau_bytes = 0;
  return new_size(power, ptau_bytes);
}

ISNARK_API int groth16_ptau_new(uint32_t power, void* out, size_t cap, uint64_t* out_len)
{
  if (!out_len) return pv::fail(pv::ERR_ARG, "null out_len");
  *out_len = 0;
  uint64_t bytes;
  if (int rc = new_size(power, &bytes)) return rc;
  *out_len = bytes;
  uint8_t* o = nullptr;
  if (int rc = pv::buffer_sink("file", out, cap)(bytes, &o)) return rc;
  new_write(power, o);
  return 0;
}

ISNARK_API int groth16_ptau_new_file(uint32_t power, const char* out_path)
{
  if (!out_path) return pv::fail(pv::ERR_ARG, "null path");
  uint64_t bytes;
  if (int rc = new_size(power, &bytes)) return rc;
  TempOutput to(out_path);
  uint8_t* o = nullptr;
  int rc = to.open(bytes, &o);
  if (rc == 0) new_write(power, o);
  return to.finish(rc);
}

ISNARK_API int groth16_ptau_contribute(const void* ptau, size_t len, const uint8_t* secret32, const char* name, void* out, size_t cap, const char* device,
                                       const Groth16PtauContributeOptions* opt, Groth16PtauContributeReport* report)
{
  return contribute_impl((const uint8_t*)ptau, len, secret32, name, device, opt, report, pv::buffer_sink("file", out, cap));
}

ISNARK_API int groth16_ptau_contribute_file(const char* in_path, const char* out_path, const uint8_t* secret32, const char* name, const char* device,
                                            const Groth16PtauContributeOptions* opt, Groth16PtauContributeReport* report)
{
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr, [&](const uint8_t* data, size_t len, const Sink& sink) {
    return contribute_impl(data, len, secret32, name, device, opt, report, sink);
  });
}

ISNARK_API int groth16_ptau_contributions(const void* ptau, size_t len, Groth16PtauContributionsReport* report, Groth16PtauContributionInfo* infos, size_t infos_cap)
{
  if (!report) return pv::fail(pv::ERR_ARG, "null report");
  memset(report, 0, sizeof *report);
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  if (int rc = pv::ptau_unprepared_layout((const uint8_t*)ptau, len, secs, &L)) return rc;
  auto fault = [&](int32_t kind, uint32_t index) {
    report->kind = kind, report->index = index;
    return 0;
  };
  std::vector<Record> recs;
  uint32_t bad;
  const int malformed = walk_records(L.sec[7], RECORD_FIXED, NAME_LEN, recs, &report->count, &bad);
  for (size_t i = 0; infos && i < recs.size() && i < infos_cap; i++) {
    const uint8_t* const p = recs[i].p;
    memcpy(infos[i].tau1, p + TAU1, 64);
    memcpy(infos[i].alpha1, p + ALPHA1, 64);
    memcpy(infos[i].beta1, p + BETA1, 64);
    memcpy(infos[i].tau2, p + TAU2, 128);
    memcpy(infos[i].beta2, p + BETA2, 128);
    memset(infos[i].name, 0, sizeof infos[i].name);
    memcpy(infos[i].name, p + RECORD_FIXED, recs[i].name_len);
  }
  if (malformed) return fault(GROTH16_CONTRIB_SECTION, bad);
  uint64_t beacon_work = 0;

  uint8_t gens[AFTER_BYTES], h[32];
  generators(gens);
  chain_start(L, h);
  const bn254_affine_t g1 = vb::g1_generator_affine();
  const bn254_g2_affine_t g2 = vb::g2_generator_affine();
  const uint8_t* before = gens;
  for (uint32_t i = 0; i < report->count; i++) {
    const Record& r = recs[i];
    // POINT: all eight on their curves (the G2 points in the subgroup), none of the five `after` points the identity
    G1::A after[3], commitment[3];
    for (int x = 0; x < 3; x++) {
      after[x] = point_at<G1::A>(r.p + 64 * x), commitment[x] = point_at<G1::A>(r.p + R_TAU + 64 * x);
      if (classify(after[x]) || classify(commitment[x]) || G1::aff_is_zero(after[x])) return fault(GROTH16_CONTRIB_POINT, i + 1);
    }
    const G2::A tau2 = point_at<G2::A>(r.p + TAU2), beta2 = point_at<G2::A>(r.p + BETA2);
    if (classify(tau2) || classify(beta2) || G2::aff_is_zero(tau2) || G2::aff_is_zero(beta2)) return fault(GROTH16_CONTRIB_POINT, i + 1);
    // POK: z_x·before.x1 = R_x + c·after.x1, compared in the file's canonical affine form
    fe c;
    chain_step(h, before, r, &c);
    const ZcDigits cd = zc29::zc_recode(c);
    for (int x = 0; x < 3; x++) {
      fe z;
      memcpy(z.l, r.p + Z_TAU + 32 * x, 32);
      if (!pok_holds(point_at<G1::A>(before + 64 * x), after[x], commitment[x], z, cd)) return fault(GROTH16_CONTRIB_POK, i + 1);
    }
    // BEACON: a flagged record within the work bound, whose three G1 points are the recomputed beacon's
    if (r.beacon && (!beacon_work_allowed(beacon_iter_exp(r), &beacon_work) || !record_is_the_beacons(r, before))) return fault(GROTH16_CONTRIB_BEACON, i + 1);
    // PAIR: e(tau1, G₂) = e(G₁, tau2) and e(beta1, G₂) = e(G₁, beta2)
    if (!vb::pairing_eq(std_affine(after[0]), g2, g1, std_affine(tau2)) || !vb::pairing_eq(std_affine(after[2]), g2, g1, std_affine(beta2))) return fault(GROTH16_CONTRIB_PAIR, i + 1);
    before = r.p;
  }
  if (!header_holds(held_points(L), before)) return fault(GROTH16_CONTRIB_HEADER, 0);
  return 1;
}

// ---- the random beacon
ISNARK_API int groth16_beacon_digest(const uint8_t hash[32], uint32_t iter_exp, uint8_t out[32])
{
  if (!hash || !out) return pv::fail(pv::ERR_ARG, "null argument");
  if (iter_exp > BEACON_ITER_EXP_MAX) return pv::fail(pv::ERR_ARG, "beacon: iter_exp %u is above %u", iter_exp, BEACON_ITER_EXP_MAX);
  beacon_digest(hash, iter_exp, out);
  return 0;
}

ISNARK_API int groth16_ptau_beacon(const void* ptau, size_t len, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name, void* out, size_t cap, const char* device,
                                   Groth16PtauContributeReport* report)
{
  const Beacon b = {beacon_hash, iter_exp};
  return contribute_impl((const uint8_t*)ptau, len, nullptr, name, device, nullptr, report, pv::buffer_sink("file", out, cap), &b);
}

ISNARK_API int groth16_ptau_beacon_file(const char* in_path, const char* out_path, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name, const char* device,
                                        Groth16PtauContributeReport* report)
{
  const Beacon b = {beacon_hash, iter_exp};
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr, [&](const uint8_t* data, size_t len, const Sink& sink) {
    return contribute_impl(data, len, nullptr, name, device, nullptr, report, sink, &b);
  });
}

ISNARK_API int groth16_ptau_beacons(const void* ptau, size_t len, Groth16BeaconInfo* infos, size_t cap)
{
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  if (int rc = pv::ptau_unprepared_layout((const uint8_t*)ptau, len, secs, &L)) return rc;
  std::vector<Record> recs;
  uint32_t count, bad;
  const int malformed = walk_records(L.sec[7], RECORD_FIXED, NAME_LEN, recs, &count, &bad);
  return list_beacons(held_records(recs, malformed, bad), infos, cap);
}
