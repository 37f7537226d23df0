// zkey_contribute.hip — groth16_zkey_contribute: one phase-2 contribution δ′ applied to a proving key, and groth16_zkey_contributions,
// the host's audit of the chain section 10 records.  include/groth16_prover.h has the contract and section 10's layout; DESIGN.md §7f.
// groth16_zkey_beacon is the same call with the secret replaced by the beacon's public digest and the record's tail added (§7o).
//
//   host, first  the container (zkey_layout), section 10's bounds and hash chain, the output's size against the room, the header's δ₁
//                and δ₂ through the key check's lane tests; δ′, the nonce k and the record — three G1 and one G2 scalar
//                multiplications by zkey_contribute29.h's zc_mul_affine, the text the kernel runs.  transcript.h has the hashes,
//                the record walk and the proof of knowledge, one text with groth16_ptau_contribute's.
//   device       sections 8 and 9 go up into one array; zc_scale_g1_kernel, one lane per point: the lane test (classify_g1: a hostile
//                file does not reach the lazy arithmetic), then δ′⁻¹·P by zc_scale with the digit masks of δ′⁻¹ in the kernel's
//                argument struct — the same scalar in every lane: no divergence, nothing per lane but the point.  A faulty point is the
//                rare branch: its lane alone counts itself and takes the minimum of (index, kind) (pack_device.h's tally).  Then
//                point_form.h's to_file_form, the identity kept as zeros, and down into the output's sections 8 and 9.
//   host, beside the sections no contribution changes are copied while the kernels run; nothing of the output is final before the tally says
//                that no point was at fault (the _file entry unlinks its temporary otherwise).
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "pack_device.h"
#include "point_form.h"
#include "prover_internal.h"
#include "transcript.h"
#include "verify_batch.h"

using namespace bn254;
using namespace isnark::transcript;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int SCALE_WG = 64;
using pv::NO_FAULT;
using pv::POINT_FAULT;
const char TAG[] = "icicle-snark zkey contribution v1";
constexpr size_t TAG_LEN = sizeof TAG - 1;
constexpr size_t HEADER_FIXED = 468;                       // section 2 up to and including γ₂
constexpr size_t DELTA1_OFF = 468, DELTA2_OFF = 532;       // in section 2's payload
// a record: after1, the commitment, the response, the name
constexpr size_t AFTER1 = 0, COMMITMENT = 64, RESPONSE = 128, NAME_LEN = 160, RECORD_FIXED = 164;

// One lane per point of sections 8 | 9 (pts[i], i < n): δ′⁻¹·P as Montgomery projective, the identity (0, 1, 0).  A lane whose point
// fails the lane test writes the identity and tallies itself (t->first: index over sections 8 | 9): nothing of such a run is used.
__global__ __launch_bounds__(SCALE_WG) void zc_scale_g1_kernel(const G1::A* __restrict__ pts, uint64_t n, ZcDigits digits, G1::P* __restrict__ out, pv::PackTally* __restrict__ t)
{
  const uint64_t i = (uint64_t)blockIdx.x * SCALE_WG + threadIdx.x;
  if (i >= n) return;
  const G1::A p = pts[i];
  const fe words[2] = {p.x, p.y};
  const int kind = p29::classify_g1(words);
  if (kind) pv::tally_fault(t, i, kind);
  if (kind || G1::aff_is_zero(p)) {
    out[i] = G1::p_zero();
    return;
  }
  out[i] = G1::x_to_projective(G1L::x_store(zc29::zc_scale<G1L>(p, digits)));
}

// ---- section 10 (the scalars, the record walk and the proof of knowledge are transcript.h's; no section 10: no records)
// h₀: what no contribution changes
void chain_start(const pv::ZkeyLayout& L, uint8_t h[32])
{
  std::vector<uint8_t> m;
  append(m, TAG, TAG_LEN);
  append(m, L.sec[2]->p, HEADER_FIXED);
  append(m, L.sec[3]->p, (size_t)L.sec[3]->size);
  isnark::sha256(m.data(), m.size(), h);
}
// e_i = SHA-256(h_{i−1} ‖ before1 ‖ after1 ‖ R ‖ name_len as stored ‖ name ‖ a beacon's trailer) → h (in place); c: its first 16
// bytes, little-endian, 0 → 1
void chain_step(uint8_t h[32], const uint8_t* before1, const Record& r, fe* c)
{
  std::vector<uint8_t> m;
  append(m, h, 32);
  append(m, before1, 64);
  append(m, r.p + AFTER1, 64);
  append(m, r.p + COMMITMENT, 64);
  append(m, r.p + NAME_LEN, hashed_tail(r));
  hash_step(m, h, c);
}

// δ′ = W(seed ‖ TAG), standard form; false when it is zero
bool derive_delta(const uint8_t seed[32], fe* delta)
{
  std::vector<uint8_t> m;
  append(m, seed, 32);
  append(m, TAG, TAG_LEN);
  *delta = wide_hash(m);
  return !Fr::is_zero(*delta);
}
// BEACON's last question (transcript.h's beacon_work_allowed has passed): with the digest and δ′ recomputed, is after1 = δ′·before1
// in the file's canonical affine bytes?
bool record_is_the_beacons(const Record& r, const G1::A& before)
{
  uint8_t digest[32];
  beacon_digest(r.trailer, beacon_iter_exp(r), digest);
  fe delta;
  if (!derive_delta(digest, &delta)) return false;
  const G1::A want = zc29::zc_mul_affine<G1, G1L>(before, delta);
  return memcmp(&want, r.p + AFTER1, 64) == 0;
}

// everything secret of one call; wiped on every way out (best effort: the compiler may have kept copies in registers or spills)
struct Secrets {
  uint8_t seed[32];
  fe delta, delta_inv, k;
  ZcDigits digits;
  ~Secrets() { explicit_bzero(this, sizeof *this); }
};

using pv::Sink;

// beacon: null for a participant's contribution; else secret32 is not read — the secret is the beacon's digest — and opt is null
int contribute_impl(const uint8_t* data, size_t len, const uint8_t* secret32, const char* name, const char* device, const Groth16ZkeyContributeOptions* opt,
                    Groth16ZkeyContributeReport* rep, const Sink& sink, const Beacon* beacon = nullptr)
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
  pv::ZkeyLayout L;
  if (int rc = pv::zkey_layout(data, len, secs, &L)) return rc;
  if (secs[10].count > 1) return pv::fail(pv::ERR_FORMAT, "Section Duplicated 10");
  const pv::Section* s10 = secs[10].count ? &secs[10] : nullptr;
  std::vector<Record> recs;
  uint32_t count, bad;
  if (walk_records(s10, RECORD_FIXED, NAME_LEN, recs, &count, &bad)) return pv::fail(pv::ERR_FORMAT, "zkey: section 10 is malformed at record %u of %u", bad, count);
  const uint8_t* const hdr = L.sec[2]->p;
  if (count && memcmp(recs.back().p + AFTER1, hdr + DELTA1_OFF, 64) != 0) return pv::fail(pv::ERR_FORMAT, "zkey: section 10's last record is not the header's delta1");

  // the output's size, before anything else is done
  const std::vector<pv::SectionEntry> order = pv::sections_in_order(data);
  const uint64_t rec_bytes = RECORD_FIXED + tail_bytes(name_len, beacon);
  uint64_t total = 12 + rec_bytes + (s10 ? 0 : 12 + 4);
  for (const pv::SectionEntry& e : order) total += 12 + e.size;
  const uint64_t n8 = L.sec[8]->size / 64, n9 = L.sec[9]->size / 64, n = n8 + n9;
  rep->contribution = count + 1;
  rep->points_c = n8, rep->points_h = n9;
  rep->zkey_bytes = total;
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;

  // the header's δ₁ and δ₂: the lane tests, and neither the identity
  const G1::A d1 = point_at<G1::A>(hdr + DELTA1_OFF);
  const G2::A d2 = point_at<G2::A>(hdr + DELTA2_OFF);
  if (const int kind = classify(d1)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta1: %s", POINT_FAULT[kind & 3]);
  if (const int kind = classify(d2)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta2: %s", POINT_FAULT[kind & 3]);
  if (G1::aff_is_zero(d1) || G2::aff_is_zero(d2)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta is the identity");

  // ---- δ′, the nonce, the record
  Secrets S;
  uint8_t digest[32];
  if (beacon) beacon_digest(beacon->hash, beacon->iter_exp, digest), secret32 = digest; // (public: nothing of it needs wiping)
  if (int rc = pv::seed_or_random(secret32, S.seed)) return rc;
  if (opt && opt->fixed_delta) {
    memcpy(S.delta.l, opt->fixed_delta, 32);
    if (!Fr::is_canonical(S.delta) || Fr::is_zero(S.delta)) return pv::fail(pv::ERR_ARG, "fixed_delta is not in [1, r)");
  } else if (!derive_delta(S.seed, &S.delta)) {
    return pv::fail(pv::ERR_ARG, "the secret gives delta' = 0");
  }
  S.delta_inv = fr_inv(S.delta);
  S.digits = zc29::zc_recode(S.delta_inv);
  // h_{i−1} over the records there are, as groth16_zkey_contributions hashes them: record 1's before1 is G₁
  uint8_t h[32];
  chain_start(L, h);
  const G1::A g1 = vb::g1_generator_mont();
  for (uint32_t i = 0; i < count; i++) {
    fe c;
    chain_step(h, i ? recs[i - 1].p + AFTER1 : (const uint8_t*)&g1, recs[i], &c);
  }
  {
    std::vector<uint8_t> m;
    append(m, S.seed, 32);
    append(m, S.delta.l, 32);
    append(m, h, 32);
    append(m, &d1, 64);
    S.k = wide_hash(m);
    if (Fr::is_zero(S.k)) return pv::fail(pv::ERR_ARG, "the secret gives the nonce 0");
  }
  const G1::A after1 = zc29::zc_mul_affine<G1, G1L>(d1, S.delta), commitment = zc29::zc_mul_affine<G1, G1L>(d1, S.k);
  const G2::A after2 = zc29::zc_mul_affine<G2, G2L>(d2, S.delta);
  std::vector<uint8_t> record(rec_bytes);
  {
    uint8_t* const b = record.data();
    memcpy(b + AFTER1, &after1, 64);
    memcpy(b + COMMITMENT, &commitment, 64);
    const Record r = put_tail(b, NAME_LEN, name, name_len, beacon);
    fe c;
    chain_step(h, hdr + DELTA1_OFF, r, &c);
    const fe z = schnorr_response(S.k, c, S.delta);
    memcpy(b + RESPONSE, z.l, 32);
  }

  pv::StageTrace trace("zkey-contribute", "ICICLE_SNARK_TRACE_ZKEY_CONTRIBUTE");
  trace.lap("layout, record");

  // ---- sections 8 | 9 through the kernel
  if (n > 0xffffffffull) return pv::fail(pv::ERR_ARG, "sections 8 and 9 hold more than 2^32 points");
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  const size_t cnt = (size_t)std::max<uint64_t>(n, 1);
  G1::A* d_in = ds.buf.alloc<G1::A>(cnt);
  G1::P* d_p = ds.buf.alloc<G1::P>(cnt);
  G1::A* d_a = ds.buf.alloc<G1::A>(cnt);
  fe* d_s = ds.buf.alloc<fe>(cnt);
  pv::PackTally* d_tally = ds.buf.alloc<pv::PackTally>(1);
  if (!d_in || !d_p || !d_a || !d_s || !d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  pv::PackTally tally; // (lives until the call's own synchronisation)
  if (int rc = pv::reset_tallies(&tally, d_tally, 1, st)) return rc;
  if (int rc = pv::timed_upload(dev, d_in, L.sec[8]->p, (size_t)n8 * 64, &rep->upload_ms)) return rc;
  if (int rc = pv::timed_upload(dev, d_in + n8, L.sec[9]->p, (size_t)n9 * 64, &rep->upload_ms)) return rc;
  trace.lap("sections 8, 9 uploaded");
  if (n) {
    DEV_LAUNCH("scale kernel launch", zc_scale_g1_kernel, dim3((uint32_t)((n + SCALE_WG - 1) / SCALE_WG)), dim3(SCALE_WG), st, d_in, n, S.digits, d_p, d_tally);
    if (int rc = pv::to_file_form<G1>(st, d_p, n, d_a, d_s)) return rc;
  }
  DEV_TRY("download", hipMemcpyAsync(&tally, d_tally, sizeof tally, hipMemcpyDeviceToHost, st));

  // ---- meanwhile: the container, and every section that is copied
  uint8_t* w = out;
  uint8_t *out8 = nullptr, *out9 = nullptr;
  auto section10 = [&] {
    const uint64_t old = s10 ? s10->size : 4;
    const uint32_t now = count + 1;
    pv::put_section(w, 10, old + rec_bytes);
    memcpy(w, &now, 4);
    if (s10) memcpy(w + 4, s10->p + 4, (size_t)old - 4);
    memcpy(w + old, record.data(), (size_t)rec_bytes);
    w += old + rec_bytes;
  };
  uint32_t version;
  memcpy(&version, data + 4, 4);
  pv::put_container_head(w, "zkey", version, (uint32_t)order.size() + (s10 ? 0 : 1));
  for (const pv::SectionEntry& e : order) {
    if (e.id == 10) {
      section10();
      continue;
    }
    pv::put_section(w, e.id, e.size);
    if (e.id == 8) out8 = w;
    else if (e.id == 9) out9 = w;
    else memcpy(w, e.p, (size_t)e.size); // (in ranges on the worker pool this took 230–253 ms instead of 155–160 at benchmark/1600k: not kept)
    if (e.id == 2) {
      memcpy(w + DELTA1_OFF, &after1, 64);
      memcpy(w + DELTA2_OFF, &after2, 128);
    }
    w += e.size;
  }
  if (!s10) section10();
  trace.lap("copied sections written");

  DEV_TRY("scale kernels", hipStreamSynchronize(st));
  rep->device_ms = pv::ms_since(t_dev);
  trace.lap("kernels done");
  rep->faults = tally.count;
  if (tally.first != NO_FAULT) {
    const uint64_t i = tally.first >> 3;
    pv::set_point_fault(rep, i < n8 ? 8 : 9, i < n8 ? i : i - n8, (int)(tally.first & 7));
    return pv::fail(pv::ERR_FORMAT, "zkey: section %d, element %llu: %s (%llu points at fault)", rep->fault_section, (unsigned long long)rep->fault_index, POINT_FAULT[rep->fault_kind & 3],
                    (unsigned long long)tally.count);
  }
  const auto t_down = std::chrono::steady_clock::now();
  const isnark::CopyJob jobs[2] = {{out8, d_a, (size_t)n8 * 64}, {out9, d_a + n8, (size_t)n9 * 64}};
  DEV_TRY("device to host download", isnark::staged_copy(dev, jobs, 2, false));
  rep->download_ms = pv::ms_since(t_down);
  trace.lap("sections 8, 9 downloaded");
  return 0;
}

} // namespace

ISNARK_API int groth16_zkey_contribute(const void* zkey, size_t len, const uint8_t* secret32, const char* name, void* out, size_t cap, const char* device,
                                       const Groth16ZkeyContributeOptions* opt, Groth16ZkeyContributeReport* report)
{
  return contribute_impl((const uint8_t*)zkey, len, secret32, name, device, opt, report, pv::buffer_sink("key", out, cap));
}

ISNARK_API int groth16_zkey_contribute_file(const char* zkey_path, const char* out_path, const uint8_t* secret32, const char* name, const char* device,
                                            const Groth16ZkeyContributeOptions* opt, Groth16ZkeyContributeReport* report)
{
  return pv::rewrite_file(zkey_path, out_path, report ? &report->write_ms : nullptr, [&](const uint8_t* data, size_t len, const Sink& sink) {
    return contribute_impl(data, len, secret32, name, device, opt, report, sink);
  });
}

ISNARK_API int groth16_zkey_contributions(const void* zkey, size_t len, Groth16ContributionsReport* report, Groth16ContributionInfo* infos, size_t infos_cap)
{
  if (!report) return pv::fail(pv::ERR_ARG, "null report");
  memset(report, 0, sizeof *report);
  std::vector<pv::Section> secs;
  pv::ZkeyLayout L;
  if (int rc = pv::zkey_layout((const uint8_t*)zkey, len, secs, &L)) return rc;
  auto fault = [&](int32_t kind, uint32_t index) {
    report->kind = kind, report->index = index;
    return 0;
  };
  if (secs[10].count > 1) return fault(GROTH16_CONTRIB_SECTION, 0);
  std::vector<Record> recs;
  uint32_t bad;
  const int malformed = walk_records(secs[10].count ? &secs[10] : nullptr, RECORD_FIXED, NAME_LEN, recs, &report->count, &bad);
  for (size_t i = 0; infos && i < recs.size() && i < infos_cap; i++) {
    memcpy(infos[i].after1, recs[i].p + AFTER1, 64);
    memset(infos[i].name, 0, sizeof infos[i].name);
    memcpy(infos[i].name, recs[i].p + RECORD_FIXED, recs[i].name_len);
  }
  if (malformed) return fault(GROTH16_CONTRIB_SECTION, bad);

  const uint8_t* const hdr = L.sec[2]->p;
  const G1::A g1 = vb::g1_generator_mont();
  uint8_t h[32];
  chain_start(L, h);
  G1::A before = g1;
  uint64_t beacon_work = 0;
  for (uint32_t i = 0; i < report->count; i++) {
    const Record& r = recs[i];
    const G1::A after = point_at<G1::A>(r.p + AFTER1), commitment = point_at<G1::A>(r.p + COMMITMENT);
    fe z;
    memcpy(z.l, r.p + RESPONSE, 32);
    if (classify(after) || classify(commitment) || G1::aff_is_zero(after)) return fault(GROTH16_CONTRIB_POINT, i + 1);
    fe c;
    chain_step(h, (const uint8_t*)&before, r, &c);
    if (!pok_holds(before, after, commitment, z, zc29::zc_recode(c))) return fault(GROTH16_CONTRIB_POK, i + 1);
    // BEACON: a flagged record within the work bound, whose after1 is the recomputed beacon's
    if (r.beacon && (!beacon_work_allowed(beacon_iter_exp(r), &beacon_work) || !record_is_the_beacons(r, before))) return fault(GROTH16_CONTRIB_BEACON, i + 1);
    before = after;
  }
  if (memcmp(&before, hdr + DELTA1_OFF, 64) != 0) return fault(GROTH16_CONTRIB_HEADER, 0);
  // e(δ₁, G₂) = e(G₁, δ₂); δ₁ is a point that has passed the lane test (or G₁), δ₂ gets its own
  const G2::A d2 = point_at<G2::A>(hdr + DELTA2_OFF);
  if (classify(d2) || G2::aff_is_zero(d2)) return fault(GROTH16_CONTRIB_PAIR, 0);
  if (!vb::pairing_eq(std_affine(before), vb::g2_generator_affine(), vb::g1_generator_affine(), std_affine(d2))) return fault(GROTH16_CONTRIB_PAIR, 0);
  return 1;
}

// ---- the random beacon (groth16_beacon_digest is ptau_contribute.hip's)
ISNARK_API int groth16_zkey_beacon(const void* zkey, size_t len, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name, void* out, size_t cap, const char* device,
                                   Groth16ZkeyContributeReport* report)
{
  const Beacon b = {beacon_hash, iter_exp};
  return contribute_impl((const uint8_t*)zkey, len, nullptr, name, device, nullptr, report, pv::buffer_sink("key", out, cap), &b);
}

ISNARK_API int groth16_zkey_beacon_file(const char* zkey_path, const char* out_path, const uint8_t beacon_hash[32], uint32_t iter_exp, const char* name, const char* device,
                                        Groth16ZkeyContributeReport* report)
{
  const Beacon b = {beacon_hash, iter_exp};
  return pv::rewrite_file(zkey_path, out_path, report ? &report->write_ms : nullptr, [&](const uint8_t* data, size_t len, const Sink& sink) {
    return contribute_impl(data, len, nullptr, name, device, nullptr, report, sink, &b);
  });
}

ISNARK_API int groth16_zkey_beacons(const void* zkey, size_t len, Groth16BeaconInfo* infos, size_t cap)
{
  std::vector<pv::Section> secs;
  pv::ZkeyLayout L;
  if (int rc = pv::zkey_layout((const uint8_t*)zkey, len, secs, &L)) return rc;
  if (secs[10].count > 1) return 0; // (the audit's SECTION fault of the count: no record's bounds hold)
  std::vector<Record> recs;
  uint32_t count, bad;
  const int malformed = walk_records(secs[10].count ? &secs[10] : nullptr, RECORD_FIXED, NAME_LEN, recs, &count, &bad);
  return list_beacons(held_records(recs, malformed, bad), infos, cap);
}
