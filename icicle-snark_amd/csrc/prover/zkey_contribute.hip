// zkey_contribute.hip — groth16_zkey_contribute: one phase-2 contribution δ′ applied to a proving key, and groth16_zkey_contributions,
// the host's audit of the chain section 10 records.  include/groth16_prover.h has the contract and section 10's layout; DESIGN.md §7f.
//
//   host, first  the container (zkey_layout), section 10's bounds and hash chain, the output's size against the room, the header's δ₁
//                and δ₂ through the key check's lane tests; δ′, the nonce k and the record — three G1 and one G2 scalar
//                multiplications by zkey_contribute29.h's zc_mul_affine, the text the kernel runs.
//   device       sections 8 and 9 go up into one array; zc_scale_g1_kernel, one lane per point: the lane test (classify_g1: a hostile
//                file does not reach the lazy arithmetic), then δ′⁻¹·P by zc_scale with the digit masks of δ′⁻¹ in the kernel's
//                argument struct — the same scalar in every lane: no divergence, nothing per lane but the point.  A faulty point is the
//                rare branch: its lane alone counts itself and takes the minimum of (index, kind).  Then batch_to_affine_kernel and
//                affine_to_mont_kernel (msm_impl.h's), the identity kept as zeros, and down into the output's sections 8 and 9.
//   host, beside the sections no contribution changes are copied while the kernels run; nothing of the output is final before the tally says
//                that no point was at fault (the _file entry unlinks its temporary otherwise).
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../msm_impl.h"
#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "sha256.h"
#include "verify_batch.h"
#include "zkey_check29.h"
#include "zkey_contribute29.h"

using namespace bn254;
using bn254::zc29::ZcDigits;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int SCALE_WG = 64;
using pv::NO_FAULT;
const char TAG[] = "icicle-snark zkey contribution v1";
constexpr size_t TAG_LEN = sizeof TAG - 1;
constexpr size_t HEADER_FIXED = 468;                       // section 2 up to and including γ₂
constexpr size_t DELTA1_OFF = 468, DELTA2_OFF = 532;       // in section 2's payload
constexpr size_t RECORD_FIXED = 64 + 64 + 32 + 4;
constexpr uint32_t NAME_BYTES_MAX = 255;
const char* const FAULT_TEXT[4] = {"", "a coordinate is not below q", "the point is not on the curve", "the point is outside the subgroup"};

struct Tally {
  unsigned long long count, first; // faulty points; min over them of (index << 3 | kind), index over sections 8 | 9
};

// One lane per point of sections 8 | 9 (pts[i], i < n): δ′⁻¹·P as Montgomery projective, the identity (0, 1, 0).  A lane whose point
// fails the lane test writes the identity and tallies itself: nothing of such a run is used.
__global__ __launch_bounds__(SCALE_WG) void zc_scale_g1_kernel(const G1::A* __restrict__ pts, uint64_t n, ZcDigits digits, G1::P* __restrict__ out, Tally* __restrict__ t)
{
  const uint64_t i = (uint64_t)blockIdx.x * SCALE_WG + threadIdx.x;
  if (i >= n) return;
  const G1::A p = pts[i];
  const fe words[2] = {p.x, p.y};
  const int kind = p29::classify_g1(words);
  if (kind) {
    atomicAdd(&t->count, 1ull);
    atomicMin(&t->first, (unsigned long long)i << 3 | (unsigned long long)kind);
  }
  if (kind || G1::aff_is_zero(p)) {
    out[i] = G1::p_zero();
    return;
  }
  out[i] = G1::x_to_projective(G1L::x_store(zc29::zc_scale<G1L>(p, digits)));
}

// ---- scalars on the host: standard form, below r
fe fr_mul(const fe& a, const fe& b) { return Fr::mul(Fr::to_mont(a), b); }
fe fr_inv(const fe& a) { return Fr::from_mont(Fr::inv(Fr::to_mont(a))); }
// a big-endian integer of `len` bytes mod r, by Horner's rule in additions
fe fr_from_be(const uint8_t* b, size_t len)
{
  fe acc = Fr::zero();
  for (size_t i = 0; i < len; i++) {
    for (int k = 0; k < 8; k++) acc = Fr::dbl(acc);
    fe d = Fr::zero();
    d.l[0] = b[i];
    acc = Fr::add(acc, d);
  }
  return acc;
}
// W(x) = SHA-256(x ‖ 0x00) ‖ SHA-256(x ‖ 0x01) as a 512-bit big-endian integer, mod r.  x is wiped: it holds the secret.
fe wide_hash(std::vector<uint8_t>& x)
{
  uint8_t d[64];
  x.push_back(0);
  isnark::sha256(x.data(), x.size(), d);
  x.back() = 1;
  isnark::sha256(x.data(), x.size(), d + 32);
  const fe v = fr_from_be(d, 64);
  explicit_bzero(d, sizeof d);
  explicit_bzero(x.data(), x.size());
  return v;
}
void append(std::vector<uint8_t>& v, const void* p, size_t n) { v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n); }

// ---- section 10
struct Record {
  const uint8_t *after1, *commitment, *z, *name;
  uint32_t name_len;
  size_t bytes() const { return RECORD_FIXED + name_len; }
};
// the records of section 10 (s10 null: no section, no records).  0, or 1 with *bad = the record that does not fit (0: the count);
// recs holds the records before it.
int walk_records(const pv::Section* s10, std::vector<Record>& recs, uint32_t* count, uint32_t* bad)
{
  recs.clear();
  *count = 0, *bad = 0;
  if (!s10) return 0;
  if (s10->size < 4) return 1;
  uint32_t n;
  memcpy(&n, s10->p, 4);
  if ((uint64_t)n * RECORD_FIXED > s10->size - 4) return 1; // (a hostile count sizes nothing)
  *count = n;
  uint64_t pos = 4;
  for (uint32_t i = 0; i < n; i++) {
    *bad = i + 1;
    if (s10->size - pos < RECORD_FIXED) return 1;
    Record r;
    r.after1 = s10->p + pos, r.commitment = r.after1 + 64, r.z = r.after1 + 128;
    memcpy(&r.name_len, r.after1 + 160, 4);
    r.name = r.after1 + RECORD_FIXED;
    if (r.name_len > NAME_BYTES_MAX || s10->size - pos - RECORD_FIXED < r.name_len) return 1;
    recs.push_back(r);
    pos += r.bytes();
  }
  *bad = n;
  return pos == s10->size ? 0 : 1; // bytes behind the last record
}
// h₀: what no contribution changes
void chain_start(const pv::ZkeyLayout& L, uint8_t h[32])
{
  std::vector<uint8_t> m;
  append(m, TAG, TAG_LEN);
  append(m, L.sec[2]->p, HEADER_FIXED);
  append(m, L.sec[3]->p, (size_t)L.sec[3]->size);
  isnark::sha256(m.data(), m.size(), h);
}
// e_i = SHA-256(h_{i−1} ‖ before1 ‖ after1 ‖ R ‖ name_len ‖ name) → h (in place); c: its first 16 bytes, little-endian, 0 → 1
void chain_step(uint8_t h[32], const uint8_t* before1, const Record& r, fe* c)
{
  std::vector<uint8_t> m;
  append(m, h, 32);
  append(m, before1, 64);
  append(m, r.after1, 64);
  append(m, r.commitment, 64);
  append(m, &r.name_len, 4);
  append(m, r.name, r.name_len);
  isnark::sha256(m.data(), m.size(), h);
  uint8_t c16[16];
  isnark::combined_coefficient_from_digest(h, c16);
  *c = Fr::zero();
  memcpy(c->l, c16, 16);
}

// everything secret of one call; wiped on every way out (best effort: the compiler may have kept copies in registers or spills)
struct Secrets {
  uint8_t seed[32];
  fe delta, delta_inv, k;
  ZcDigits digits;
  ~Secrets() { explicit_bzero(this, sizeof *this); }
};

using pv::Sink;

int contribute_impl(const uint8_t* data, size_t len, const uint8_t* secret32, const char* name, const char* device, const Groth16ZkeyContributeOptions* opt,
                    Groth16ZkeyContributeReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
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
  if (walk_records(s10, recs, &count, &bad)) return pv::fail(pv::ERR_FORMAT, "zkey: section 10 is malformed at record %u of %u", bad, count);
  const uint8_t* const hdr = L.sec[2]->p;
  if (count && memcmp(recs.back().after1, hdr + DELTA1_OFF, 64) != 0) return pv::fail(pv::ERR_FORMAT, "zkey: section 10's last record is not the header's delta1");

  // the output's size, before anything else is done
  const std::vector<pv::SectionEntry> order = pv::sections_in_order(data);
  const uint64_t rec_bytes = RECORD_FIXED + name_len;
  uint64_t total = 12 + rec_bytes + (s10 ? 0 : 12 + 4);
  for (const pv::SectionEntry& e : order) total += 12 + e.size;
  const uint64_t n8 = L.sec[8]->size / 64, n9 = L.sec[9]->size / 64, n = n8 + n9;
  rep->contribution = count + 1;
  rep->points_c = n8, rep->points_h = n9;
  rep->zkey_bytes = total;
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;

  // the header's δ₁ and δ₂: the lane tests, and neither the identity
  G1::A d1;
  G2::A d2;
  memcpy(&d1, hdr + DELTA1_OFF, 64);
  memcpy(&d2, hdr + DELTA2_OFF, 128);
  {
    const fe w1[2] = {d1.x, d1.y};
    const fe2 w2[2] = {d2.x, d2.y};
    if (const int kind = p29::classify_g1(w1)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta1: %s", FAULT_TEXT[kind & 3]);
    if (const int kind = p29::classify_g2(w2)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta2: %s", FAULT_TEXT[kind & 3]);
    if (G1::aff_is_zero(d1) || G2::aff_is_zero(d2)) return pv::fail(pv::ERR_FORMAT, "zkey: the header's delta is the identity");
  }

  // ---- δ′, the nonce, the record
  Secrets S;
  if (int rc = pv::seed_or_random(secret32, S.seed)) return rc;
  if (opt && opt->fixed_delta) {
    memcpy(S.delta.l, opt->fixed_delta, 32);
    if (!Fr::is_canonical(S.delta) || Fr::is_zero(S.delta)) return pv::fail(pv::ERR_ARG, "fixed_delta is not in [1, r)");
  } else {
    std::vector<uint8_t> m;
    append(m, S.seed, 32);
    append(m, TAG, TAG_LEN);
    S.delta = wide_hash(m);
    if (Fr::is_zero(S.delta)) return pv::fail(pv::ERR_ARG, "the secret gives delta' = 0");
  }
  S.delta_inv = fr_inv(S.delta);
  S.digits = zc29::zc_recode(S.delta_inv);
  // h_{i−1} over the records there are, as groth16_zkey_contributions hashes them: record 1's before1 is G₁
  uint8_t h[32];
  chain_start(L, h);
  const G1::A g1 = vb::g1_generator_mont();
  for (uint32_t i = 0; i < count; i++) {
    fe c;
    chain_step(h, i ? recs[i - 1].after1 : (const uint8_t*)&g1, recs[i], &c);
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
    const uint32_t nl = (uint32_t)name_len;
    uint8_t* const b = record.data();
    memcpy(b, &after1, 64);
    memcpy(b + 64, &commitment, 64);
    memcpy(b + 160, &nl, 4);
    memcpy(b + RECORD_FIXED, name, name_len);
    const Record r = {b, b + 64, b + 128, b + RECORD_FIXED, nl};
    fe c;
    chain_step(h, hdr + DELTA1_OFF, r, &c);
    const fe z = Fr::add(S.k, fr_mul(c, S.delta));
    memcpy(b + 128, z.l, 32);
  }

  pv::StageTrace trace("zkey-contribute", "ICICLE_SNARK_TRACE_ZKEY_CONTRIBUTE");
  trace.lap("layout, record");

  // ---- sections 8 | 9 through the kernel
  if (n > 0xffffffffull) return pv::fail(pv::ERR_ARG, "sections 8 and 9 hold more than 2^32 points");
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (ds.open(dev, 1)) return pv::fail(pv::ERR_DEVICE, "%s", groth16_verify_last_error());
  const hipStream_t st = ds.stream(0);
  const size_t cnt = (size_t)std::max<uint64_t>(n, 1);
  G1::A* d_in = ds.buf.alloc<G1::A>(cnt);
  G1::P* d_p = ds.buf.alloc<G1::P>(cnt);
  G1::A* d_a = ds.buf.alloc<G1::A>(cnt);
  fe* d_s = ds.buf.alloc<fe>(cnt);
  Tally* d_tally = ds.buf.alloc<Tally>(1);
  if (!d_in || !d_p || !d_a || !d_s || !d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  Tally tally = {0, NO_FAULT};
  DEV_TRY("upload", hipMemcpyAsync(d_tally, &tally, sizeof tally, hipMemcpyHostToDevice, st));
  DEV_TRY("upload", hipStreamSynchronize(st)); // (`tally` is pageable: the copy has read it)
  if (int rc = pv::timed_upload(dev, d_in, L.sec[8]->p, (size_t)n8 * 64, &rep->upload_ms)) return rc;
  if (int rc = pv::timed_upload(dev, d_in + n8, L.sec[9]->p, (size_t)n9 * 64, &rep->upload_ms)) return rc;
  trace.lap("sections 8, 9 uploaded");
  if (n) {
    const int chunk = 32;
    const uint64_t threads = (n + chunk - 1) / chunk;
    DEV_LAUNCH("scale kernel launch", zc_scale_g1_kernel, dim3((uint32_t)((n + SCALE_WG - 1) / SCALE_WG)), dim3(SCALE_WG), st, d_in, n, S.digits, d_p, d_tally);
    DEV_LAUNCH("batch_to_affine launch", (batch_to_affine_kernel<G1, FqOps>), dim3((uint32_t)((threads + 63) / 64)), dim3(64), st, d_p, n, chunk, d_a, d_s);
    DEV_LAUNCH("affine_to_mont launch", (affine_to_mont_kernel<G1::A>), dim3((uint32_t)((2 * n + 255) / 256)), dim3(256), st, d_a, 2 * n);
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
    rep->fault_kind = (int32_t)(tally.first & 7);
    rep->fault_section = i < n8 ? 8 : 9;
    rep->fault_index = i < n8 ? i : i - n8;
    return pv::fail(pv::ERR_FORMAT, "zkey: section %d, element %llu: %s (%llu points at fault)", rep->fault_section, (unsigned long long)rep->fault_index, FAULT_TEXT[rep->fault_kind & 3],
                    (unsigned long long)tally.count);
  }
  const auto t_down = std::chrono::steady_clock::now();
  const isnark::CopyJob jobs[2] = {{out8, d_a, (size_t)n8 * 64}, {out9, d_a + n8, (size_t)n9 * 64}};
  DEV_TRY("device to host download", isnark::staged_copy(dev, jobs, 2, false));
  rep->download_ms = pv::ms_since(t_down);
  trace.lap("sections 8, 9 downloaded");
  return 0;
}

// a Montgomery-form header point as the host pairing takes it
bn254_affine_t std_affine(const G1::A& a)
{
  const G1::A s = {Fq::from_mont(a.x), Fq::from_mont(a.y)};
  bn254_affine_t p;
  memcpy(&p, &s, sizeof p);
  return p;
}
bn254_g2_affine_t std_affine(const G2::A& a)
{
  const G2::A s = {Fq2Ops::from_mont(a.x), Fq2Ops::from_mont(a.y)};
  bn254_g2_affine_t p;
  memcpy(&p, &s, sizeof p);
  return p;
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
  const int malformed = walk_records(secs[10].count ? &secs[10] : nullptr, recs, &report->count, &bad);
  for (size_t i = 0; infos && i < recs.size() && i < infos_cap; i++) {
    memcpy(infos[i].after1, recs[i].after1, 64);
    memset(infos[i].name, 0, sizeof infos[i].name);
    memcpy(infos[i].name, recs[i].name, recs[i].name_len);
  }
  if (malformed) return fault(GROTH16_CONTRIB_SECTION, bad);

  const uint8_t* const hdr = L.sec[2]->p;
  const G1::A g1 = vb::g1_generator_mont();
  uint8_t h[32];
  chain_start(L, h);
  G1::A before = g1;
  for (uint32_t i = 0; i < report->count; i++) {
    const Record& r = recs[i];
    G1::A after, commitment;
    fe z;
    memcpy(&after, r.after1, 64);
    memcpy(&commitment, r.commitment, 64);
    memcpy(z.l, r.z, 32);
    const fe wa[2] = {after.x, after.y}, wc[2] = {commitment.x, commitment.y};
    if (p29::classify_g1(wa) || p29::classify_g1(wc) || G1::aff_is_zero(after)) return fault(GROTH16_CONTRIB_POINT, i + 1);
    fe c;
    chain_step(h, (const uint8_t*)&before, r, &c);
    if (!Fr::is_canonical(z)) return fault(GROTH16_CONTRIB_POK, i + 1);
    // z·before1 = R + c·after1, compared in the file's canonical affine form
    const G1::A lhs = zc29::zc_mul_affine<G1, G1L>(before, z);
    G1L::X acc = zc29::zc_scale<G1L>(after, zc29::zc_recode(c));
    if (!G1::aff_is_zero(commitment)) G1L::x_madd(acc, G1L::load_affine(commitment, G1L::MONT256, false));
    const G1::A rhs = G1::p_to_affine(G1::x_to_projective(G1L::x_store(acc)));
    if (memcmp(&lhs, &rhs, sizeof lhs) != 0) return fault(GROTH16_CONTRIB_POK, i + 1);
    before = after;
  }
  if (memcmp(&before, hdr + DELTA1_OFF, 64) != 0) return fault(GROTH16_CONTRIB_HEADER, 0);
  // e(δ₁, G₂) = e(G₁, δ₂); δ₁ is a point that has passed the lane test (or G₁), δ₂ gets its own
  G2::A d2;
  memcpy(&d2, hdr + DELTA2_OFF, 128);
  const fe2 w2[2] = {d2.x, d2.y};
  if (p29::classify_g2(w2) || G2::aff_is_zero(d2)) return fault(GROTH16_CONTRIB_PAIR, 0);
  if (!vb::pairing_eq(std_affine(before), vb::g2_generator_affine(), vb::g1_generator_affine(), std_affine(d2))) return fault(GROTH16_CONTRIB_PAIR, 0);
  return 1;
}
