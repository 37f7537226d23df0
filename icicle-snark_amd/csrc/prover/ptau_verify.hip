// ptau_verify.hip — groth16_ptau_verify: are sections 2 … 6 of a powers-of-tau file the powers of one (τ, α, β), and — when the file
// is prepared — are sections 12 … 15 the inverse transforms of 2 … 5 that groth16_ptau_prepare and snarkjs write?
// include/groth16_prover.h has the contract and the equations; ptau_verify29.h the scalars of the Lagrange equations; DESIGN.md §7i.
//
//   host, first  the container in either form (ptau_either_layout), section 6 through the lane test; x, y, μ_p, C, T (pv_derive) and
//                the four small tables lo[j] = y^j, hi[m] = y·y^(m·2^k), lo[j] = Ω^j, hi[m] = Ω^(m·2^k); ρ_i on the worker pool while
//                section 2 goes up.
//   device       pair by pair — (2, 12), (3, 13), (4, 14), (5, 15): the pair goes up and through ptau_ranges.h's lane tests (the G2
//                sections with the subgroup test), the source also through pv_identity_kernel; the verdicts are read before any sum
//                sees a point.  L = Σ ρ_i·S_i and R = Σ ρ_i·S_{i+1} over 128-bit scalars (R's base pointer is one element on); for
//                a prepared file Σ λ_e·B_e and Σ d_i·S_i at full width.  The pair's buffers are freed before the next pair goes
//                up: no more than one pair is resident.
//                λ_e is a function of (e, power) alone and section 12 is the longest, so pv_lagrange_scalars_kernel runs ONCE, over
//                section 12's 4N − 1 elements, and the other three sections read a prefix of its output; d_i depends on pmax, so
//                pv_power_scalars_kernel runs for section 2 (pmax = power + 1) and once more for 3 … 5 (pmax = power).
//   host, last   the stored words of the generators, six equations by pairing_eq (twelve pairings), four by same_point.
// No (bases, count) of one MSM recurs in another, and the bases are DevBuf's plain hipMalloc, which the runtime does not track:
// bn254_msm's automatic fixed-base table (msm_plan.h) is never looked up, let alone built.  The NTT domain is not touched.
#include <algorithm>
#include <chrono>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "ptau_ranges.h"
#include "ptau_verify29.h"
#include "verify_batch.h"
#include "zkey_check29.h"

using namespace bn254;
using bn254::pv29::PvBlockTable;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int PV_WG = 256;

// out[i] = d_i = y^(i+1)·T[q(i)], i < n, standard form.  lo[j] = y^j for j < 2^k, hi[m] = y·y^(m·2^k) for m ≤ (n − 1) ≫ k, Montgomery
// form: the host sizes hi for 2^(power+1) indices, n is at most 2^(power+1) − 1.
struct PowerArgs {
  const fe *lo, *hi;
  uint32_t k;
  uint64_t n;
  PvBlockTable t; // standard form
};
__global__ __launch_bounds__(PV_WG) void pv_power_scalars_kernel(const PowerArgs a, fe* __restrict__ out)
{
  const uint64_t i = (uint64_t)blockIdx.x * PV_WG + threadIdx.x;
  if (i >= a.n) return;
  st(out + i, pv29::pv_power_scalar(ld(a.hi + (i >> a.k)), ld(a.lo + (i & (((uint64_t)1 << a.k) - 1))), a.t.v[pv29::pv_first_block_over(i)]));
}

// out[e] = λ_e = C[p]·(x − Ω^t)⁻¹, e < n ≤ 2^(power+2) − 1, standard form.  lo[j] = Ω^j for j < 2^k, hi[m] = Ω^(m·2^k) for
// m < 2^(power+1−k), Montgomery form: t = j·2^(power+1−p) < 2^(power+1) for every e.  One Fermat inversion per lane: the exponent
// r − 2 is the same in every lane, so the walk is uniform over the wave.
struct LagrangeArgs {
  const fe *lo, *hi;
  uint32_t k, power;
  uint64_t n;
  fe x; // Montgomery form
  PvBlockTable c; // standard form
};
__global__ __launch_bounds__(PV_WG) void pv_lagrange_scalars_kernel(const LagrangeArgs a, fe* __restrict__ out)
{
  const uint64_t e = (uint64_t)blockIdx.x * PV_WG + threadIdx.x;
  if (e >= a.n) return;
  uint32_t p;
  const uint64_t t = pv29::pv_lagrange_exponent(e, a.power, &p);
  st(out + e, pv29::pv_lagrange_scalar(a.x, ld(a.hi + (t >> a.k)), ld(a.lo + (t & (((uint64_t)1 << a.k) - 1))), a.c.v[p]));
}

// the identity (all-zero words) among cnt points of ROW uint4 each: min over the lanes that hold one of their index
template <int ROW>
__global__ __launch_bounds__(PV_WG) void pv_identity_kernel(const uint4* __restrict__ pts, uint64_t cnt, unsigned long long* __restrict__ first)
{
  const uint64_t i = (uint64_t)blockIdx.x * PV_WG + threadIdx.x;
  if (i >= cnt) return;
  uint32_t any = 0;
#pragma unroll
  for (int w = 0; w < ROW; w++) {
    const uint4 v = pts[i * ROW + w];
    any |= v.x | v.y | v.z | v.w;
  }
  if (!any) atomicMin(first, (unsigned long long)i);
}

// a Montgomery-form point of the file as the host pairing takes it
bn254_affine_t std_g1(const uint8_t* p)
{
  G1::A a;
  memcpy(&a, p, sizeof a);
  const G1::A s = {Fq::from_mont(a.x), Fq::from_mont(a.y)};
  bn254_affine_t o;
  memcpy(&o, &s, sizeof o);
  return o;
}
bn254_g2_affine_t std_g2(const uint8_t* p)
{
  G2::A a;
  memcpy(&a, p, sizeof a);
  const G2::A s = {Fq2Ops::from_mont(a.x), Fq2Ops::from_mont(a.y)};
  bn254_g2_affine_t o;
  memcpy(&o, &s, sizeof o);
  return o;
}

enum { F_POINT_SRC = 0, F_IDENT_SRC, F_POINT_PREP, N_FIRST };

int verify_impl(const uint8_t* data, size_t len, const uint8_t* seed32, const char* device, Groth16PtauVerifyReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  bool prepared = false;
  if (int rc = pv::ptau_either_layout(data, len, secs, &L, &prepared)) return rc;
  const uint32_t power = L.power;
  const uint64_t N = (uint64_t)1 << power;
  const uint64_t src_cnt[4] = {2 * N - 1, N, N, N};
  rep->power = power;
  rep->prepared = prepared ? 1 : 0;
  for (int k4 = 0; k4 < 4; k4++) {
    rep->points[k4] = src_cnt[k4];
    rep->points[4 + k4] = prepared ? pv::ptau_prepared_section_bytes(power, 12 + k4) / (k4 == 1 ? 128 : 64) : 0;
  }
  uint8_t seed[32];
  if (int rc = pv::seed_or_random(seed32, seed)) return rc;
  // a faulty point is a verdict: nothing below it has been summed, the mask says nothing
  auto fault = [&](int32_t kind, int section, uint64_t element, int point_kind) {
    rep->kind = kind, rep->failed_mask = 0;
    rep->fault_section = section, rep->fault_index = element, rep->fault_kind = point_kind;
    return 0;
  };
  {
    fe2 beta2[2];
    memcpy(beta2, L.sec[6]->p, 128);
    if (const int kind = p29::classify_g2(beta2)) return fault(GROTH16_PTAU_VERIFY_POINT, 6, 0, kind);
    if (vb::words_zero(beta2, sizeof beta2)) return fault(GROTH16_PTAU_VERIFY_IDENTITY, 6, 0, 0);
  }

  pv::StageTrace trace("ptau-verify", "ICICLE_SNARK_TRACE_PTAU_VERIFY");
  // ---- x, y, μ_p, C, T; the tables of y and of Ω, Montgomery form: lo_y ‖ hi_y ‖ lo_Ω ‖ hi_Ω
  pv29::PvDerived D;
  const uint32_t kbits = pc29::pc_table_bits(power);
  const size_t n_lo = (size_t)1 << kbits, n_hi = (size_t)1 << (power + 1 - kbits);
  std::vector<fe> tables;
  if (prepared) {
    pv29::pv_derive(seed, power, &D);
    bn254_scalar_t rou;
    if (bn254_get_root_of_unity((uint64_t)2 << power, &rou) != ICICLE_SUCCESS) return pv::fail(pv::ERR_ARG, "ptau: no root of unity of order 2^%u", power + 1);
    fe w;
    memcpy(w.l, &rou, 32);
    tables.resize(2 * (n_lo + n_hi));
    const fe one_m = Fr::one_mont(), base_m[2] = {D.y_mont, Fr::to_mont(w)}, start_hi[2] = {D.y_mont, one_m};
    for (int which = 0; which < 2; which++) {
      fe* const t = tables.data() + which * (n_lo + n_hi);
      const fe step_m = pc29::pc_pow(base_m[which], n_lo);
      isnark::run_ranges(n_lo, 1024, [&](int, size_t lo, size_t hi) { pc29::pc_fill_powers(base_m[which], one_m, lo, hi, t); });
      isnark::run_ranges(n_hi, 1024, [&](int, size_t lo, size_t hi) { pc29::pc_fill_powers(step_m, start_hi[which], lo, hi, t + n_lo); });
    }
  }
  trace.lap("layout, derived values, tables");

  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (ds.open(dev, 1)) return pv::fail(pv::ERR_DEVICE, "%s", groth16_verify_last_error());
  const hipStream_t st = ds.stream(0);
  // what stays for the whole call: ρ, and for a prepared file λ, d and the tables
  const uint64_t n_rho = std::max<uint64_t>(2 * N - 2, 1), n_lambda = 4 * N - 1, n_d = 2 * N - 1;
  fe* const d_rho = ds.buf.alloc<fe>((size_t)n_rho);
  unsigned long long* const d_first = ds.buf.alloc<unsigned long long>(N_FIRST);
  fe *d_lambda = nullptr, *d_d = nullptr, *d_tables = nullptr;
  if (prepared) {
    d_lambda = ds.buf.alloc<fe>((size_t)n_lambda);
    d_d = ds.buf.alloc<fe>((size_t)n_d);
    d_tables = ds.buf.alloc<fe>(tables.size());
  }
  if (!d_rho || !d_first || (prepared && (!d_lambda || !d_d || !d_tables))) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  const fe *d_lo_y = d_tables, *d_hi_y = d_tables + n_lo, *d_lo_w = d_tables + n_lo + n_hi, *d_hi_w = d_tables + 2 * n_lo + n_hi;
  if (prepared) {
    if (int rc = pv::timed_upload(dev, d_tables, tables.data(), tables.size() * sizeof(fe), &rep->upload_ms)) return rc;
    LagrangeArgs la;
    la.lo = d_lo_w, la.hi = d_hi_w, la.k = kbits, la.power = power, la.n = n_lambda, la.x = D.x_mont, la.c = D.c;
    DEV_LAUNCH("lagrange scalars kernel launch", pv_lagrange_scalars_kernel, dim3((uint32_t)((n_lambda + PV_WG - 1) / PV_WG)), dim3(PV_WG), st, la, d_lambda);
  }

  bn254_projective_t l1[4], r1[4], lag_l1[4], lag_r1[4];
  bn254_g2_projective_t l2, r2, lag_l2, lag_r2;
  memset(l1, 0, sizeof l1), memset(r1, 0, sizeof r1), memset(lag_l1, 0, sizeof lag_l1), memset(lag_r1, 0, sizeof lag_r1);
  memset(&l2, 0, sizeof l2), memset(&r2, 0, sizeof r2), memset(&lag_l2, 0, sizeof lag_l2), memset(&lag_r2, 0, sizeof lag_r2);
  std::vector<fe> rho((size_t)n_rho);
  for (int k4 = 0; k4 < 4; k4++) {
    const int src_id = 2 + k4, prep_id = 12 + k4;
    const bool g2 = k4 == 1;
    const size_t elem = g2 ? 128 : 64;
    const uint64_t n_src = src_cnt[k4], n_prep = rep->points[4 + k4];
    vb::DevBuf pair; // freed at the end of this turn: one pair resident
    uint8_t* const d_src = pair.alloc<uint8_t>((size_t)(n_src * elem));
    uint8_t* const d_prep = prepared ? pair.alloc<uint8_t>((size_t)(n_prep * elem)) : nullptr;
    if (!d_src || (prepared && !d_prep)) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
    int up_rc = 0;
    const auto upload_src = [&]() { up_rc = pv::timed_upload(dev, d_src, L.sec[src_id]->p, (size_t)(n_src * elem), &rep->upload_ms); };
    if (k4 == 0) {
      // ρ_i, one vector for the four sections, on the worker pool while section 2 goes up
      pv::fill_coefficients(seed, 0, (size_t)n_rho, rho.data(), upload_src);
      if (up_rc) return up_rc;
      if (int rc = pv::timed_upload(dev, d_rho, rho.data(), (size_t)n_rho * sizeof(fe), &rep->upload_ms)) return rc;
    } else {
      upload_src();
      if (up_rc) return up_rc;
    }
    DEV_TRY("hipMemset", hipMemsetAsync(d_first, 0xff, N_FIRST * sizeof *d_first, st));
    const auto lane_test = [&](const uint8_t* pts, uint64_t n, unsigned long long* first) -> int {
      if (g2) DEV_LAUNCH("ptau membership kernel launch", ptau_g2_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), st, (const fe2*)pts, (uint32_t)n, first);
      else DEV_LAUNCH("ptau membership kernel launch", ptau_g1_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), st, (const fe*)pts, (uint32_t)n, first);
      return 0;
    };
    if (int rc = lane_test(d_src, n_src, d_first + F_POINT_SRC)) return rc;
    {
      const dim3 grid((uint32_t)((n_src + PV_WG - 1) / PV_WG));
      if (g2) DEV_LAUNCH("identity kernel launch", pv_identity_kernel<8>, grid, dim3(PV_WG), st, (const uint4*)d_src, n_src, d_first + F_IDENT_SRC);
      else DEV_LAUNCH("identity kernel launch", pv_identity_kernel<4>, grid, dim3(PV_WG), st, (const uint4*)d_src, n_src, d_first + F_IDENT_SRC);
    }
    uint64_t n_full = 0; // the source elements the Lagrange equation sums
    if (prepared) {
      if (int rc = pv::timed_upload(dev, d_prep, L.sec[prep_id]->p, (size_t)(n_prep * elem), &rep->upload_ms)) return rc;
      if (int rc = lane_test(d_prep, n_prep, d_first + F_POINT_PREP)) return rc;
      n_full = std::min<uint64_t>(n_src, (uint64_t)1 << (k4 == 0 ? power + 1 : power));
      if (k4 < 2) { // d for pmax = power + 1, then for pmax = power: sections 4 and 5 read section 3's
        PowerArgs pa;
        pa.lo = d_lo_y, pa.hi = d_hi_y, pa.k = kbits, pa.n = n_full, pa.t = k4 == 0 ? D.t12 : D.t13;
        DEV_LAUNCH("power scalars kernel launch", pv_power_scalars_kernel, dim3((uint32_t)((n_full + PV_WG - 1) / PV_WG)), dim3(PV_WG), st, pa, d_d);
      }
    }
    unsigned long long first[N_FIRST];
    DEV_TRY("download", hipMemcpyAsync(first, d_first, sizeof first, hipMemcpyDeviceToHost, st));
    DEV_TRY("lane tests", hipStreamSynchronize(st));
    if (trace.on) {
      char what[40];
      snprintf(what, sizeof what, "pair %d: up, lane tests", src_id);
      trace.lap(what);
    }
    // the source first, a faulty point before an identity; then the prepared section
    if (first[F_POINT_SRC] != NO_FAULT) return fault(GROTH16_PTAU_VERIFY_POINT, src_id, first[F_POINT_SRC] >> 3, (int)(first[F_POINT_SRC] & 7));
    if (first[F_IDENT_SRC] != NO_FAULT) return fault(GROTH16_PTAU_VERIFY_IDENTITY, src_id, first[F_IDENT_SRC], 0);
    if (first[F_POINT_PREP] != NO_FAULT) return fault(GROTH16_PTAU_VERIFY_POINT, prep_id, first[F_POINT_PREP] >> 3, (int)(first[F_POINT_PREP] & 7));

    const MSMConfig narrow = pv::device_msm_config(ds.streams[0], 128), full = pv::device_msm_config(ds.streams[0], 0);
    int rc;
    if (g2) {
      rc = pv::sliced_msm(narrow, d_rho, d_src, n_src - 1, &l2);
      if (!rc) rc = pv::sliced_msm(narrow, d_rho, d_src + elem, n_src - 1, &r2);
      if (!rc && prepared) rc = pv::sliced_msm(full, d_lambda, d_prep, n_prep, &lag_l2);
      if (!rc && prepared) rc = pv::sliced_msm(full, d_d, d_src, n_full, &lag_r2);
    } else {
      rc = pv::sliced_msm(narrow, d_rho, d_src, n_src - 1, &l1[k4]);
      if (!rc) rc = pv::sliced_msm(narrow, d_rho, d_src + elem, n_src - 1, &r1[k4]);
      if (!rc && prepared) rc = pv::sliced_msm(full, d_lambda, d_prep, n_prep, &lag_l1[k4]);
      if (!rc && prepared) rc = pv::sliced_msm(full, d_d, d_src, n_full, &lag_r1[k4]);
    }
    if (rc) return rc;
    DEV_TRY("sums", hipStreamSynchronize(st));
    if (trace.on) {
      char what[40];
      snprintf(what, sizeof what, "pair %d: sums", src_id);
      trace.lap(what);
    }
  }
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;

  // ---- the verdict: stored words, pairings, comparisons — every equation, whatever failed first
  const auto t_pair = std::chrono::steady_clock::now();
  uint32_t mask = 0;
  auto failed = [&](int32_t kind) { mask |= 1u << (kind - GROTH16_PTAU_VERIFY_GENERATORS); };
  const G1::A g1m = vb::g1_generator_mont();
  const G2::A g2m = vb::g2_generator_mont();
  const bn254_affine_t g1 = vb::g1_generator_affine();
  const bn254_g2_affine_t g2 = vb::g2_generator_affine();
  using vb::affine_or_zero;
  if (memcmp(L.sec[2]->p, &g1m, 64) != 0 || memcmp(L.sec[3]->p, &g2m, 128) != 0) failed(GROTH16_PTAU_VERIFY_GENERATORS);
  if (!vb::pairing_eq(std_g1(L.sec[5]->p), g2, g1, std_g2(L.sec[6]->p))) failed(GROTH16_PTAU_VERIFY_BETA_PAIR);
  if (power >= 1) {
    const bn254_affine_t tau1 = std_g1(L.sec[2]->p + 64);
    const bn254_g2_affine_t tau2 = std_g2(L.sec[3]->p + 128);
    // (Y, X = τ₂·Y) in G1, for section 3's equation: (G₁, τ₁) when TAU_PAIR says so, else (L, R) of the first G1 section whose own
    // equation holds — that equation IS R = τ₂·L
    bn254_affine_t y1 = g1, x1 = tau1;
    bool have_ratio = vb::pairing_eq(tau1, g2, g1, tau2);
    if (!have_ratio) failed(GROTH16_PTAU_VERIFY_TAU_PAIR);
    const int32_t g1_kind[4] = {GROTH16_PTAU_VERIFY_TAU_G1, 0, GROTH16_PTAU_VERIFY_ALPHA_TAU, GROTH16_PTAU_VERIFY_BETA_TAU};
    for (int k4 = 0; k4 < 4; k4++) {
      if (k4 == 1) continue;
      const bn254_affine_t l = affine_or_zero(l1[k4]), r = affine_or_zero(r1[k4]);
      if (!vb::pairing_eq(l, tau2, r, g2)) failed(g1_kind[k4]);
      else if (!have_ratio && !vb::words_zero(&l, sizeof l)) y1 = l, x1 = r, have_ratio = true;
    }
    if (!have_ratio || !vb::pairing_eq(x1, affine_or_zero(l2), y1, affine_or_zero(r2))) failed(GROTH16_PTAU_VERIFY_TAU_G2);
  }
  if (prepared) {
    for (int k4 = 0; k4 < 4; k4++)
      if (!(k4 == 1 ? vb::same_point(lag_l2, lag_r2) : vb::same_point(lag_l1[k4], lag_r1[k4]))) failed(GROTH16_PTAU_VERIFY_LAGRANGE_12 + k4);
  }
  rep->pairing_ms = pv::ms_since(t_pair);
  trace.lap("words, pairings, comparisons");
  rep->failed_mask = mask;
  rep->kind = mask ? GROTH16_PTAU_VERIFY_GENERATORS + __builtin_ctz(mask) : 0;
  return mask ? 0 : 1;
}

} // namespace

ISNARK_API int groth16_ptau_verify(const void* ptau, size_t len, const uint8_t* seed32, const char* device, Groth16PtauVerifyReport* report)
{
  return verify_impl((const uint8_t*)ptau, len, seed32, device, report);
}

ISNARK_API int groth16_ptau_verify_file(const char* path, const uint8_t* seed32, const char* device, Groth16PtauVerifyReport* report)
{
  if (!path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile mf;
  if (int rc = mf.open_ro(path)) return rc;
  const pv::FileHint hint(mf.data, mf.len, mf.fd); // (the staging workers pread() the file instead of copying out of the mapping)
  return verify_impl(mf.data, mf.len, seed32, device, report);
}
