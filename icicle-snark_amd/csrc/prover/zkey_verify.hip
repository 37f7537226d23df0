// zkey_verify.hip — groth16_zkey_verify_ptau: is a proving key the Groth16 key of an .r1cs over a .ptau?  (include/groth16_prover.h
// has the contract and the equations)
//
//   host      zkey_layout, ptau_layout, the sizes against the handle's, the ptau's power against the domain, then groth16_zkey_check
//             itself on the handle's device with this call's seed: its report is embedded, and nothing below runs on a key it faults
//             (but for a lone section-6/7 mismatch, which B1 and B2 resolve).
//             HEADER is three comparisons of stored words.  z (one coefficient per wire) and y (one per row of the domain) are made on
//             the worker pool.
//   rows      verify_split_kernel writes z^pub and z^priv; the witness check's kernel in its third mode (r1cs_emit_abc) evaluates
//             a, b, c at each; verify_assemble_kernel — one lane per row j < n — writes the eight scalar vectors of the right sides
//             with the public-binding rows and the zero tail applied.
//   ptau      block k of sections 12, 13, 14, 15 and block k + 1 of section 12 go up (nothing else of the file is touched) and
//             through ptau_g1_kernel / ptau_g2_kernel (ptau_ranges.h's PtauRanges: zkey_check29.h's tests, one lane per point);
//             odd_gather_kernel makes [L'_{2i+1}]₁ contiguous.
//   sums      six left sides with bitsize = 128 over the key's sections (uploaded here a second time: the key check keeps only 6 and
//             7 and frees them with its session), ten full-width right sides; bases in slices, partial sums added (device_call.h: sliced_msm).
//   verdict   A, B1, B2 as points; IC, C, H by two host pairings each.
#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "ptau_ranges.h"
#include "sha256.h"
#include "verify_batch.h"
#include "zkey_check29.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;

enum { V_A = 0, V_B, V_A_PUB, V_B_PUB, V_C_PUB, V_A_PRIV, V_B_PRIV, V_C_PRIV, N_VEC };

// z^pub = z on the wires 0 … n_public, 0 above; z^priv = z − z^pub.  One lane per wire.
__global__ __launch_bounds__(256) void verify_split_kernel(const fe* __restrict__ z, uint32_t n_wires, uint32_t n_public, fe* __restrict__ z_pub, fe* __restrict__ z_priv)
{
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_wires) return;
  const fe v = ld(z + s);
  const bool pub = s <= n_public;
  st(z_pub + s, pub ? v : Fr::zero());
  st(z_priv + s, pub ? Fr::zero() : v);
}

// Row j < n of the eight scalar vectors out[v·n + j] (standard form, the MSM's), from the rows pub[·], priv[·] = a | b | c at z^pub
// and z^priv (m each, r1cs_emit_abc's layout): below m the rows themselves and, for A and B at z, their sums; on the
// public-binding rows m … m + n_public (snarkjs adds them to A alone) z_{j−m} — a public wire, so it goes to a(z) and a(z^pub) —
// and 0 elsewhere; 0 above.  Fr::add takes canonical operands and returns one: the rows are sums out of r1cs_eval (canonical by
// add's reduction), z is below 2^128.
__global__ __launch_bounds__(256) void verify_assemble_kernel(const fe* __restrict__ pub, const fe* __restrict__ priv, const fe* __restrict__ z, uint32_t n, uint32_t m,
                                                               uint32_t n_public, fe* __restrict__ out)
{
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  fe v[N_VEC];
#pragma unroll
  for (int k = 0; k < N_VEC; k++) v[k] = Fr::zero();
  if (j < m) {
    v[V_A_PUB] = ld(pub + j), v[V_B_PUB] = ld(pub + (size_t)m + j), v[V_C_PUB] = ld(pub + 2 * (size_t)m + j);
    v[V_A_PRIV] = ld(priv + j), v[V_B_PRIV] = ld(priv + (size_t)m + j), v[V_C_PRIV] = ld(priv + 2 * (size_t)m + j);
    v[V_A] = Fr::add(v[V_A_PUB], v[V_A_PRIV]);
    v[V_B] = Fr::add(v[V_B_PUB], v[V_B_PRIV]);
  } else if (j - m <= n_public) {
    v[V_A] = v[V_A_PUB] = ld(z + (j - m));
  }
#pragma unroll
  for (int k = 0; k < N_VEC; k++) st(out + (size_t)k * n + j, v[k]);
}

// the device side of one call
struct Verify {
  const pv::ZkeyLayout& L;
  const pv::PtauLayout& PL;
  Groth16R1cs* const h;
  const pv::R1csShape shape;
  const uint32_t n, m, k; // the domain, the wires, log2 n
  const pv::FileRange zkey_file, ptau_file; // which mapped file the staging workers may pread() for a source pointer (the _file entry)
  isnark::vb::DeviceSession ds;
  double upload_ms = 0;

  Verify(const pv::ZkeyLayout& zl, const pv::PtauLayout& pl, Groth16R1cs* handle, uint32_t log_n, const pv::FileRange& zf, const pv::FileRange& pf)
      : L(zl), PL(pl), h(handle), shape(pv::r1cs_shape(handle)), n(zl.domain), m(zl.n_vars), k(log_n), zkey_file(zf), ptau_file(pf)
  {
  }

  template <class T>
  int alloc(T** p, size_t count)
  {
    *p = ds.buf.alloc<T>(std::max<size_t>(count, 1));
    return *p ? 0 : pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  }
  int upload(void* dst, const void* src, size_t bytes)
  {
    const pv::FileHint hint(zkey_file.holds(src) ? zkey_file : ptau_file.holds(src) ? ptau_file : pv::FileRange());
    return pv::timed_upload(shape.dev, dst, src, bytes, &upload_ms);
  }
  template <class T>
  int put(T** d, const void* src, size_t count)
  {
    if (int rc = alloc(d, count)) return rc;
    return upload(*d, src, count * sizeof(T));
  }
  // Σ scalars[i]·bases[i] over `count` Montgomery-form affine bases on the device, on the second stream; the group is out's
  template <class P>
  int sum(const fe* scalars, const uint8_t* bases, uint64_t count, int bitsize, P* out)
  {
    return pv::sliced_msm(pv::device_msm_config(ds.streams[1], bitsize), scalars, bases, count, out);
  }
};

int verify_impl(Groth16R1cs* h, const uint8_t* zkey, size_t zkey_len, const uint8_t* ptau, size_t ptau_len, const uint8_t* seed32, Groth16ZkeyVerifyReport* rep, int zkey_fd, int ptau_fd)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  std::vector<pv::Section> zsecs, psecs;
  pv::ZkeyLayout L;
  pv::PtauLayout PL;
  if (int rc = pv::zkey_layout(zkey, zkey_len, zsecs, &L)) return rc;
  if (int rc = pv::ptau_layout(ptau, ptau_len, psecs, &PL)) return rc;
  const pv::R1csShape shape = pv::r1cs_shape(h);
  // sizes, as groth16_r1cs_match_zkey
  uint32_t k;
  const uint64_t domain = pv::circuit_domain(shape.m, shape.n_public, &k);
  const bool size_ok[3] = {L.n_vars == shape.n_wires, L.n_public == shape.n_public, L.domain == domain};
  for (int i = 0; i < 3; i++)
    if (!size_ok[i]) {
      rep->kind = GROTH16_VERIFY_SIZES;
      rep->index = (uint64_t)i;
      return 0;
    }
  if (int rc = pv::ptau_blocks_for_domain(PL, k)) return rc;
  uint8_t seed[32];
  if (int rc = pv::seed_or_random(seed32, seed)) return rc;

  pv::StageTrace trace("zkey-verify", "ICICLE_SNARK_TRACE_ZKEY_VERIFY");

  // the key's own soundness first: the equations below mean nothing over points off their curves
  char device[32];
  snprintf(device, sizeof device, "HIP:%d", shape.dev);
  const Groth16ZkeyCheckOptions opt = {0, seed};
  const pv::FileRange zkey_file = {zkey, zkey_len, zkey_fd}, ptau_file = {ptau, ptau_len, ptau_fd};
  int key_rc;
  {
    const pv::FileHint hint(zkey_file);
    key_rc = groth16_zkey_check(zkey, zkey_len, device, &opt, &rep->key);
  }
  trace.lap("key check");
  if (key_rc < 0) return key_rc;
  // A mismatch of section 6 against 7 as the key's ONLY fault leaves every point where the sums are defined, and B1 and B2 below say
  // which of the two sections is not the circuit's: the equations run.  Any other fault ends the call here.
  uint64_t key_faults = 0;
  for (uint64_t f : rep->key.faults) key_faults += f;
  const bool only_b1_b2 = key_rc == 0 && rep->key.kind == GROTH16_ZKEY_PAIR_MISMATCH && rep->key.section == 6 && key_faults == 1;
  if (key_rc == 0 && !only_b1_b2) {
    rep->kind = GROTH16_VERIFY_KEY;
    return 0;
  }

  // HEADER: α₁, β₁, β₂ against the ptau's, as stored words (the key's are canonical by now)
  int32_t first_kind = 0;
  uint64_t first_index = 0;
  auto fault = [&](int32_t kind, uint64_t index) {
    rep->failed_mask |= 1u << (kind - GROTH16_VERIFY_HEADER);
    if (!first_kind) first_kind = kind, first_index = index;
  };
  const uint8_t* const hdr_ptau[3] = {PL.sec[4]->p, PL.sec[5]->p, PL.sec[6]->p};
  const size_t hdr_off[3] = {0, 64, 128}, hdr_len[3] = {64, 64, 128};
  for (int i = 0; i < 3; i++)
    if (memcmp(L.header_points + hdr_off[i], hdr_ptau[i], hdr_len[i]) != 0) fault(GROTH16_VERIFY_HEADER, (uint64_t)i);

  const uint32_t n = L.domain, m = L.n_vars, npub = L.n_public, nc = shape.m;
  // z_s = coefficient s, y_i = coefficient m + i: one vector, 128 bits each in 32-byte standard form
  std::vector<fe> zy((size_t)m + n);
  pv::fill_coefficients(seed, 0, zy.size(), zy.data());
  trace.lap("coefficients");

  std::lock_guard<std::mutex> lk(pv::r1cs_mutex(h));
  const auto t_dev = std::chrono::steady_clock::now();
  Verify c(L, PL, h, k, zkey_file, ptau_file);
  if (int rc = pv::open_session(c.ds, shape.dev, 2)) return rc;
  const hipStream_t st = c.ds.stream(0);

  // rows: z^pub, z^priv, a | b | c at each, the eight scalar vectors
  fe *d_zy, *d_zpub, *d_zpriv, *d_pub, *d_priv, *d_vec;
  PtauRanges ranges;
  if (int rc = c.put(&d_zy, zy.data(), zy.size())) return rc;
  if (int rc = c.alloc(&d_zpub, m)) return rc;
  if (int rc = c.alloc(&d_zpriv, m)) return rc;
  if (int rc = c.alloc(&d_pub, 3 * (size_t)nc)) return rc;
  if (int rc = c.alloc(&d_priv, 3 * (size_t)nc)) return rc;
  if (int rc = c.alloc(&d_vec, (size_t)N_VEC * n)) return rc;
  if (int rc = ranges.reset(c.ds, st)) return rc;
  DEV_LAUNCH("split kernel launch", verify_split_kernel, dim3((m + 255) / 256), dim3(256), st, d_zy, m, npub, d_zpub, d_zpriv);
  if (int rc = pv::r1cs_emit_abc(h, d_zpub, d_pub, st)) return rc;
  if (int rc = pv::r1cs_emit_abc(h, d_zpriv, d_priv, st)) return rc;
  DEV_LAUNCH("assemble kernel launch", verify_assemble_kernel, dim3((n + 255) / 256), dim3(256), st, d_pub, d_priv, d_zy, n, nc, npub, d_vec);

  // the ptau's ranges, each tested where it lands (both lane tests on this one stream), and [L'_{2i+1}]₁ made contiguous
  {
    const pv::FileHint hint(ptau_file);
    if (int rc = ranges.stage(PL, k, c.ds, shape.dev, st, st, &c.upload_ms)) return rc;
  }
  uint8_t* d_odd;
  if (int rc = c.alloc(&d_odd, (size_t)n * 64)) return rc;
  if (int rc = ranges.gather_odd(st, n, d_odd)) return rc;
  trace.lap("rows, ptau ranges");

  // the key's sections, a second time (the key check's session has freed them)
  const int key_sec[6] = {5, 6, 7, 8, 9, 3};
  const uint64_t key_cnt[6] = {m, m, m, (uint64_t)m - npub - 1, n, (uint64_t)npub + 1};
  uint8_t* d_key[6];
  for (int i = 0; i < 6; i++)
    if (int rc = c.put(&d_key[i], L.sec[key_sec[i]]->p, key_cnt[i] * (key_sec[i] == 7 ? 128 : 64))) return rc;
  trace.lap("key sections");

  unsigned long long first[PtauRanges::N];
  DEV_TRY("download", hipMemcpyAsync(first, ranges.d_first, sizeof first, hipMemcpyDeviceToHost, st));
  DEV_TRY("row and ptau kernels", hipStreamSynchronize(st));
  if (int rc = ranges.verdict(first)) return rc;
  trace.lap("kernels done");

  // left sides over 128-bit scalars, right sides full width
  const fe *d_z = d_zy, *d_y = d_zy + m;
  auto vec = [&](int v) { return d_vec + (size_t)v * n; };
  bn254_projective_t la, lb1, lic, lc, lh, ra, rb1, rh, ric[3], rc3[3];
  bn254_g2_projective_t lb2, rb2;
  int rc = c.sum(d_z, d_key[0], m, 128, &la);
  if (!rc) rc = c.sum(d_z, d_key[1], m, 128, &lb1);
  if (!rc) rc = c.sum(d_z, d_key[2], m, 128, &lb2);
  if (!rc) rc = c.sum(d_z + npub + 1, d_key[3], key_cnt[3], 128, &lc);
  if (!rc) rc = c.sum(d_y, d_key[4], n, 128, &lh);
  if (!rc) rc = c.sum(d_z, d_key[5], key_cnt[5], 128, &lic);
  trace.lap("left sides");
  if (!rc) rc = c.sum(vec(V_A), ranges.l1(), n, 0, &ra);
  if (!rc) rc = c.sum(vec(V_B), ranges.l1(), n, 0, &rb1);
  if (!rc) rc = c.sum(vec(V_B), ranges.l2(), n, 0, &rb2);
  const int pub_vec[3] = {V_A_PUB, V_B_PUB, V_C_PUB}, priv_vec[3] = {V_A_PRIV, V_B_PRIV, V_C_PRIV};
  const uint8_t* const t_blk[3] = {ranges.beta_l1(), ranges.alpha_l1(), ranges.l1()}; // a with [β·L]₁ (section 15), b with [α·L]₁ (section 14), c with [L]₁ (section 12)
  for (int i = 0; i < 3 && !rc; i++) {
    rc = c.sum(vec(pub_vec[i]), t_blk[i], n, 0, &ric[i]);
    if (!rc) rc = c.sum(vec(priv_vec[i]), t_blk[i], n, 0, &rc3[i]);
  }
  if (!rc) rc = c.sum(d_y, d_odd, n, 0, &rh);
  trace.lap("right sides");
  if (rc) return rc;
  rep->upload_ms = c.upload_ms;
  rep->device_ms = pv::ms_since(t_dev);

  const auto t_pair = std::chrono::steady_clock::now();
  bn254_projective_t t_ic = ric[0], t_c = rc3[0];
  for (int i = 1; i < 3; i++) {
    bn254_ecadd(&t_ic, &ric[i], &t_ic);
    bn254_ecadd(&t_c, &rc3[i], &t_c);
  }
  G2::A gm, dm;
  memcpy(&gm, L.header_points + 256, 128);
  memcpy(&dm, L.header_points + 448, 128);
  const G2::A gs = {Fq2Ops::from_mont(gm.x), Fq2Ops::from_mont(gm.y)}, dls = {Fq2Ops::from_mont(dm.x), Fq2Ops::from_mont(dm.y)};
  bn254_g2_affine_t gamma2, delta2;
  memcpy(&gamma2, &gs, sizeof gamma2);
  memcpy(&delta2, &dls, sizeof delta2);
  using isnark::vb::affine_or_zero;
  using isnark::vb::same_point;
  // e(S, Q) = e(T, G₂), Q a header point (not the identity: the key check has said so): the identity on both sides holds, on one fails
  const bn254_g2_affine_t g2 = isnark::vb::g2_generator_affine();
  auto pair_holds = [&](const bn254_projective_t& s, const bn254_g2_affine_t& q, const bn254_projective_t& t) {
    return isnark::vb::pairing_eq(affine_or_zero(s), q, affine_or_zero(t), g2);
  };
  if (!same_point(la, ra)) fault(GROTH16_VERIFY_A, 0);
  if (!same_point(lb1, rb1)) fault(GROTH16_VERIFY_B1, 0);
  if (!same_point(lb2, rb2)) fault(GROTH16_VERIFY_B2, 0);
  if (!pair_holds(lic, gamma2, t_ic)) fault(GROTH16_VERIFY_IC, 0);
  if (!pair_holds(lc, delta2, t_c)) fault(GROTH16_VERIFY_C, 0);
  if (!pair_holds(lh, delta2, rh)) fault(GROTH16_VERIFY_H, 0);
  rep->pairing_ms = pv::ms_since(t_pair);
  trace.lap("comparisons, pairings");
  if (!first_kind && key_rc == 0) first_kind = GROTH16_VERIFY_KEY; // (the key check's seeded test failed where B1 and B2 held)
  rep->kind = first_kind;
  rep->index = first_index;
  return first_kind ? 0 : 1;
}

} // namespace

ISNARK_API int groth16_zkey_verify_ptau(Groth16R1cs* h, const void* zkey, size_t zkey_len, const void* ptau, size_t ptau_len, const uint8_t* seed32, Groth16ZkeyVerifyReport* report)
{
  return verify_impl(h, (const uint8_t*)zkey, zkey_len, (const uint8_t*)ptau, ptau_len, seed32, report, -1, -1);
}

ISNARK_API int groth16_zkey_verify_ptau_file(Groth16R1cs* h, const char* zkey_path, const char* ptau_path, const uint8_t* seed32, Groth16ZkeyVerifyReport* report)
{
  if (!zkey_path || !ptau_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile zf, pf;
  if (int rc = zf.open_ro(zkey_path)) return rc;
  if (int rc = pf.open_ro(ptau_path, /*read_ahead=*/false)) return rc; // only the ranges that are read are touched
  return verify_impl(h, zf.data, zf.len, pf.data, pf.len, seed32, report, zf.fd, pf.fd);
}
