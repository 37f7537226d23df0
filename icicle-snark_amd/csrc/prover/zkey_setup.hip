// zkey_setup.hip — groth16_setup: the Groth16 proving key of a loaded circuit made DIRECTLY from toxic waste (τ, α, β, γ, δ) on one
// GPU, without a .ptau: what arkworks' generate_random_parameters, gnark's groth16.Setup and `snarkjs groth16 setup` make.  Whoever
// ran the call can forge proofs for the key.  include/groth16_prover.h has the contract; synth.key_scalars is the
// definition of every scalar.
//
//   host, first  the toxic waste through zs_toxic_check before any device work; zs_derive's shared values; the two tables of ω
//                (lo[i] = ω^i, hi[i] = ω^(i·2^k): 2^k + 2^(p−k) entries, never n).
//   transpose    zkey_columns.h's transpose_rows, shared with groth16_zkey_new: column lists and section 4's records.
//   lagrange     zs_lagrange_kernel: a lane per (row, j), j < n: row 0 is L_j(τ), row 1 is section 9's L_j(τ/g)·(τⁿ − 1)/(−2δ), written
//                straight into the G1 scalar array.  One Fermat inversion a lane.
//   columns      zs_plan_kernel: a lane per (matrix, wire) cuts a column of more than heavy_column_terms terms into items;
//                zs_columns_kernel: a lane per (matrix, wire) sums a light column in Fr; zs_item_kernel: a workgroup per item, each
//                lane a slice, then an LDS tree of Fr::add; zs_combine_kernel: a workgroup per heavy column adds its items.
//   outputs      zs_outputs_kernel: a lane per wire: a_s, b_s into A, B1, B2; comb_s = β·a_s + α·b_s + c_s times γ⁻¹ into IC (s ≤ npub)
//                or times δ⁻¹ into C.  G1 array: α, β, δ | IC | A | B1 | C | H; G2 array: β, γ, δ | B2 — standard form.
//   points       point_form.h's generator_mul_to_file_form over both arrays (G2 on the second stream): affine, Montgomery, the
//                identity — scalar 0: a wire in no matrix, a cancelling column — all zero bytes.
//   file         zkey_columns.h's FileLayout and write_key_frame; the arrays come down through the pinned staging.
//   Every device buffer that held a secret-derived scalar is overwritten before it is freed, the host's copies wiped on every way
//   out: best effort (the compiler may have kept copies in registers or spills; the points of the key are public).
#include <algorithm>
#include <chrono>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "point_form.h"
#include "prover_internal.h"
#include "verify_batch.h"
#include "zkey_columns.h"
#include "zkey_setup29.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;
using zs29::ZsDerived;

constexpr int ZS_WG = 256;
static const char* const TOXIC_NAMES[5] = {"tau", "alpha", "beta", "gamma", "delta"};

// what the Lagrange kernel reads: the two tables and, on the device (never in a kernel's arguments), zs_derive's values
struct LagrangeArgs {
  const ZsDerived* d;
  const fe *lo, *hi;
  uint32_t p, k;
};
// lane t < 2n: row t ≫ p, j = t mod n.  Row 0 to l0[j], row 1 to h[j].
__global__ __launch_bounds__(ZS_WG) void zs_lagrange_kernel(const LagrangeArgs a, fe* __restrict__ l0, fe* __restrict__ h)
{
  const uint64_t t = (uint64_t)blockIdx.x * ZS_WG + threadIdx.x;
  if (t >= (uint64_t)2 << a.p) return;
  const uint32_t row = (uint32_t)(t >> a.p), j = (uint32_t)(t & (((uint64_t)1 << a.p) - 1));
  const fe v = zs29::zs_lagrange(ld(a.d->x_mont + row), ld(a.hi + (j >> a.k)), ld(a.lo + (j & ((1u << a.k) - 1))), ld(a.d->c_std + row));
  st((row ? h : l0) + j, v);
}

// one lane per job mat·m + s: a column of more than thr terms is cut into items of thr terms.  heavy / items have room for every
// column that can be heavy and every item they can have (the host sizes them from the term total).
__global__ __launch_bounds__(ZS_WG) void zs_plan_kernel(Columns c, Counters* __restrict__ cnt, Heavy* __restrict__ heavy, Item* __restrict__ items)
{
  const uint64_t job64 = (uint64_t)blockIdx.x * ZS_WG + threadIdx.x;
  if (job64 >= 3 * (uint64_t)c.m) return;
  const uint32_t job = (uint32_t)job64;
  const uint32_t len = c.colptr[job + 1] - c.colptr[job];
  atomicMax(&cnt->longest, len);
  if (len <= c.thr) return;
  const uint32_t n_items = (len + c.thr - 1) / c.thr;
  const uint32_t slot = atomicAdd(&cnt->heavy[0], 1u), first = atomicAdd(&cnt->items[0], n_items);
  heavy[slot] = {job, first, n_items};
  for (uint32_t i = 0; i < n_items; i++) items[first + i] = {job, i * c.thr, min(len, (i + 1) * c.thr)};
}

// abc[mat·m + s] = Σ_j M[j, s]·L_j for a light column (an empty one: 0)
__global__ __launch_bounds__(ZS_WG) void zs_columns_kernel(Columns c, const fe* __restrict__ l0, fe* __restrict__ abc)
{
  const uint64_t job = (uint64_t)blockIdx.x * ZS_WG + threadIdx.x;
  if (job >= 3 * (uint64_t)c.m) return;
  const uint32_t lo = c.colptr[job], hi = c.colptr[job + 1];
  if (hi - lo > c.thr) return; // the item kernels'
  st(abc + job, zs29::zs_column_sum(c.entries, lo, hi, c.vals, l0));
}

// Σ over the workgroup's lanes, left in sh[0]
__device__ __forceinline__ void fr_tree_sum(fe* sh, const fe& mine)
{
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int half = ITEM_WG / 2; half; half >>= 1) {
    if ((int)threadIdx.x < half) sh[threadIdx.x] = Fr::add(sh[threadIdx.x], sh[threadIdx.x + half]);
    __syncthreads();
  }
}
// one workgroup per item: lane t sums the t-th slice of the item's positions
__global__ __launch_bounds__(ITEM_WG) void zs_item_kernel(Columns c, const Item* __restrict__ items, const fe* __restrict__ l0, fe* __restrict__ partial)
{
  __shared__ fe sh[ITEM_WG];
  const Item it = items[blockIdx.x];
  const uint32_t base = c.colptr[it.job];
  const uint32_t per = (it.hi - it.lo + ITEM_WG - 1) / ITEM_WG;
  const uint32_t lo = min(it.hi, it.lo + threadIdx.x * per), hi = min(it.hi, lo + per);
  fr_tree_sum(sh, zs29::zs_column_sum(c.entries + base, lo, hi, c.vals, l0));
  if (threadIdx.x == 0) st(partial + blockIdx.x, sh[0]);
}
// one workgroup per heavy column: its items' sums, added
__global__ __launch_bounds__(ITEM_WG) void zs_combine_kernel(const Heavy* __restrict__ heavy, const fe* __restrict__ partial, fe* __restrict__ abc)
{
  __shared__ fe sh[ITEM_WG];
  const Heavy h = heavy[blockIdx.x];
  fe acc = Fr::zero();
  for (uint32_t i = threadIdx.x; i < h.n_items; i += ITEM_WG) acc = Fr::add(acc, ld(partial + h.first + i));
  fr_tree_sum(sh, acc);
  if (threadIdx.x == 0) st(abc + h.job, sh[0]);
}

// where the scalars go: G1 array α, β, δ | IC | A | B1 | C | H, G2 array β, γ, δ | B2
struct ScalarLayout {
  uint64_t ic, a, b1, c, h, n1, b2, n2;
  ScalarLayout(uint64_t m, uint64_t npub, uint64_t n)
  {
    ic = 3, a = ic + npub + 1, b1 = a + m, c = b1 + m, h = c + (m - npub - 1), n1 = h + n;
    b2 = 3, n2 = b2 + m;
  }
};
// one lane per wire; lane 0 also writes the six head scalars
__global__ __launch_bounds__(ZS_WG) void zs_outputs_kernel(const ZsDerived* __restrict__ d, const fe* __restrict__ abc, uint32_t m, uint32_t npub, ScalarLayout sl,
                                                           fe* __restrict__ s1, fe* __restrict__ s2)
{
  const uint32_t s = blockIdx.x * ZS_WG + threadIdx.x;
  if (s >= m) return;
  if (s == 0) {
    for (int i = 0; i < 3; i++) {
      st(s1 + i, ld(d->head1 + i));
      st(s2 + i, ld(d->head2 + i));
    }
  }
  const fe a = ld(abc + s), b = ld(abc + (size_t)m + s), c = ld(abc + 2 * (size_t)m + s);
  st(s1 + sl.a + s, a);
  st(s1 + sl.b1 + s, b);
  st(s2 + sl.b2 + s, b);
  const fe comb = zs29::zs_comb(a, b, c, ld(&d->alpha_mont), ld(&d->beta_mont));
  if (s <= npub) st(s1 + sl.ic + s, zs29::zs_quot(comb, ld(&d->gamma_inv_mont)));
  else st(s1 + sl.c + (s - npub - 1), zs29::zs_quot(comb, ld(&d->delta_inv_mont)));
}

// everything secret of one call on the host; wiped on every way out (best effort)
struct Secrets {
  uint8_t toxic[160];
  ZsDerived d;
  ~Secrets()
  {
    explicit_bzero(toxic, sizeof toxic);
    explicit_bzero(&d, sizeof d);
  }
};
// the device buffers that held a secret-derived scalar: overwritten on every way out, before the session frees them
struct DeviceWipe {
  struct Range {
    void* p;
    size_t bytes;
  };
  std::vector<Range> ranges;
  hipStream_t st = nullptr;
  void add(void* p, size_t bytes) { ranges.push_back({p, bytes}); }
  ~DeviceWipe()
  {
    bool any = false;
    for (const Range& r : ranges)
      if (r.p && r.bytes && hipMemsetAsync(r.p, 0, r.bytes, st) == hipSuccess) any = true;
    if (any) (void)hipStreamSynchronize(st);
  }
};
// stage boundaries on a stream, read once both streams have drained
struct TimedEvent {
  hipEvent_t e = nullptr;
  int record(hipStream_t st)
  {
    if (!e) DEV_TRY("hipEventCreate", hipEventCreate(&e));
    DEV_TRY("hipEventRecord", hipEventRecord(e, st));
    return 0;
  }
  ~TimedEvent()
  {
    if (e) (void)hipEventDestroy(e);
  }
};
double between(const TimedEvent& a, const TimedEvent& b)
{
  float ms = 0;
  return hipEventElapsedTime(&ms, a.e, b.e) == hipSuccess ? (double)ms : 0.0;
}

using pv::Sink;

int toxic_fail(int kind, int which, uint32_t p)
{
  if (kind == zs29::ZS_RANGE) return pv::fail(pv::ERR_FORMAT, "toxic waste: %s is not below r", TOXIC_NAMES[which]);
  if (kind == zs29::ZS_ZERO) return pv::fail(pv::ERR_FORMAT, "toxic waste: %s is zero", TOXIC_NAMES[which]);
  return pv::fail(pv::ERR_FORMAT, "toxic waste: tau lies in the domain of order 2^%u or in its coset (tau^(2n) = 1): a Lagrange denominator vanishes", p);
}

int setup_impl(Groth16R1cs* h, const uint8_t* toxic160, const Groth16SetupOptions* opt, Groth16SetupReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  const pv::R1csShape shape = pv::r1cs_shape(h);
  const uint32_t m = shape.n_wires, npub = shape.n_public, nc = shape.m;
  if ((uint64_t)m < (uint64_t)npub + 1) return pv::fail(pv::ERR_FORMAT, "r1cs: %u wires cannot hold the constant and %u public signals", m, npub);
  uint32_t p;
  const uint64_t domain = pv::circuit_domain(nc, npub, &p);
  if (p > zs29::ZS_MAX_POWER) return pv::fail(pv::ERR_ARG, "the circuit's domain 2^%u is above 2^%u, the largest whose coset the field holds", p, zs29::ZS_MAX_POWER);
  const uint32_t n = (uint32_t)domain;
  rep->n_vars = m, rep->n_public = npub, rep->domain = n;
  const pv::R1csDeviceRows rows = pv::r1cs_device_rows(h);
  const uint64_t n_entries = rows.n_terms + npub + 1;
  if (3 * (uint64_t)m + 1 > 0xffffffffull || n_entries > 0xffffffffull) return pv::fail(pv::ERR_ARG, "the circuit's columns do not fit 32-bit offsets");

  // ---- the toxic waste, before any device work
  Secrets S;
  if (toxic160) {
    memcpy(S.toxic, toxic160, 160);
    int which;
    if (const int kind = zs29::zs_toxic_check(S.toxic, p, &which)) return toxic_fail(kind, which, p);
  } else {
    // the operating system's randomness, redrawn until valid: 254 bits a scalar, below r three times in four
    int tries = 0;
    for (;; tries++) {
      if (tries == 4096 || !vb::os_random(S.toxic, sizeof S.toxic)) return pv::fail(pv::ERR_ARG, "no randomness from the operating system (getrandom, /dev/urandom)");
      for (int i = 0; i < 5; i++) S.toxic[32 * i + 31] &= 0x3f;
      if (zs29::zs_toxic_check(S.toxic, p, nullptr) == zs29::ZS_OK) break;
    }
  }
  pv::StageTrace trace("zkey-setup", "ICICLE_SNARK_TRACE_ZKEY_SETUP");
  zs29::zs_derive(S.toxic, p, &S.d);
  const uint32_t kbits = zs29::zs_table_bits(p);
  const size_t n_lo = (size_t)1 << kbits, n_hi = (size_t)1 << (p - kbits);
  std::vector<fe> tables(n_lo + n_hi); // powers of ω: public
  isnark::run_ranges(n_lo, 1024, [&](int, size_t lo, size_t hi) { zs29::zs_fill_lo(p, lo, hi, tables.data()); });
  isnark::run_ranges(n_hi, 1024, [&](int, size_t lo, size_t hi) { zs29::zs_fill_hi(p, lo, hi, tables.data() + n_lo); });
  trace.lap("toxic waste, tables");

  const uint32_t thr = heavy_threshold(opt ? opt->heavy_column_terms : 0);
  const ScalarLayout SL(m, npub, n);

  std::lock_guard<std::mutex> lk(pv::r1cs_mutex(h));
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, shape.dev, 2)) return rc;
  const hipStream_t st = ds.stream(0), st2 = ds.stream(1);
  DeviceWipe wipe; // (declared behind the session: it runs before the session drains and frees)
  wipe.st = st;
  pv::Event ev_scalars;
  if (int rc = ev_scalars.create()) return rc;
  TimedEvent t0, t_lag, t_cols, t_g1, t_g2a, t_g2b;
  bool oom = false;
  auto alloc = [&](auto** ptr, size_t count) {
    typedef typename std::remove_pointer<typename std::remove_pointer<decltype(ptr)>::type>::type T;
    *ptr = ds.buf.alloc<T>(std::max<size_t>(count, 1));
    if (!*ptr) oom = true;
  };

  // ---- transpose, plan
  // a heavy column has more than thr terms, and all columns share n_entries of them
  const uint64_t cap_heavy = n_entries / thr + 1, cap_items = 2 * cap_heavy + 1;
  Transposed T;
  Counters* d_cnt;
  Heavy* d_heavy;
  Item* d_items;
  ZsDerived* d_derived;
  fe *d_tables, *d_l0, *d_abc, *d_s1, *d_s2;
  alloc(&d_cnt, 1);
  alloc(&d_heavy, (size_t)cap_heavy);
  alloc(&d_items, (size_t)cap_items);
  alloc(&d_derived, 1);
  alloc(&d_tables, tables.size());
  alloc(&d_l0, (size_t)n);
  alloc(&d_abc, 3 * (size_t)m);
  alloc(&d_s1, (size_t)SL.n1);
  alloc(&d_s2, (size_t)SL.n2);
  if (oom) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  wipe.add(d_derived, sizeof(ZsDerived));
  wipe.add(d_tables, tables.size() * sizeof(fe));
  wipe.add(d_l0, (size_t)n * sizeof(fe));
  wipe.add(d_abc, 3 * (size_t)m * sizeof(fe));
  wipe.add(d_s1, (size_t)SL.n1 * sizeof(fe));
  wipe.add(d_s2, (size_t)SL.n2 * sizeof(fe));
  DEV_TRY("hipMemset", hipMemsetAsync(d_cnt, 0, sizeof(Counters), st));
  if (int rc = transpose_rows(ds, st, rows, nc, m, npub, &T)) return rc;
  const Columns cols = T.columns(rows.d_vals, m, thr);
  DEV_LAUNCH("plan kernel launch", zs_plan_kernel, dim3((uint32_t)((3 * (uint64_t)m + ZS_WG - 1) / ZS_WG)), dim3(ZS_WG), st, cols, d_cnt, d_heavy, d_items);
  if (int rc = pv::timed_upload(shape.dev, d_derived, &S.d, sizeof(ZsDerived), &rep->upload_ms)) return rc;
  if (int rc = pv::timed_upload(shape.dev, d_tables, tables.data(), tables.size() * sizeof(fe), &rep->upload_ms)) return rc;
  trace.lap("session, transpose enqueued");

  // ---- what the host has to know before the file is sized: the record count, the heavy columns
  Counters cnt;
  uint32_t n_ab = 0;
  DEV_TRY("download", hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  DEV_TRY("download", hipMemcpyAsync(&n_ab, T.d_recoff + nc, 4, hipMemcpyDeviceToHost, st));
  DEV_TRY("transpose kernels", hipStreamSynchronize(st));
  trace.lap("transpose, plan");
  const uint64_t n_coeffs = (uint64_t)n_ab + npub + 1;
  const FileLayout F(m, npub, n, n_coeffs);
  rep->n_coeffs = n_coeffs;
  rep->zkey_bytes = F.total;
  rep->longest_column = cnt.longest;
  rep->heavy_columns = cnt.heavy[0];
  rep->heavy_items = cnt.items[0];
  if (cnt.heavy[0] > cap_heavy || cnt.items[0] > cap_items)
    return pv::fail(pv::ERR_DEVICE, "device: the heavy-column plan overran its bounds"); // (cannot happen: the bounds are sums of terms)
  uint8_t* out = nullptr;
  if (int rc = sink(F.total, &out)) return rc;

  // ---- scalars
  fe* d_partial;
  G1::X* d_t1;
  G2::X* d_t2;
  G1::P* d_p1;
  G2::P* d_p2;
  G1::A* d_a1;
  G2::A* d_a2;
  fe* d_i1;
  fe2* d_i2;
  alloc(&d_partial, (size_t)cnt.items[0]);
  alloc(&d_t1, pv::FIXED_BASE_TABLE_POINTS);
  alloc(&d_t2, pv::FIXED_BASE_TABLE_POINTS);
  alloc(&d_p1, (size_t)SL.n1);
  alloc(&d_p2, (size_t)SL.n2);
  alloc(&d_a1, (size_t)SL.n1);
  alloc(&d_a2, (size_t)SL.n2);
  alloc(&d_i1, (size_t)SL.n1);
  alloc(&d_i2, (size_t)SL.n2);
  if (oom) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  wipe.add(d_partial, (size_t)cnt.items[0] * sizeof(fe));
  if (int rc = t0.record(st)) return rc;
  const LagrangeArgs la = {d_derived, d_tables, d_tables + n_lo, p, kbits};
  DEV_LAUNCH("lagrange kernel launch", zs_lagrange_kernel, dim3((uint32_t)((2 * (uint64_t)n + ZS_WG - 1) / ZS_WG)), dim3(ZS_WG), st, la, d_l0, d_s1 + SL.h);
  if (int rc = t_lag.record(st)) return rc;
  DEV_LAUNCH("columns kernel launch", zs_columns_kernel, dim3((uint32_t)((3 * (uint64_t)m + ZS_WG - 1) / ZS_WG)), dim3(ZS_WG), st, cols, d_l0, d_abc);
  if (cnt.heavy[0]) {
    DEV_LAUNCH("item kernel launch", zs_item_kernel, dim3(cnt.items[0]), dim3(ITEM_WG), st, cols, d_items, d_l0, d_partial);
    DEV_LAUNCH("combine kernel launch", zs_combine_kernel, dim3(cnt.heavy[0]), dim3(ITEM_WG), st, d_heavy, d_partial, d_abc);
  }
  DEV_LAUNCH("outputs kernel launch", zs_outputs_kernel, dim3((m + ZS_WG - 1) / ZS_WG), dim3(ZS_WG), st, d_derived, d_abc, m, npub, SL, d_s1, d_s2);
  if (int rc = t_cols.record(st)) return rc;
  DEV_TRY("hipEventRecord", hipEventRecord(ev_scalars.e, st));
  DEV_TRY("hipStreamWaitEvent", hipStreamWaitEvent(st2, ev_scalars.e, 0));

  // ---- points: G2 on the second stream, beside G1
  if (int rc = t_g2a.record(st2)) return rc;
  if (int rc = pv::generator_mul_to_file_form<G2>(st2, d_s2, SL.n2, vb::g2_generator_mont(), d_t2, d_p2, d_a2, d_i2)) return rc;
  if (int rc = t_g2b.record(st2)) return rc;
  if (int rc = pv::generator_mul_to_file_form<G1>(st, d_s1, SL.n1, vb::g1_generator_mont(), d_t1, d_p1, d_a1, d_i1)) return rc;
  if (int rc = t_g1.record(st)) return rc;
  DEV_TRY("G1 kernels", hipStreamSynchronize(st));
  trace.lap("scalars, G1 points");
  DEV_TRY("G2 kernels", hipStreamSynchronize(st2));
  trace.lap("G2 points");
  rep->device_ms = pv::ms_since(t_dev);
  rep->lagrange_ms = between(t0, t_lag);
  rep->columns_ms = between(t_lag, t_cols);
  rep->g1_ms = between(t_cols, t_g1);
  rep->g2_ms = between(t_g2a, t_g2b);

  // ---- the file
  const auto t_down = std::chrono::steady_clock::now();
  const uint8_t *a1 = (const uint8_t*)d_a1, *a2 = (const uint8_t*)d_a2;
  uint8_t head1[3 * 64], head2[3 * 128]; // [α]₁ [β]₁ [δ]₁, [β]₂ [γ]₂ [δ]₂
  const isnark::CopyJob jobs[9] = {
    {head1, a1, sizeof head1},
    {head2, a2, sizeof head2},
    {out + F.off[3], a1 + SL.ic * 64, (size_t)F.len[3]},
    {out + F.off[4] + 4, T.d_rec, (size_t)(n_coeffs * pv::COEF_RECORD_BYTES)},
    {out + F.off[5], a1 + SL.a * 64, (size_t)F.len[5]},
    {out + F.off[6], a1 + SL.b1 * 64, (size_t)F.len[6]},
    {out + F.off[7], a2 + SL.b2 * 128, (size_t)F.len[7]},
    {out + F.off[8], a1 + SL.c * 64, (size_t)F.len[8]},
    {out + F.off[9], a1 + SL.h * 64, (size_t)F.len[9]},
  };
  DEV_TRY("device to host download", isnark::staged_copy(shape.dev, jobs, 9, false));
  rep->download_ms = pv::ms_since(t_down);
  write_key_frame(out, F, m, npub, n, n_coeffs, {head1, head1 + 64, head2, head2 + 128, head1 + 128, head2 + 256});
  trace.lap("download, header");
  return 0;
}

} // namespace

ISNARK_API int groth16_setup_toxic_check(const uint8_t* toxic160, uint32_t domain_power)
{
  if (!toxic160) return pv::fail(pv::ERR_ARG, "null toxic waste");
  if (domain_power > zs29::ZS_MAX_POWER) return pv::fail(pv::ERR_ARG, "domain power %u is above %u", domain_power, zs29::ZS_MAX_POWER);
  return zs29::zs_toxic_check(toxic160, domain_power, nullptr);
}

ISNARK_API int groth16_setup(Groth16R1cs* h, const uint8_t* toxic160, void* zkey_out, size_t cap, const Groth16SetupOptions* opt, Groth16SetupReport* report)
{
  return setup_impl(h, toxic160, opt, report, pv::buffer_sink("key", zkey_out, cap));
}

ISNARK_API int groth16_setup_file(Groth16R1cs* h, const uint8_t* toxic160, const char* zkey_path, const Groth16SetupOptions* opt, Groth16SetupReport* report)
{
  if (!zkey_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::TempOutput to(zkey_path); // a failed call leaves nothing there
  int rc = setup_impl(h, toxic160, opt, report, [&](uint64_t bytes, uint8_t** out) { return to.open(bytes, out); });
  const auto t_write = std::chrono::steady_clock::now();
  rc = to.finish(rc);
  if (rc == 0 && report) report->write_ms = pv::ms_since(t_write);
  return rc;
}
