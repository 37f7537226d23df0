// zkey_new.hip — groth16_zkey_new: the Groth16 proving key of an .r1cs over a prepared .ptau, before any phase-2 contribution
// (γ = δ = 1; what `snarkjs zkey new` writes, without its circuit hash).  include/groth16_prover.h has the contract and the file's
// layout; DESIGN.md §7e.
//
//   transpose   zkey_columns.h's transpose_rows (shared with groth16_setup): the handle's rows become column lists, one per
//               (matrix, wire), and section 4's records are written.  The order inside a column is whatever the atomics gave: the
//               sums do not depend on it, and the affine bytes that leave are canonical.
//   ptau        block k of sections 12, 13, 14, 15 and block k + 1 of section 12 go up and through ptau_g1_kernel / ptau_g2_kernel
//               (ptau_ranges.h's PtauRanges), as groth16_zkey_verify_ptau stages them; odd_gather_kernel makes section 9.
//   columns     zn_g1_kernel: one lane per (output, wire) for A_s, B1_s and comb_s; zn_g2_kernel: one lane per wire for B2_s — a
//               kernel of its own, so that G2's registers do not set G1's occupancy.  Each lane walks its column through
//               zkey_new29.h's zn_walk in lazy XYZZ registers.  A column of more than heavy_column_terms terms is left out: the
//               plan kernel has cut it into items of that many terms, zn_item_kernel sums an item with one workgroup (each lane a
//               slice, then an LDS tree of x_add), and zn_combine_kernel adds a column's items the same way.
//   output      projective sums → point_form.h's to_file_form (G2's on the second stream), the identity kept as zeros, and down
//               into the caller's buffer or the mapped output file through the pinned staging.
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
#include "ptau_ranges.h"
#include "verify_batch.h"
#include "zkey_columns.h"
#include "zkey_new29.h"

using namespace bn254;
using bn254::zn29::ZnList;

namespace {

namespace pv = isnark::prover;

// G1 job o·m + s: o = 0 A_s, 1 B1_s, 2 comb_s; the G2 job s: B2_s
enum { OUT_A = 0, OUT_B1 = 1, OUT_COMB = 2, G1_OUTPUTS = 3 };
__device__ __forceinline__ ZnList<G1L> list_of(const Columns& c, int mat, uint32_t s, const G1::A* bases)
{
  const uint32_t lo = c.colptr[(size_t)mat * c.m + s];
  return {c.entries + lo, c.colptr[(size_t)mat * c.m + s + 1] - lo, bases};
}
// the lists of a G1 job: A and B1 read one column against [L]₁ (the other two lists stay empty), comb all three
struct G1Job {
  ZnList<G1L> ls[3];
  uint32_t len;
};
__device__ __forceinline__ G1Job g1_job(const Columns& c, uint32_t job, const G1::A* l, const G1::A* al, const G1::A* bl)
{
  const uint32_t o = job / c.m, s = job - o * c.m;
  G1Job j;
  const ZnList<G1L> none = {c.entries, 0, l};
  if (o == OUT_COMB) {
    j.ls[0] = list_of(c, 0, s, bl);
    j.ls[1] = list_of(c, 1, s, al);
    j.ls[2] = list_of(c, 2, s, l);
  } else {
    j.ls[0] = list_of(c, (int)o, s, l);
    j.ls[1] = none;
    j.ls[2] = none;
  }
  j.len = j.ls[0].len + j.ls[1].len + j.ls[2].len;
  return j;
}
__device__ __forceinline__ ZnList<G2L> g2_job(const Columns& c, uint32_t s, const G2::A* l2)
{
  const uint32_t lo = c.colptr[(size_t)c.m + s];
  return {c.entries + lo, c.colptr[(size_t)c.m + s + 1] - lo, l2};
}

// one lane per job: a job of more than thr terms is cut into items of thr terms.  heavy / items have room for every job that can
// be heavy and every item they can have (the host sizes them from the term total).
template <bool G2_JOBS>
__global__ __launch_bounds__(256) void zn_plan_kernel(Columns c, Counters* __restrict__ cnt, Heavy* __restrict__ heavy, Item* __restrict__ items)
{
  const uint64_t job64 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (job64 >= (uint64_t)(G2_JOBS ? 1 : G1_OUTPUTS) * c.m) return;
  const uint32_t job = (uint32_t)job64;
  uint32_t len;
  if (G2_JOBS) {
    len = c.colptr[(size_t)c.m + job + 1] - c.colptr[(size_t)c.m + job];
  } else {
    const uint32_t o = job / c.m, s = job - o * c.m;
    if (o == OUT_COMB) {
      const uint32_t lc = c.colptr[2 * (size_t)c.m + s + 1] - c.colptr[2 * (size_t)c.m + s];
      len = lc + (c.colptr[s + 1] - c.colptr[s]) + (c.colptr[(size_t)c.m + s + 1] - c.colptr[(size_t)c.m + s]);
      atomicMax(&cnt->longest, lc);
    } else {
      len = c.colptr[(size_t)o * c.m + s + 1] - c.colptr[(size_t)o * c.m + s];
      atomicMax(&cnt->longest, len);
    }
  }
  if (len <= c.thr) return;
  const uint32_t n_items = (len + c.thr - 1) / c.thr;
  const uint32_t slot = atomicAdd(&cnt->heavy[G2_JOBS], 1u), first = atomicAdd(&cnt->items[G2_JOBS], n_items);
  heavy[slot] = {job, first, n_items};
  for (uint32_t i = 0; i < n_items; i++) items[first + i] = {job, i * c.thr, min(len, (i + 1) * c.thr)};
}

template <class C, class CL>
__device__ __forceinline__ void store_sum(typename C::P* out, const typename CL::X& x)
{
  *out = C::x_to_projective(CL::x_store(x)); // Montgomery-256 projective, the identity (0, 1, 0)
}

__global__ __launch_bounds__(64) void zn_g1_kernel(Columns c, const G1::A* __restrict__ l, const G1::A* __restrict__ al, const G1::A* __restrict__ bl, G1::P* __restrict__ out)
{
  const uint64_t job = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (job >= (uint64_t)G1_OUTPUTS * c.m) return;
  const G1Job j = g1_job(c, (uint32_t)job, l, al, bl);
  if (j.len > c.thr) return; // the item kernels'
  store_sum<G1, G1L>(out + job, zn29::zn_walk<G1L, 3>(j.ls, c.vals, 0, j.len));
}
__global__ __launch_bounds__(64) void zn_g2_kernel(Columns c, const G2::A* __restrict__ l2, G2::P* __restrict__ out)
{
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= c.m) return;
  const ZnList<G2L> ls[1] = {g2_job(c, s, l2)};
  if (ls[0].len > c.thr) return;
  store_sum<G2, G2L>(out + s, zn29::zn_walk<G2L, 1>(ls, c.vals, 0, ls[0].len));
}

// Σ over the workgroup's lanes, left in sh[0]
template <class CL>
__device__ __forceinline__ void tree_sum(typename CL::X* sh, const typename CL::X& mine)
{
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int half = ITEM_WG / 2; half; half >>= 1) {
    if ((int)threadIdx.x < half) sh[threadIdx.x] = CL::x_add(sh[threadIdx.x], sh[threadIdx.x + half]);
    __syncthreads();
  }
}

// one workgroup per item: lane t walks the t-th slice of the item's positions
__global__ __launch_bounds__(ITEM_WG) void zn_item_g1_kernel(Columns c, const Item* __restrict__ items, const G1::A* __restrict__ l, const G1::A* __restrict__ al,
                                                              const G1::A* __restrict__ bl, G1L::X* __restrict__ partial)
{
  __shared__ G1L::X sh[ITEM_WG];
  const Item it = items[blockIdx.x];
  const G1Job j = g1_job(c, it.job, l, al, bl);
  const uint32_t per = (it.hi - it.lo + ITEM_WG - 1) / ITEM_WG;
  const uint32_t lo = min(it.hi, it.lo + threadIdx.x * per), hi = min(it.hi, lo + per);
  tree_sum<G1L>(sh, zn29::zn_walk<G1L, 3>(j.ls, c.vals, lo, hi));
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(ITEM_WG) void zn_item_g2_kernel(Columns c, const Item* __restrict__ items, const G2::A* __restrict__ l2, G2L::X* __restrict__ partial)
{
  __shared__ G2L::X sh[ITEM_WG];
  const Item it = items[blockIdx.x];
  const ZnList<G2L> ls[1] = {g2_job(c, it.job, l2)};
  const uint32_t per = (it.hi - it.lo + ITEM_WG - 1) / ITEM_WG;
  const uint32_t lo = min(it.hi, it.lo + threadIdx.x * per), hi = min(it.hi, lo + per);
  tree_sum<G2L>(sh, zn29::zn_walk<G2L, 1>(ls, c.vals, lo, hi));
  if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}
// one workgroup per heavy column: its items' sums, added
template <class C, class CL>
__global__ __launch_bounds__(ITEM_WG) void zn_combine_kernel(const Heavy* __restrict__ heavy, const typename CL::X* __restrict__ partial, typename C::P* __restrict__ out)
{
  __shared__ typename CL::X sh[ITEM_WG];
  const Heavy h = heavy[blockIdx.x];
  typename CL::X acc = CL::x_zero();
  for (uint32_t i = threadIdx.x; i < h.n_items; i += ITEM_WG) acc = CL::x_add(acc, partial[h.first + i]);
  tree_sum<CL>(sh, acc);
  if (threadIdx.x == 0) store_sum<C, CL>(out + h.job, sh[0]);
}

// where the key goes, once its size is known: the caller's buffer, or the mapped temporary of the _file entry
using pv::Sink;

int zkey_new_impl(Groth16R1cs* h, const uint8_t* ptau, size_t ptau_len, int ptau_fd, const Groth16ZkeyNewOptions* opt, Groth16ZkeyNewReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  std::vector<pv::Section> psecs;
  pv::PtauLayout PL;
  if (int rc = pv::ptau_layout(ptau, ptau_len, psecs, &PL)) return rc;
  const pv::R1csShape shape = pv::r1cs_shape(h);
  const uint32_t m = shape.n_wires, npub = shape.n_public, nc = shape.m;
  if ((uint64_t)m < (uint64_t)npub + 1) return pv::fail(pv::ERR_FORMAT, "r1cs: %u wires cannot hold the constant and %u public signals", m, npub);
  uint32_t k;
  const uint64_t domain = pv::circuit_domain(nc, npub, &k);
  if (k > 28) return pv::fail(pv::ERR_ARG, "the circuit's domain 2^%u is above the field's two-adicity", k);
  if (int rc = pv::ptau_blocks_for_domain(PL, k)) return rc;
  const uint32_t n = (uint32_t)domain;
  rep->n_vars = m, rep->n_public = npub, rep->domain = n;
  const pv::R1csDeviceRows rows = pv::r1cs_device_rows(h);
  const uint64_t n_entries = rows.n_terms + npub + 1;
  if (3 * (uint64_t)m + 1 > 0xffffffffull || n_entries > 0xffffffffull) return pv::fail(pv::ERR_ARG, "the circuit's columns do not fit 32-bit offsets");
  // the header's α₁, β₁, β₂ are copied words: the lane tests on the host first, as the key check runs them on a header
  {
    fe p1[2];
    fe2 p2[2];
    const int hdr_sec[2] = {4, 5};
    for (int sid : hdr_sec) {
      memcpy(p1, PL.sec[sid]->p, 64);
      if (const int kind = p29::classify_g1(p1)) return pv::ptau_point_fail(sid, 0, kind);
    }
    memcpy(p2, PL.sec[6]->p, 128);
    if (const int kind = p29::classify_g2(p2)) return pv::ptau_point_fail(6, 0, kind);
  }

  pv::StageTrace trace("zkey-new", "ICICLE_SNARK_TRACE_ZKEY_NEW");

  const uint32_t thr = heavy_threshold(opt ? opt->heavy_column_terms : 0);

  std::lock_guard<std::mutex> lk(pv::r1cs_mutex(h));
  const auto t_dev = std::chrono::steady_clock::now();
  isnark::vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, shape.dev, 2)) return rc;
  const hipStream_t st = ds.stream(0), st2 = ds.stream(1);
  pv::Event ev_cols, ev_g2;
  if (int rc = ev_cols.create()) return rc;
  if (int rc = ev_g2.create()) return rc;
  bool oom = false;
  auto alloc = [&](auto** p, size_t count) {
    typedef typename std::remove_pointer<typename std::remove_pointer<decltype(p)>::type>::type T;
    *p = ds.buf.alloc<T>(std::max<size_t>(count, 1));
    if (!*p) oom = true;
  };

  // ---- transpose: column lists, and section 4's records
  // a heavy job has more than thr terms and the jobs of a group share at most 2·n_entries (G1) / n_entries (G2) of them
  const uint64_t cap_heavy[2] = {2 * n_entries / thr + 1, n_entries / thr + 1};
  const uint64_t cap_items[2] = {2 * cap_heavy[0] + 1, 2 * cap_heavy[1] + 1};
  Transposed T;
  Counters* d_cnt;
  PtauRanges ranges;
  Heavy* d_heavy[2];
  Item* d_items[2];
  alloc(&d_cnt, 1);
  for (int g = 0; g < 2; g++) {
    alloc(&d_heavy[g], (size_t)cap_heavy[g]);
    alloc(&d_items[g], (size_t)cap_items[g]);
  }
  if (oom) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  DEV_TRY("hipMemset", hipMemsetAsync(d_cnt, 0, sizeof(Counters), st));
  if (int rc = ranges.reset(ds, st)) return rc;
  if (int rc = transpose_rows(ds, st, rows, nc, m, npub, &T)) return rc;
  uint32_t* const d_recoff = T.d_recoff;
  uint32_t* const d_rec = T.d_rec;
  const Columns cols = T.columns(rows.d_vals, m, thr);
  DEV_LAUNCH("plan kernel launch", zn_plan_kernel<false>, dim3((uint32_t)((3 * (uint64_t)m + 255) / 256)), dim3(256), st, cols, d_cnt, d_heavy[0], d_items[0]);
  DEV_LAUNCH("plan kernel launch", zn_plan_kernel<true>, dim3((m + 255) / 256), dim3(256), st, cols, d_cnt, d_heavy[1], d_items[1]);
  // (the second stream's first kernel writes the ranges' d_first: behind the memsets)
  DEV_TRY("hipEventRecord", hipEventRecord(ev_cols.e, st));
  DEV_TRY("hipStreamWaitEvent", hipStreamWaitEvent(st2, ev_cols.e, 0));
  trace.lap("session, transpose enqueued");

  // ---- the ptau's ranges, each tested where it lands.  (The G2 block's test on the second stream: it is the long one, and the
  // uploads behind it do not wait for it.)
  {
    const pv::FileHint hint(ptau, ptau_len, ptau_fd);
    if (int rc = ranges.stage(PL, k, ds, shape.dev, st, st2, &rep->upload_ms)) return rc;
  }
  trace.lap("ptau ranges uploaded");

  // ---- what the host has to know before the columns run: the lane tests' verdicts, the record count, the heavy columns
  DEV_TRY("hipEventRecord", hipEventRecord(ev_g2.e, st2));
  DEV_TRY("hipStreamWaitEvent", hipStreamWaitEvent(st, ev_g2.e, 0));
  unsigned long long first[PtauRanges::N];
  Counters cnt;
  uint32_t n_ab = 0;
  DEV_TRY("download", hipMemcpyAsync(first, ranges.d_first, sizeof first, hipMemcpyDeviceToHost, st));
  DEV_TRY("download", hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
  DEV_TRY("download", hipMemcpyAsync(&n_ab, d_recoff + nc, 4, hipMemcpyDeviceToHost, st));
  DEV_TRY("transpose and ptau kernels", hipStreamSynchronize(st));
  if (int rc = ranges.verdict(first)) return rc;
  trace.lap("lane tests, plan");
  const uint64_t n_coeffs = (uint64_t)n_ab + npub + 1;
  const FileLayout F(m, npub, n, n_coeffs);
  rep->n_coeffs = n_coeffs;
  rep->zkey_bytes = F.total;
  rep->longest_column = cnt.longest;
  rep->heavy_columns = cnt.heavy[0] + cnt.heavy[1];
  rep->heavy_items = cnt.items[0] + cnt.items[1];
  if (cnt.heavy[0] > cap_heavy[0] || cnt.heavy[1] > cap_heavy[1] || cnt.items[0] > cap_items[0] || cnt.items[1] > cap_items[1])
    return pv::fail(pv::ERR_DEVICE, "device: the heavy-column plan overran its bounds"); // (cannot happen: the bounds are sums of terms)
  uint8_t* out = nullptr;
  if (int rc = sink(F.total, &out)) return rc;

  // ---- columns
  G1::P* d_p1;
  G2::P* d_p2;
  G1::A* d_a1;
  G2::A* d_a2;
  fe* d_s1;
  fe2* d_s2;
  uint8_t* d_odd;
  G1L::X* d_part1;
  G2L::X* d_part2;
  alloc(&d_p1, (size_t)G1_OUTPUTS * m);
  alloc(&d_p2, (size_t)m);
  alloc(&d_a1, (size_t)G1_OUTPUTS * m);
  alloc(&d_a2, (size_t)m);
  alloc(&d_s1, (size_t)G1_OUTPUTS * m);
  alloc(&d_s2, (size_t)m);
  alloc(&d_odd, (size_t)n * 64);
  alloc(&d_part1, (size_t)cnt.items[0]);
  alloc(&d_part2, (size_t)cnt.items[1]);
  if (oom) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  const G1::A *l1 = (const G1::A*)ranges.l1(), *al = (const G1::A*)ranges.alpha_l1(), *bl = (const G1::A*)ranges.beta_l1();
  const G2::A* l2 = (const G2::A*)ranges.l2();
  // G2 on the second stream, beside the G1 kernels
  DEV_LAUNCH("G2 column kernel launch", zn_g2_kernel, dim3((m + 63) / 64), dim3(64), st2, cols, l2, d_p2);
  if (cnt.heavy[1]) {
    DEV_LAUNCH("G2 item kernel launch", zn_item_g2_kernel, dim3(cnt.items[1]), dim3(ITEM_WG), st2, cols, d_items[1], l2, d_part2);
    DEV_LAUNCH("G2 combine kernel launch", (zn_combine_kernel<G2, G2L>), dim3(cnt.heavy[1]), dim3(ITEM_WG), st2, d_heavy[1], d_part2, d_p2);
  }
  if (int rc = pv::to_file_form<G2>(st2, d_p2, m, d_a2, d_s2)) return rc;
  DEV_LAUNCH("G1 column kernel launch", zn_g1_kernel, dim3((uint32_t)((G1_OUTPUTS * (uint64_t)m + 63) / 64)), dim3(64), st, cols, l1, al, bl, d_p1);
  if (cnt.heavy[0]) {
    DEV_LAUNCH("G1 item kernel launch", zn_item_g1_kernel, dim3(cnt.items[0]), dim3(ITEM_WG), st, cols, d_items[0], l1, al, bl, d_part1);
    DEV_LAUNCH("G1 combine kernel launch", (zn_combine_kernel<G1, G1L>), dim3(cnt.heavy[0]), dim3(ITEM_WG), st, d_heavy[0], d_part1, d_p1);
  }
  if (int rc = pv::to_file_form<G1>(st, d_p1, G1_OUTPUTS * (uint64_t)m, d_a1, d_s1)) return rc;
  if (int rc = ranges.gather_odd(st, n, d_odd)) return rc;
  DEV_TRY("G1 column kernels", hipStreamSynchronize(st));
  trace.lap("G1 kernels done");
  DEV_TRY("G2 column kernels", hipStreamSynchronize(st2));
  trace.lap("G2 kernels done");
  rep->device_ms = pv::ms_since(t_dev);

  // ---- the file
  const auto t_down = std::chrono::steady_clock::now();
  const uint8_t *a1 = (const uint8_t*)d_a1, *a2 = (const uint8_t*)d_a2;
  const size_t per = (size_t)m * 64;
  const isnark::CopyJob jobs[7] = {
    {out + F.off[3], a1 + OUT_COMB * per, (size_t)F.len[3]},                   // comb_s, s <= npub
    {out + F.off[4] + 4, d_rec, (size_t)(n_coeffs * pv::COEF_RECORD_BYTES)},
    {out + F.off[5], a1 + OUT_A * per, per},
    {out + F.off[6], a1 + OUT_B1 * per, per},
    {out + F.off[7], a2, (size_t)m * 128},
    {out + F.off[8], a1 + OUT_COMB * per + F.len[3], (size_t)F.len[8]},        // comb_s, s > npub
    {out + F.off[9], d_odd, (size_t)n * 64},
  };
  DEV_TRY("device to host download", isnark::staged_copy(shape.dev, jobs, 7, false));
  rep->download_ms = pv::ms_since(t_down);
  // α₁ β₁ β₂ the ptau's stored words; γ₂ = G₂, δ₁ = G₁, δ₂ = G₂ in Montgomery form
  const G1::A g1 = isnark::vb::g1_generator_mont();
  const G2::A g2 = isnark::vb::g2_generator_mont();
  write_key_frame(out, F, m, npub, n, n_coeffs, {PL.sec[4]->p, PL.sec[5]->p, PL.sec[6]->p, &g2, &g1, &g2});
  trace.lap("download, header");
  return 0;
}

} // namespace

ISNARK_API int groth16_zkey_new(Groth16R1cs* h, const void* ptau, size_t ptau_len, void* zkey_out, size_t cap, const Groth16ZkeyNewOptions* opt, Groth16ZkeyNewReport* report)
{
  return zkey_new_impl(h, (const uint8_t*)ptau, ptau_len, -1, opt, report, pv::buffer_sink("key", zkey_out, cap));
}

ISNARK_API int groth16_zkey_new_file(Groth16R1cs* h, const char* ptau_path, const char* zkey_path, const Groth16ZkeyNewOptions* opt, Groth16ZkeyNewReport* report)
{
  if (!ptau_path || !zkey_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile pf;
  if (int rc = pf.open_ro(ptau_path, /*read_ahead=*/false)) return rc; // only the ranges that are read are touched
  pv::TempOutput to(zkey_path); // a failed call leaves nothing there
  int rc = zkey_new_impl(h, pf.data, pf.len, pf.fd, opt, report, [&](uint64_t bytes, uint8_t** out) { return to.open(bytes, out); });
  const auto t_write = std::chrono::steady_clock::now();
  rc = to.finish(rc);
  if (rc == 0 && report) report->write_ms = pv::ms_since(t_write);
  return rc;
}
