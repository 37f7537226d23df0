// zkey_check.hip — groth16_zkey_check: is a proving key sound?  (include/groth16_prover.h has the contract)
//
//   membership   every point of sections 3 (IC), 5 (A), 6 (B1), 8 (C), 9 (H) through zkey_g1_kernel and of section 7 (B2) through
//                zkey_g2_kernel, one lane per point, in the file's Montgomery-256 form (zkey_check29.h: classify_g1 / classify_g2 —
//                canonical, on the curve / the twist, G2: in the order-r subgroup); the six header points through the same two
//                functions on the host; the records of section 4 through zkey_coef_kernel (qap.h's range rule, value < r).
//                A fault is the rare branch: the faulting lane alone adds 1 to its section's count and takes the minimum of
//                (index, kind) — nothing per element comes back from the device.
//   pairs        e(β₁, G₂) = e(G₁, β₂) and e(δ₁, G₂) = e(G₁, δ₂) by the host pairing; sections 6 against 7 by ONE such equation on
//                S₁ = Σ zᵢ·B1ᵢ, S₂ = Σ zᵢ·B2ᵢ — the library's MSMs with bitsize = 128 over the bases the membership stage left on
//                the device, zᵢ the combined verifier's coefficients of a secret seed, made on the worker pool while this thread
//                walks the sections.
// The sections are walked in slices of slice_points: a slice goes up through the library's pinned staging (staged_copy, which
// returns when it has landed) and its kernel runs behind it while the next slice is on its way — the G2 kernel on stream 0, the
// others on stream 1.  Sections 6 and 7 stay on the device for the MSMs (stream 1); every other slice goes through a ring of two
// buffers.  The header's two pair checks run on a pooled worker beside all that.
#include <algorithm>
#include <chrono>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "sha256.h"
#include "verify_batch.h"
#include "zkey_check29.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;

constexpr int G1_WG = 256;                      // points per block of zkey_g1_kernel (its LDS tile: 256 rows of 64 + 16 B)
constexpr int G2_WG = 64;
constexpr uint32_t DEFAULT_SLICE = 1u << 20;    // points per upload slice: 64 MB of G1 rows, 128 MB of G2 rows
using pv::NO_FAULT;

// per zkey section id: how many elements are at fault, and min over them of (index << 3 | kind)
struct Tally {
  unsigned long long count[10];
  unsigned long long first[10];
};
__device__ inline void tally_fault(Tally* t, int sec, unsigned long long index, int kind)
{
  atomicAdd(&t->count[sec], 1ull);
  atomicMin(&t->first[sec], index << 3 | (unsigned long long)kind);
}

// G1 points rows[4·i … 4·i + 3] (64-byte rows: x, y), i < m; point i has index base + i in section `sec`.  The block reads its
// 16 KB of rows with four fully coalesced 16-byte loads per lane and hands each lane its own row through LDS (rows padded to
// 80 bytes: consecutive lanes start on different bank groups).
__global__ __launch_bounds__(G1_WG) void zkey_g1_kernel(const uint4* __restrict__ rows, uint32_t m, unsigned long long base, int sec, Tally* __restrict__ t)
{
  __shared__ uint4 tile[G1_WG * 5];
  const uint32_t b0 = blockIdx.x * G1_WG; // < m: the grid has ⌈m / G1_WG⌉ blocks
  const uint32_t cnt = m - b0 < (uint32_t)G1_WG ? m - b0 : (uint32_t)G1_WG;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t q = k * G1_WG + threadIdx.x;
    if (q < 4 * cnt) tile[(q >> 2) * 5 + (q & 3)] = rows[(size_t)b0 * 4 + q];
  }
  __syncthreads();
  if (threadIdx.x >= cnt) return;
  fe p[2];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint4 v = tile[threadIdx.x * 5 + j];
    uint32_t* w = p[j >> 1].l + 4 * (j & 1);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
  const int kind = p29::classify_g1(p);
  if (kind) tally_fault(t, sec, base + b0 + threadIdx.x, kind);
}

// G2 points pts[2·i], pts[2·i + 1] (x, y), i < m.  A kernel of its own: the 63-bit multiplication of the subgroup test sets its
// register demand, which must not set the G1 kernel's occupancy.
__global__ __launch_bounds__(G2_WG) void zkey_g2_kernel(const fe2* __restrict__ pts, uint32_t m, unsigned long long base, int sec, Tally* __restrict__ t)
{
  const uint32_t i = blockIdx.x * G2_WG + threadIdx.x;
  if (i >= m) return;
  const fe2 p[2] = {pts[2 * (size_t)i], pts[2 * (size_t)i + 1]};
  const int kind = p29::classify_g2(p);
  if (kind) tally_fault(t, sec, base + i, kind);
}

// section-4 records {m:u32 c:u32 s:u32 value[8×u32]}, i < m: the loader's range rule, and the stored residue below r
__global__ __launch_bounds__(256) void zkey_coef_kernel(const uint32_t* __restrict__ rec, uint32_t m, unsigned long long base, uint32_t n, uint32_t n_vars, Tally* __restrict__ t)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint32_t* e = rec + (size_t)i * 11;
  fe v;
#pragma unroll
  for (int k = 0; k < 8; k++) v.l[k] = e[3 + k];
  if (!isnark::qap_record_in_range(e[0], e[1], e[2], n, n_vars) || !Fr::is_canonical(v)) tally_fault(t, 4, base + i, GROTH16_ZKEY_COEFFICIENT);
}

using pv::ZkeyLayout;

// the device side of one call
struct Check {
  const ZkeyLayout& L;
  const int dev;
  const uint32_t slice;
  isnark::vb::DeviceSession ds;
  Tally* d_tally = nullptr;
  uint8_t* ring[2] = {nullptr, nullptr};
  pv::Event ring_ev[2]; // (destroyed before the session, whose destructor drains the streams before it frees the buffers)
  bool ring_used[2] = {false, false};
  int ring_k = 0;
  uint8_t *d_b1 = nullptr, *d_b2 = nullptr;
  double upload_ms = 0;
  Tally tally;

  Check(const ZkeyLayout& layout, int device, uint32_t slice_points) : L(layout), dev(device), slice(slice_points) {}

  int open()
  {
    if (int rc = pv::open_session(ds, dev, 2)) return rc;
    const uint64_t longest = std::max<uint64_t>(std::max<uint64_t>(L.n_vars, L.domain), L.n_coef);
    const size_t ring_bytes = (size_t)std::min<uint64_t>(slice, longest) * 64;
    d_tally = ds.buf.alloc<Tally>(1);
    ring[0] = ds.buf.alloc<uint8_t>(ring_bytes);
    ring[1] = ds.buf.alloc<uint8_t>(ring_bytes);
    d_b1 = ds.buf.alloc<uint8_t>((size_t)L.n_vars * 64);
    d_b2 = ds.buf.alloc<uint8_t>((size_t)L.n_vars * 128);
    if (!d_tally || !ring[0] || !ring[1] || !d_b1 || !d_b2) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
    for (pv::Event& e : ring_ev)
      if (int rc = e.create()) return rc;
    for (int s = 0; s < 10; s++) {
      tally.count[s] = 0;
      tally.first[s] = NO_FAULT;
    }
    DEV_TRY("upload", hipMemcpyAsync(d_tally, &tally, sizeof tally, hipMemcpyHostToDevice, ds.stream(0)));
    DEV_TRY("upload", hipStreamSynchronize(ds.stream(0))); // (`tally` is pageable: the copy has read it)
    return 0;
  }

  // one section (`kind` 1: G1 rows, 2: G2 rows, 4: coefficient records) in slices; keep: where the whole section stays, or nullptr
  int walk(int sec, int kind, const uint8_t* src, uint64_t count, uint8_t* keep)
  {
    const size_t elem = kind == 1 ? 64 : kind == 2 ? 128 : 44;
    // the G2 kernel on a stream of its own: behind it on one stream the G1 kernels — and with them the ring's buffers — would wait
    // for it (measured: 103 instead of 72–82 ms for the 1.6 M-wire key).  Which of the two streams it takes made no difference.
    const hipStream_t st = ds.stream(kind == 2 ? 0 : 1);
    for (uint64_t off = 0; off < count; off += slice) {
      const uint32_t m = (uint32_t)std::min<uint64_t>(slice, count - off);
      uint8_t* dst = keep ? keep + off * elem : ring[ring_k];
      if (!keep && ring_used[ring_k]) DEV_TRY("membership kernel", hipEventSynchronize(ring_ev[ring_k].e)); // the kernel that last read this buffer
      if (int rc = pv::timed_upload(dev, dst, src + off * elem, (size_t)m * elem, &upload_ms)) return rc;
      const char* const what = "membership kernel launch";
      if (kind == 1) DEV_LAUNCH(what, zkey_g1_kernel, dim3((m + G1_WG - 1) / G1_WG), dim3(G1_WG), st, (const uint4*)dst, m, (unsigned long long)off, sec, d_tally);
      else if (kind == 2) DEV_LAUNCH(what, zkey_g2_kernel, dim3((m + G2_WG - 1) / G2_WG), dim3(G2_WG), st, (const fe2*)dst, m, (unsigned long long)off, sec, d_tally);
      else DEV_LAUNCH(what, zkey_coef_kernel, dim3((m + 255) / 256), dim3(256), st, (const uint32_t*)dst, m, (unsigned long long)off, L.domain, L.n_vars, d_tally);
      if (!keep) {
        DEV_TRY("hipEventRecord", hipEventRecord(ring_ev[ring_k].e, st));
        ring_used[ring_k] = true;
        ring_k ^= 1;
      }
    }
    return 0;
  }

  // B2 first: its kernel is the long one, and every later upload runs beside it
  int membership(pv::StageTrace& trace)
  {
    const uint64_t nv = L.n_vars;
    if (int rc = walk(7, 2, L.sec[7]->p, nv, d_b2)) return rc;
    if (int rc = walk(6, 1, L.sec[6]->p, nv, d_b1)) return rc;
    if (int rc = walk(3, 1, L.sec[3]->p, (uint64_t)L.n_public + 1, nullptr)) return rc;
    if (int rc = walk(4, 4, L.sec[4]->p + 4, L.n_coef, nullptr)) return rc;
    if (int rc = walk(5, 1, L.sec[5]->p, nv, nullptr)) return rc;
    if (int rc = walk(8, 1, L.sec[8]->p, nv - L.n_public - 1, nullptr)) return rc;
    if (int rc = walk(9, 1, L.sec[9]->p, L.domain, nullptr)) return rc;
    trace.lap("sections uploaded");
    DEV_TRY("membership kernels", hipStreamSynchronize(ds.stream(1)));
    trace.lap("G1 kernels done");
    DEV_TRY("download", hipMemcpyAsync(&tally, d_tally, sizeof tally, hipMemcpyDeviceToHost, ds.stream(0)));
    DEV_TRY("membership kernels", hipStreamSynchronize(ds.stream(0)));
    trace.lap("membership kernels done");
    return 0;
  }

  // S₁ = Σ zᵢ·B1ᵢ, S₂ = Σ zᵢ·B2ᵢ over the bases the walk left on the device (Montgomery form; an identity base adds nothing)
  int sums(const std::vector<bn254_scalar_t>& z, bn254_projective_t* s1, bn254_g2_projective_t* s2)
  {
    // the coefficients go up once and serve both MSMs
    bn254_scalar_t* d_z = ds.buf.alloc<bn254_scalar_t>(z.size());
    if (!d_z) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
    const isnark::CopyJob job = {d_z, z.data(), z.size() * sizeof z[0]};
    DEV_TRY("host to device upload", isnark::staged_copy(dev, &job, 1, true));
    const MSMConfig mc = pv::device_msm_config(ds.streams[1], 128);
    if (int rc = pv::sliced_msm(mc, d_z, d_b1, L.n_vars, s1)) return rc;
    return pv::sliced_msm(mc, d_z, d_b2, L.n_vars, s2);
  }
};

using isnark::vb::words_zero;

// e(P₁, G₂) = e(G₁, P₂) for standard-form affine points, (0, 0) = the identity, by the host pairing
bool pair_holds(const bn254_affine_t& p1, const bn254_g2_affine_t& p2)
{
  return isnark::vb::pairing_eq(p1, isnark::vb::g2_generator_affine(), isnark::vb::g1_generator_affine(), p2);
}

struct First { // the first fault so far, in the header's order of reporting
  int32_t kind = 0, section = 0;
  uint64_t index = 0;
  void offer(int32_t k, int32_t s, uint64_t i)
  {
    if (kind && (section < s || (section == s && index <= i))) return;
    kind = k, section = s, index = i;
  }
};

int zkey_check_impl(const uint8_t* data, size_t len, const char* device, const Groth16ZkeyCheckOptions* opt, Groth16ZkeyReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  ZkeyLayout L;
  if (int rc = pv::zkey_layout(data, len, secs, &L)) return rc;
  uint8_t seed[32];
  if (int rc = pv::seed_or_random(opt ? opt->seed32 : nullptr, seed)) return rc;

  // the header's six points, in file order, on the host: kinds 1 2 3 by the kernels' functions, then 4
  First first;
  const bool slot_g2[6] = {false, false, true, true, false, true};
  const size_t slot_off[6] = {0, 64, 128, 256, 384, 448};
  for (int k = 0; k < 6; k++) {
    int kind;
    bool zero;
    if (slot_g2[k]) {
      fe2 p[2];
      memcpy(p, L.header_points + slot_off[k], 128);
      kind = p29::classify_g2(p);
      zero = words_zero(p, 128);
    } else {
      fe p[2];
      memcpy(p, L.header_points + slot_off[k], 64);
      kind = p29::classify_g1(p);
      zero = words_zero(p, 64);
    }
    if (!kind && zero) kind = GROTH16_ZKEY_IDENTITY;
    if (kind) {
      rep->faults[2]++;
      first.offer(kind, 2, (uint64_t)k);
    }
  }

  // the device part; the coefficients of the 6/7 check are made on the pool meanwhile
  const auto t_dev = std::chrono::steady_clock::now();
  pv::StageTrace trace("zkey-check", "ICICLE_SNARK_TRACE_ZKEY_CHECK");
  Check c(L, dev, opt && opt->slice_points ? opt->slice_points : DEFAULT_SLICE);
  std::vector<bn254_scalar_t> z(L.n_vars);
  memset(z.data(), 0, z.size() * sizeof z[0]);
  // (every range on the pool, none kept for this thread as run_ranges — and with it device_call.h's fill_coefficients — would: this
  //  thread's part is the walk, and a range behind it would run after the device has finished)
  const int tasks = isnark::ranges_of(L.n_vars, 4096);
  std::vector<isnark::HostTask> ht(tasks);
  for (int t = 0; t < tasks; t++) {
    const size_t lo = (size_t)L.n_vars * t / tasks, hi = (size_t)L.n_vars * (t + 1) / tasks;
    ht[t].fn = [&z, &seed, lo, hi] {
      for (size_t i = lo; i < hi; i++) isnark::combined_coefficient(seed, (uint64_t)i, (uint8_t*)&z[i]);
    };
    isnark::WorkerPool::get().run_or_inline(&ht[t]);
  }
  // β₁ / β₂ and δ₁ / δ₂ on a pooled worker meanwhile: four host pairings
  const int header_g1_slot[2] = {1, 4}, header_g2_slot[2] = {2, 5};
  const bool header_pairs = rep->faults[2] == 0;
  bool header_pair_ok[2] = {true, true};
  double header_pair_ms = 0;
  isnark::HostTask header_task;
  header_task.fn = [&] {
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < 2; k++) {
      G1::A a;
      G2::A b;
      memcpy(&a, L.header_points + slot_off[header_g1_slot[k]], 64);
      memcpy(&b, L.header_points + slot_off[header_g2_slot[k]], 128);
      const G1::A as = {Fq::from_mont(a.x), Fq::from_mont(a.y)};
      const G2::A bs = {Fq2Ops::from_mont(b.x), Fq2Ops::from_mont(b.y)};
      bn254_affine_t p1;
      bn254_g2_affine_t p2;
      memcpy(&p1, &as, sizeof p1);
      memcpy(&p2, &bs, sizeof p2);
      header_pair_ok[k] = pair_holds(p1, p2);
    }
    header_pair_ms = pv::ms_since(t0);
  };
  if (header_pairs) isnark::WorkerPool::get().run_or_inline(&header_task);
  int rc = c.open();
  trace.lap("session, buffers");
  if (!rc) rc = c.membership(trace);
  for (int t = 0; t < tasks; t++)
    if (ht[t].queued) isnark::WorkerPool::wait(&ht[t]);
  if (header_task.queued) isnark::WorkerPool::wait(&header_task);
  trace.lap("pool joined");
  if (rc) return rc;
  for (int s = 3; s < 10; s++) {
    rep->faults[s] = c.tally.count[s];
    if (c.tally.first[s] != NO_FAULT) first.offer((int32_t)(c.tally.first[s] & 7), s, c.tally.first[s] >> 3);
  }
  bn254_projective_t s1;
  bn254_g2_projective_t s2;
  const bool pair67 = rep->faults[6] == 0 && rep->faults[7] == 0;
  if (pair67)
    if (int rc2 = c.sums(z, &s1, &s2)) return rc2;
  trace.lap("sums");
  rep->upload_ms = c.upload_ms;
  rep->device_ms = pv::ms_since(t_dev);

  // pair checks, each only over sections without a membership fault (the header's ran on the pool)
  const auto t_pair = std::chrono::steady_clock::now();
  for (int k = 0; k < 2; k++)
    if (header_pairs && !header_pair_ok[k]) {
      rep->faults[2]++;
      first.offer(GROTH16_ZKEY_PAIR_MISMATCH, 2, (uint64_t)header_g1_slot[k]);
    }
  if (pair67 && !pair_holds(isnark::vb::affine_or_zero(s1), isnark::vb::affine_or_zero(s2))) {
    rep->faults[6]++;
    first.offer(GROTH16_ZKEY_PAIR_MISMATCH, 6, UINT64_MAX);
  }
  rep->pairing_ms = pv::ms_since(t_pair) + header_pair_ms;
  trace.lap("pair checks");
  rep->kind = first.kind;
  rep->section = first.section;
  rep->index = first.index;
  return first.kind ? 0 : 1;
}

} // namespace

ISNARK_API int groth16_zkey_check(const void* zkey, size_t len, const char* device, const Groth16ZkeyCheckOptions* opt, Groth16ZkeyReport* report)
{
  return zkey_check_impl((const uint8_t*)zkey, len, device, opt, report);
}

ISNARK_API int groth16_zkey_check_file(const char* zkey_path, const char* device, const Groth16ZkeyCheckOptions* opt, Groth16ZkeyReport* report)
{
  if (!zkey_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile mf;
  if (int rc = mf.open_ro(zkey_path)) return rc;
  // (the staging workers pread() the file instead of copying out of the mapping)
  const pv::FileHint hint(mf.data, mf.len, mf.fd);
  return zkey_check_impl(mf.data, mf.len, device, opt, report);
}
