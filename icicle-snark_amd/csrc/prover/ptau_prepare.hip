// ptau_prepare.hip — groth16_ptau_prepare: sections 12 … 15 of a powers-of-tau file from its sections 2 … 5, what `snarkjs powersoftau
// prepare phase2` makes.  include/groth16_prover.h has the contract and the definition of the output; DESIGN.md §7g.
//
// Block p of a section is the inverse NTT of size 2^p of the first 2^p points of its source, over curve points:
//   out_j = (1/2^p)·Σ_i ω_p^(−ij)·S_i.
//   host    the container (ptau_unprepared_layout), the output's size against the room, section 6 through the lane test; the table
//           tw[i] = ω^(−i), i < 2^power, of the root of order 2^(power+1) — every twiddle of every level of every block is one of them.
//   device  section by section (2 → 12, 3 → 13, 4 → 14, 5 → 15): the source goes up and through the lane tests (ptau_ranges.h's
//           kernels; section 3 with the subgroup test) before any arithmetic sees it.  Then decimation in time with affine points
//           between the levels, in two passes: the blocks below the top one side by side (a level of all of them is ONE launch — a
//           level is a full-width scalar multiplication long whatever the block's size, so a launch per block and level would cost
//           Σ p of them), then the top block alone:
//             pp_load_kernel   lane per element: (1/2^p)·S[bitrev_p(i)], zc_scale with the digits of 2^(−p) from a table of 29 — one
//                              scalar per block, the same words in every lane of a wave inside a block.  An index past the source's
//                              end is the identity: the zero-extended vector of section 12's block power + 1.
//             pp_level_kernel  level s, a lane per butterfly of every block p > s: a[i0], a[i0 + 2^s] with the twiddle ω_(s+1)^(−j) =
//                              tw[j·2^(power−s)], a scalar per lane (ptau_prepare29.h: pp_twiddled, pp_side).  Level 0 multiplies nothing.
//           each followed by point_form.h's to_file_form: the block is in the file's form after every level, the identity all
//           zero.  The finished blocks go down into the output at element 2^p − 1 of their section.
//   Resident: one source section, the top block's working buffers (affine, projective, the inversion's scratch) and the twiddles.
#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "point_form.h"
#include "prover_internal.h"
#include "ptau_prepare29.h"
#include "ptau_ranges.h"
#include "verify_batch.h"
#include "zkey_check29.h"

using namespace bn254;
using bn254::zc29::ZcDigits;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;
using pv::Group;

constexpr int PP_WG = 64;

// Blocks p_lo … p_hi of a section side by side in the working buffers, as they lie in the section: block p begins at element
// 2^p − 2^p_lo of the buffers (2^p − 1 of the section), so the blocks 0 … p − 1 together are one element shorter than block p alone.
// lane e' < count = 2^(p_hi+1) − 2^p_lo: element i of block p, out[e'] = 2^(−p)·src[bitrev_p(i)], the identity for an index that is not
// below `avail` — Montgomery projective, the identity (0, 1, 0).  inv[p]: the digits of 2^(−p), read by the walk a word per 32 steps
// with the loop counter as the index — the same words in every lane of a wave whose lanes share a block.
template <class C>
__global__ __launch_bounds__(PP_WG) void pp_load_kernel(const typename C::A* __restrict__ src, uint64_t avail, uint32_t p_lo, uint64_t count, const ZcDigits* __restrict__ inv,
                                                        typename C::P* __restrict__ out)
{
  typedef CurveL<typename Group<C>::F> CL;
  const uint64_t e = (uint64_t)blockIdx.x * PP_WG + threadIdx.x;
  if (e >= count) return;
  const uint64_t e1 = e + ((uint64_t)1 << p_lo); // the section's element index + 1: in [2^p, 2^(p+1))
  const uint32_t p = 63 - __clzll((long long)e1);
  const uint64_t i = e1 - ((uint64_t)1 << p), r = p ? __brevll(i) >> (64 - p) : 0;
  typename C::P res = C::p_zero();
  if (r < avail) {
    const typename C::A a = src[r];
    if (!C::aff_is_zero(a)) res = C::x_to_projective(CL::x_store(zc29::zc_scale<CL>(a, inv[p])));
  }
  out[e] = res;
}

// level s of every block p_lo … p_hi that has one (p > s): lane g < count = 2^p_hi − first, first = 2^(max(p_lo, s + 1) − 1).  g + first
// lies in [2^(p−1), 2^p) for butterfly t = g + first − 2^(p−1) of block p, which takes a[i0] and a[i1 = i0 + 2^s], i0 = (block p's
// begin) + (t >> s)·2^(s+1) + j, j = t mod 2^s, and writes a[i0] + w·a[i1] and a[i0] − w·a[i1] to out[i0] and out[i1]; w = tw[j << tw_shift]
// whatever the block.  FIRST: level 0, w = 1.
template <class C, bool FIRST>
__global__ __launch_bounds__(PP_WG) void pp_level_kernel(const typename C::A* __restrict__ a, uint64_t first, uint64_t count, uint32_t s, uint32_t p_lo, const fe* __restrict__ tw,
                                                         uint32_t tw_shift, typename C::P* __restrict__ out)
{
  typedef typename Group<C>::F F;
  typedef CurveL<F> CL;
  const uint64_t g = (uint64_t)blockIdx.x * PP_WG + threadIdx.x;
  if (g >= count) return;
  const uint64_t g1 = g + first;
  const uint32_t p = 64 - __clzll((long long)g1);
  const uint64_t t = g1 - ((uint64_t)1 << (p - 1)), begin = ((uint64_t)1 << p) - ((uint64_t)1 << p_lo);
  const uint64_t j = t & (((uint64_t)1 << s) - 1), i0 = begin + ((t >> s) << (s + 1)) + j, i1 = i0 + ((uint64_t)1 << s);
  const typename C::A pt = a[i0], q = a[i1];
  typename CL::X tq; // T = w·Q
  if (FIRST) {
    tq = pp29::pp_twiddled<F>(q, nullptr);
  } else {
    const ZcDigits d = zc29::zc_recode(ld(tw + (j << tw_shift)));
    tq = pp29::pp_twiddled<F>(q, &d);
  }
  // P + T to i0, then P − T to i1: one after the other, so that one x_madd's registers are live and not two
#pragma unroll 1
  for (int side = 0; side < 2; side++) out[side ? i1 : i0] = C::x_to_projective(CL::x_store(pp29::pp_side<F>(tq, pt, side != 0)));
}

// ---- scalars on the host
// tw[i] = w^(−i), i < count, standard form; w the root of order 2·count (count = 1: the table is {1})
int twiddle_table(uint32_t power, std::vector<fe>& tw)
{
  const size_t count = (size_t)1 << power;
  fe w;
  if (int rc = pv::root_of_unity(power + 1, &w)) return rc;
  const fe winv = Fr::inv(Fr::to_mont(w));
  tw.resize(count);
  isnark::run_ranges(count, 1 << 14, [&](int, size_t lo, size_t hi) {
    fe x = pc29::pc_pow(winv, lo);
    for (size_t i = lo; i < hi; i++) {
      tw[i] = Fr::from_mont(x);
      x = Fr::mul(x, winv);
    }
  });
  return 0;
}
fe inverse_of_two_to(uint32_t p)
{
  fe two = Fr::zero();
  two.l[0] = 2;
  return Fr::from_mont(Fr::inv(pc29::pc_pow(Fr::to_mont(two), p)));
}

struct Buffers {
  uint8_t *src = nullptr, *aff = nullptr, *proj = nullptr, *scratch = nullptr;
  fe* tw = nullptr;
  ZcDigits* inv = nullptr; // [p]: the digits of 2^(−p), p ≤ 28
  unsigned long long* first = nullptr;
};
constexpr uint32_t INV_COUNT = 29;

// blocks p_lo … p_hi on the device: b.aff holds them side by side, in the file's form, when the stream has drained
template <class C>
int transform_blocks(hipStream_t st, const Buffers& b, uint64_t avail, uint32_t p_lo, uint32_t p_hi, uint32_t power)
{
  typedef typename C::A A;
  typedef typename C::P P;
  const uint64_t n = ((uint64_t)2 << p_hi) - ((uint64_t)1 << p_lo);
  A* const d_a = (A*)b.aff;
  P* const d_p = (P*)b.proj;
  auto to_file_form = [&] { return pv::to_file_form<C>(st, d_p, n, d_a, (typename Group<C>::Fo::T*)b.scratch); };
  DEV_LAUNCH("load kernel launch", (pp_load_kernel<C>), dim3((uint32_t)((n + PP_WG - 1) / PP_WG)), dim3(PP_WG), st, (const A*)b.src, avail, p_lo, n, (const ZcDigits*)b.inv, d_p);
  if (int rc = to_file_form()) return rc;
  for (uint32_t s = 0; s < p_hi; s++) {
    const uint64_t first = (uint64_t)1 << (std::max(p_lo, s + 1) - 1), count = ((uint64_t)1 << p_hi) - first;
    const dim3 grid((uint32_t)((count + PP_WG - 1) / PP_WG));
    // ω_(s+1)^(−j) = (root of order 2^(power+1))^(−j·2^(power−s)): j < 2^s ≤ 2^(p_hi−1) ≤ 2^power keeps the index below the table's 2^power
    if (s == 0) DEV_LAUNCH("level kernel launch", (pp_level_kernel<C, true>), grid, dim3(PP_WG), st, (const A*)d_a, first, count, s, p_lo, (const fe*)b.tw, power - s, d_p);
    else DEV_LAUNCH("level kernel launch", (pp_level_kernel<C, false>), grid, dim3(PP_WG), st, (const A*)d_a, first, count, s, p_lo, (const fe*)b.tw, power - s, d_p);
    if (int rc = to_file_form()) return rc;
  }
  return 0;
}

using pv::Sink;

int prepare_impl(const uint8_t* data, size_t len, const char* device, Groth16PtauPrepareReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  if (int rc = pv::ptau_unprepared_layout(data, len, secs, &L)) return rc;
  const uint32_t power = L.power;
  rep->power = power;
  const uint64_t N = (uint64_t)1 << power;
  uint64_t total = len;
  for (int k = 0; k < 4; k++) {
    const uint64_t bytes = pv::ptau_prepared_section_bytes(power, 12 + k);
    rep->points[k] = bytes / (k == 1 ? 128 : 64);
    total += 12 + bytes;
  }
  rep->ptau_bytes = total;
  // section 12's block power + 1 is a transform of size 2^(power+1)
  if (power > 27) return pv::fail(pv::ERR_ARG, "ptau: power %u: section 12's block for power %u needs a root of unity of order 2^%u, the field has 2^28", power, power + 1, power + 1);
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;
  auto fault = [&](int section, uint64_t element, int kind) {
    pv::set_point_fault(rep, section, element, kind);
    return pv::ptau_point_fail(section, element, kind);
  };
  {
    fe2 beta2[2];
    memcpy(beta2, L.sec[6]->p, 128);
    if (const int kind = p29::classify_g2(beta2)) return fault(6, 0, kind);
  }

  pv::StageTrace trace("ptau-prepare", "ICICLE_SNARK_TRACE_PTAU_PREPARE");
  std::vector<fe> tw;
  if (int rc = twiddle_table(power, tw)) return rc;
  trace.lap("layout, twiddles");

  // the input as it is, the section count four higher; the new sections' headers
  memcpy(out, data, len);
  {
    uint32_t nsec;
    memcpy(&nsec, data + 8, 4);
    nsec += 4;
    memcpy(out + 8, &nsec, 4);
  }
  trace.lap("sections 1 to 7 copied");

  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  // every section's largest block has 2^(power+1) G1 points or 2^power G2 points: the same bytes
  const size_t top = (size_t)(2 * N);
  Buffers b;
  b.src = ds.buf.alloc<uint8_t>(top * sizeof(G1::A));
  b.aff = ds.buf.alloc<uint8_t>(top * sizeof(G1::A));
  b.proj = ds.buf.alloc<uint8_t>(top * sizeof(G1::P));
  b.scratch = ds.buf.alloc<uint8_t>(top * sizeof(fe));
  b.tw = ds.buf.alloc<fe>(tw.size());
  b.inv = ds.buf.alloc<ZcDigits>(INV_COUNT);
  b.first = ds.buf.alloc<unsigned long long>(1);
  if (!b.src || !b.aff || !b.proj || !b.scratch || !b.tw || !b.inv || !b.first) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  static_assert(sizeof(G2::A) == 2 * sizeof(G1::A) && sizeof(G2::P) == 2 * sizeof(G1::P), "a G2 block of 2^power points fills the buffers of a G1 block of 2^(power+1)");
  if (int rc = pv::timed_upload(dev, b.tw, tw.data(), tw.size() * sizeof(fe), &rep->upload_ms)) return rc;
  {
    ZcDigits inv[INV_COUNT];
    for (uint32_t p = 0; p < INV_COUNT; p++) inv[p] = zc29::zc_recode(inverse_of_two_to(p));
    if (int rc = pv::timed_upload(dev, b.inv, inv, sizeof inv, &rep->upload_ms)) return rc;
  }
  trace.lap("twiddles uploaded");

  uint8_t* w = out + len;
  for (int k = 0; k < 4; k++) {
    const int sid = 12 + k, src_id = 2 + k;
    const bool g2 = sid == 13;
    const size_t elem = g2 ? 128 : 64;
    const uint64_t avail = L.sec[src_id]->size / elem, bytes = pv::ptau_prepared_section_bytes(power, sid);
    const uint32_t blocks = power + (sid == 12 ? 2 : 1);
    {
      const uint32_t id = (uint32_t)sid;
      memcpy(w, &id, 4);
      memcpy(w + 4, &bytes, 8);
      w += 12;
    }
    // up, and through the lane tests before anything else reads it
    if (int rc = pv::timed_upload(dev, b.src, L.sec[src_id]->p, (size_t)(avail * elem), &rep->upload_ms)) return rc;
    DEV_TRY("hipMemset", hipMemsetAsync(b.first, 0xff, sizeof *b.first, st));
    if (int rc = enqueue_lane_test(st, g2, b.src, avail, b.first)) return rc;
    unsigned long long first = NO_FAULT;
    DEV_TRY("download", hipMemcpyAsync(&first, b.first, sizeof first, hipMemcpyDeviceToHost, st));
    DEV_TRY("lane tests", hipStreamSynchronize(st));
    if (first != NO_FAULT) return fault(src_id, first >> 3, (int)(first & 7));
    // two passes: the blocks below the top one side by side — together one element shorter than the top block, so they fit its
    // buffers, and their levels are launched once and not once per block — then the top block alone
    const uint32_t top_block = blocks - 1;
    const uint32_t ranges[2][2] = {{0, top_block ? top_block - 1 : 0}, {top_block, top_block}};
    for (int pass = top_block ? 0 : 1; pass < 2; pass++) {
      const uint32_t p_lo = ranges[pass][0], p_hi = ranges[pass][1];
      if (int rc = g2 ? transform_blocks<G2>(st, b, avail, p_lo, p_hi, power) : transform_blocks<G1>(st, b, avail, p_lo, p_hi, power)) return rc;
      DEV_TRY("transform kernels", hipStreamSynchronize(st));
      const auto t_down = std::chrono::steady_clock::now();
      const uint64_t first_elem = ((uint64_t)1 << p_lo) - 1, count = ((uint64_t)2 << p_hi) - ((uint64_t)1 << p_lo);
      const isnark::CopyJob job = {w + first_elem * elem, b.aff, (size_t)(count * elem)};
      DEV_TRY("device to host download", isnark::staged_copy(dev, &job, 1, false));
      rep->download_ms += pv::ms_since(t_down);
    }
    w += bytes;
    if (trace.on) {
      char what[32];
      snprintf(what, sizeof what, "section %d done", sid);
      trace.lap(what);
    }
  }
  rep->device_ms = pv::ms_since(t_dev) - rep->download_ms;
  return 0;
}

} // namespace

ISNARK_API int groth16_ptau_prepare(const void* ptau, size_t len, void* out, size_t cap, uint64_t* out_len, const char* device, Groth16PtauPrepareReport* report)
{
  if (!out_len) return pv::fail(pv::ERR_ARG, "null out_len");
  *out_len = 0;
  if (int rc = prepare_impl((const uint8_t*)ptau, len, device, report, pv::buffer_sink("prepared file", out, cap))) return rc;
  *out_len = report->ptau_bytes;
  return 1;
}

ISNARK_API int groth16_ptau_prepare_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPrepareReport* report)
{
  const int rc = pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr,
                                  [&](const uint8_t* data, size_t len, const Sink& sink) { return prepare_impl(data, len, device, report, sink); });
  return rc ? rc : 1;
}
