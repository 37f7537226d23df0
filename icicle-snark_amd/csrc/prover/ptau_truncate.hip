// ptau_truncate.hip — groth16_ptau_truncate: a powers-of-tau file of power P cut down to power p ≤ P, what `snarkjs powersoftau
// truncate` is for — with the one block that a prefix copy gets wrong made right on the GPU.  include/groth16_prover.h has the
// contract and the definition of the output; ptau_truncate29.h the lane; DESIGN.md §7m.
//
//   host, first  the container — a .ptau in either form (ptau_either_layout bounds every point section to its exact element count) —
//                p against P, the output's size against the room.  An unprepared file, or p = P, is finished here: prefixes of the
//                sections, section 1 with the new power, and NO device is opened.
//   device       (prepared, p < P) Q = element 2^(p+1) − 1 of section 2 goes through classify_g1 on the host, which builds its table;
//                section 12's block p + 1 and the tables go up — nothing else does — and the block through the same lane test
//                (ptau_g1_kernel's, with a tally): the verdict is read before any arithmetic and before anything is written.  Then ONE launch of pt_fix_kernel, a lane per element j of the block:
//                  B′_j = B_j − s_j·Q,  s_j = ω′^j/2^(p+1) from two small tables (ptau_contribute29.h's split, built by device_call.h's
//                split_power_tables), Q's table of 816 signed-window multiples staged in LDS (52 224 bytes a workgroup of 256 lanes:
//                three a CU), at most 51 mixed additions for s_j·Q and one for B_j, no doubling.  point_form.h's to_file_form puts
//                the block back in the file's form, the identity all zero.
//   host, last   the container in the input's order, the block down into its place.
//   The COPIED PREFIXES ARE NOT TESTED: they are bytes of the input, and groth16_ptau_verify judges a file.  Q the identity (no
//   honest file has one): nothing to subtract, the block is copied and no device is opened.
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "pack_device.h"
#include "point_form.h"
#include "prover_internal.h"
#include "ptau_truncate29.h"
#include "verify_batch.h"
#include "zkey_check29.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int PT_WG = 256;
constexpr uint32_t PT_GRID_MAX = 3072; // 256 CUs × 3 resident workgroups × 4: a workgroup strides over the block and stages the table once

typedef pv::PackTally Tally;
using pv::NO_FAULT;

// the lane test of the ranges that went up: pts[i], i < cnt, through classify_g1; the lowest faulty element and their number.
// This is ptau_ranges.h's ptau_g1_kernel plus the count the report's fault_count needs: that kernel is compiled into five objects
// and is not to change for one caller's count, so the test with a tally stays a kernel of this file.
__global__ __launch_bounds__(PT_WG) void pt_test_kernel(const fe* __restrict__ pts, uint64_t cnt, Tally* __restrict__ tally)
{
  const uint64_t i = (uint64_t)blockIdx.x * PT_WG + threadIdx.x;
  if (i >= cnt) return;
  const fe p[2] = {ld(pts + 2 * i), ld(pts + 2 * i + 1)};
  const int kind = p29::classify_g1(p);
  if (kind) pv::tally_fault(tally, i, kind);
}

// entry i of Q's table out of LDS: four 16-byte reads at an address the lane's digit chose
struct LdsFetch {
  const uint4* tab;
  __host__ __device__ G1::A operator()(uint32_t i) const
  {
    const uint4 a = tab[4 * i], b = tab[4 * i + 1], c = tab[4 * i + 2], d = tab[4 * i + 3];
    G1::A r;
    r.x.l[0] = a.x, r.x.l[1] = a.y, r.x.l[2] = a.z, r.x.l[3] = a.w, r.x.l[4] = b.x, r.x.l[5] = b.y, r.x.l[6] = b.z, r.x.l[7] = b.w;
    r.y.l[0] = c.x, r.y.l[1] = c.y, r.y.l[2] = c.z, r.y.l[3] = c.w, r.y.l[4] = d.x, r.y.l[5] = d.y, r.y.l[6] = d.z, r.y.l[7] = d.w;
    return r;
  }
};

// blk[j] − s_j·Q for j < n = 2^(p+1) as Montgomery projective, the identity (0, 1, 0).  table: pt_fill_table's 816 points; lo[i] = ω′^i
// for i < 2^k and hi[m] = (2n′)⁻¹·ω′^(m·2^k) for m < n ≫ k, Montgomery form.  The points have passed their lane test.
__global__ __launch_bounds__(PT_WG) void pt_fix_kernel(const G1::A* __restrict__ blk, uint64_t n, const uint4* __restrict__ table, const fe* __restrict__ lo, const fe* __restrict__ hi,
                                                       uint32_t k, G1::P* __restrict__ out)
{
  __shared__ uint4 s_tab[pt29::PT_LDS_BYTES / 16];
  for (uint32_t v = threadIdx.x; v < pt29::PT_LDS_BYTES / 16; v += PT_WG) s_tab[v] = table[v];
  __syncthreads();
  const LdsFetch fetch = {s_tab};
  for (uint64_t j = (uint64_t)blockIdx.x * PT_WG + threadIdx.x; j < n; j += (uint64_t)gridDim.x * PT_WG) {
    const G1::A b = blk[j];
    out[j] = G1::x_to_projective(G1L::x_store(pt29::pt_lane(b, ld(hi + (j >> k)), ld(lo + (j & (((uint64_t)1 << k) - 1))), fetch)));
  }
}

// ---- the container
// the bytes of section `id` of a file cut to power p (sections of a .ptau ptau_either_layout has passed); `size` its bytes now
uint64_t cut_bytes(uint32_t id, uint64_t size, uint32_t p, bool prepared)
{
  const uint64_t n = (uint64_t)1 << p;
  switch (id) {
  case 2: return (2 * n - 1) * 64;
  case 3: return n * 128;
  case 4:
  case 5: return n * 64;
  case 12:
  case 13:
  case 14:
  case 15: return prepared ? pv::ptau_prepared_section_bytes(p, (int)id) : size;
  default: return size; // 1, 6, 7 and any section this library does not know
  }
}
uint64_t cut_total(const uint8_t* data, uint32_t p, bool prepared)
{
  uint64_t total = 12;
  for (const pv::SectionEntry& e : pv::sections_in_order(data)) total += 12 + cut_bytes(e.id, e.size, p, prepared);
  return total;
}

struct Fix { // the device's part of one call
  uint64_t n = 0;         // 2^(p+1): the block's elements
  const uint8_t* block = nullptr;
  const uint8_t* q = nullptr;
  uint8_t* dst = nullptr; // the block's place in the output
};

using pv::Sink;

// `place` runs once the verdicts are in, while the fix kernels run: it writes the container and sets fx.dst
int fix_on_device(int dev, uint32_t p, Fix& fx, Groth16PtauTruncateReport* rep, pv::StageTrace& trace, const std::function<void()>& place)
{
  const uint64_t n = fx.n;
  // ---- the host's tables: the scalars' two, and Q's
  const uint32_t kbits = pc29::pc_table_bits(p);
  const size_t n_lo = (size_t)1 << kbits, n_hi = (size_t)1 << (p + 1 - kbits);
  std::vector<fe> tables(n_lo + n_hi);
  {
    fe w, order = Fr::zero();
    if (int rc = pv::root_of_unity(p + 1, &w)) return rc;
    order.l[0] = (uint32_t)n; // n ≤ 2^27
    const fe ninv_m = Fr::inv(Fr::to_mont(order));
    pv::split_power_tables(Fr::to_mont(w), kbits, n_hi, &ninv_m, 1, tables.data());
  }
  std::vector<G1::A> qtab(pt29::PT_TABLE_POINTS);
  G1::A q;
  memcpy(&q, fx.q, 64);
  {
    // Q through the same lane test on the host, before the host's own arithmetic reads it: a faulty Q is reported before the block
    const fe w[2] = {q.x, q.y};
    if (const int kind = p29::classify_g1(w)) {
      pv::set_point_fault(rep, 2, n - 1, kind), rep->fault_count = 1;
      return pv::ptau_point_fail(2, n - 1, kind);
    }
  }
  {
    G1::A bases[pt29::PT_WINDOWS];
    pt29::pt_fill_bases(q, bases);
    isnark::run_ranges(pt29::PT_WINDOWS, 1, [&](int, size_t lo, size_t hi) { pt29::pt_fill_rows(bases, (int)lo, (int)hi, qtab.data()); });
  }
  trace.lap("tables");

  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  uint8_t* const d_blk = ds.buf.alloc<uint8_t>((size_t)(n * sizeof(G1::A))); // the block, then the result
  uint8_t* const d_proj = ds.buf.alloc<uint8_t>((size_t)(n * sizeof(G1::P)));
  fe* const d_scratch = ds.buf.alloc<fe>((size_t)n);
  fe* const d_tables = ds.buf.alloc<fe>(tables.size());
  uint4* const d_qtab = ds.buf.alloc<uint4>(pt29::PT_LDS_BYTES / 16);
  Tally* const d_tally = ds.buf.alloc<Tally>(1);
  if (!d_blk || !d_proj || !d_scratch || !d_tables || !d_qtab || !d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  static_assert(sizeof(G1::A) == 64 && pt29::PT_TABLE_POINTS * sizeof(G1::A) == pt29::PT_LDS_BYTES, "a table entry is 64 bytes");
  Tally tally;
  if (int rc = pv::reset_tallies(&tally, d_tally, 1, st)) return rc;
  if (int rc = pv::timed_upload(dev, d_blk, fx.block, (size_t)(n * 64), &rep->upload_ms)) return rc;
  if (int rc = pv::timed_upload(dev, d_tables, tables.data(), tables.size() * sizeof(fe), &rep->upload_ms)) return rc;
  if (int rc = pv::timed_upload(dev, d_qtab, qtab.data(), pt29::PT_LDS_BYTES, &rep->upload_ms)) return rc;
  DEV_LAUNCH("lane test launch", pt_test_kernel, dim3((uint32_t)((n + PT_WG - 1) / PT_WG)), dim3(PT_WG), st, (const fe*)d_blk, n, d_tally);
  DEV_TRY("download", hipMemcpyAsync(&tally, d_tally, sizeof tally, hipMemcpyDeviceToHost, st));
  DEV_TRY("lane tests", hipStreamSynchronize(st));
  trace.lap("block up, lane tests");
  if (tally.first != NO_FAULT) {
    const uint64_t e = n - 1 + (tally.first >> 3); // block p + 1 begins at element 2^(p+1) − 1 of section 12
    const int kind = (int)(tally.first & 7);
    pv::set_point_fault(rep, 12, e, kind), rep->fault_count = tally.count;
    return pv::ptau_point_fail(12, e, kind);
  }

  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + PT_WG - 1) / PT_WG, PT_GRID_MAX);
  DEV_LAUNCH("fix kernel launch", pt_fix_kernel, dim3(grid), dim3(PT_WG), st, (const G1::A*)d_blk, n, (const uint4*)d_qtab, (const fe*)d_tables, (const fe*)(d_tables + n_lo), kbits,
             (G1::P*)d_proj);
  if (int rc = pv::to_file_form<G1>(st, (const G1::P*)d_proj, n, (G1::A*)d_blk, d_scratch)) return rc;
  const auto t_place = std::chrono::steady_clock::now();
  place();
  const double place_ms = pv::ms_since(t_place);
  trace.lap("container, copied sections");
  DEV_TRY("fix kernels", hipStreamSynchronize(st));
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms - place_ms;
  trace.lap("fix kernels");
  const auto t_down = std::chrono::steady_clock::now();
  const isnark::CopyJob job = {fx.dst, d_blk, (size_t)(n * 64)};
  DEV_TRY("device to host download", isnark::staged_copy(dev, &job, 1, false));
  rep->download_ms = pv::ms_since(t_down);
  rep->points_fixed = n;
  trace.lap("block downloaded");
  return 0;
}

int truncate_impl(const uint8_t* data, size_t len, uint32_t p, const char* device, Groth16PtauTruncateReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  bool prepared = false;
  if (int rc = pv::ptau_either_layout(data, len, secs, &L, &prepared)) return rc;
  const uint32_t P = L.power;
  rep->power_in = P, rep->power_out = p, rep->prepared = prepared ? 1 : 0, rep->in_bytes = len;
  if (p > P) return pv::fail(pv::ERR_ARG, "ptau: power %u is above the file's %u: a truncation lowers the power", p, P);
  const uint64_t total = p == P ? (uint64_t)len : cut_total(data, p, prepared);
  rep->out_bytes = total;
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;
  pv::StageTrace trace("ptau-truncate", "ICICLE_SNARK_TRACE_PTAU_TRUNCATE");
  if (p == P) { // the file itself
    memcpy(out, data, len);
    trace.lap("copied");
    return 0;
  }

  // ---- the container: the input's order, prefixes of the point sections, section 1 with the new power
  const uint64_t n2 = (uint64_t)2 << p; // 2n′: the elements of section 12's block p + 1
  Fix fx;
  const auto write_container = [&]() {
    memcpy(out, data, 12);
    uint8_t* w = out + 12;
    for (const pv::SectionEntry& e : pv::sections_in_order(data)) {
      const uint64_t size = cut_bytes(e.id, e.size, p, prepared);
      pv::put_section(w, e.id, size);
      if (e.id == 12 && prepared && fx.n) {
        const uint64_t head = (n2 - 1) * 64; // blocks 0 … p
        memcpy(w, e.p, (size_t)head);
        fx.dst = w + head;
      } else {
        memcpy(w, e.p, (size_t)size);
      }
      if (e.id == 1) memcpy(w + 36, &p, 4);
      w += size;
    }
  };
  if (prepared) {
    fx.block = L.sec[12]->p + (n2 - 1) * 64;
    fx.q = L.sec[2]->p + (n2 - 1) * 64; // p < P: section 2 holds 2^(P+1) − 1 ≥ 2^(p+2) − 1 elements
    G1::A q;
    memcpy(&q, fx.q, 64);
    if (!G1::aff_is_zero(q)) fx.n = n2; // Q the identity: nothing to subtract
  }
  if (!fx.n) {
    write_container();
    trace.lap("container, copied sections");
    return 0;
  }
  // the verdicts first: a faulty point leaves nothing written.  The block comes down last, into its place.
  return fix_on_device(dev, p, fx, rep, trace, write_container);
}

} // namespace

ISNARK_API int groth16_ptau_truncated_size(const void* ptau, size_t len, uint32_t power, uint64_t* bytes)
{
  if (!bytes) return pv::fail(pv::ERR_ARG, "null output");
  *bytes = 0;
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  bool prepared = false;
  if (int rc = pv::ptau_either_layout((const uint8_t*)ptau, len, secs, &L, &prepared)) return rc;
  if (power > L.power) return pv::fail(pv::ERR_ARG, "ptau: power %u is above the file's %u: a truncation lowers the power", power, L.power);
  *bytes = power == L.power ? (uint64_t)len : cut_total((const uint8_t*)ptau, power, prepared);
  return 0;
}

ISNARK_API int groth16_ptau_truncate(const void* ptau, size_t len, uint32_t power, void* out, size_t cap, const char* device, Groth16PtauTruncateReport* report)
{
  return truncate_impl((const uint8_t*)ptau, len, power, device, report, pv::buffer_sink("file", out, cap));
}

ISNARK_API int groth16_ptau_truncate_file(const char* in_path, const char* out_path, uint32_t power, const char* device, Groth16PtauTruncateReport* report)
{
  if (report) memset(report, 0, sizeof *report);
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr,
                          [&](const uint8_t* data, size_t len, const Sink& sink) { return truncate_impl(data, len, power, device, report, sink); });
}
