// ptau_pack.hip — groth16_ptau_pack / groth16_ptau_unpack: a powers-of-tau file with every point as x and one bit of y, half the
// bytes, and back; groth16_points_pack / groth16_points_unpack: the same over a plain buffer of points.  include/groth16_prover.h
// has the contract and the packed container; point_pack29.h the packed point and its lane code; DESIGN.md §7j.  enqueue_point_ranges
// (prover_internal.h) is how the ranges of this tool and of the packed proving key (zkey_pack.hip) go up and through their launches.
//
//   host, first  the container — a .ptau in either form (ptau_either_layout) for pack, a packed file (ptau_packed_layout) for unpack:
//                both bound every point section to its exact element count before a byte goes up — the output's size against the
//                room, section 6 through the lane code on the host.
//   device       every other point section goes up and through ONE launch, a lane per point.  pack: zkey_check29.h's lane test
//                (the G2 sections with the subgroup test), then x and the sign of y — so a file packed here always unpacks.
//                unpack: the flags, x < q, the root of x³ + b — 252 squares and 97 products in Fq for G1, two such walks for G2 —
//                the sign, and for G2 the subgroup test.  A faulty lane writes zeros and tallies: per section the lowest faulty
//                element and a count.  unpack_on_device leaves file-form points in a device buffer: a later reader of packed files
//                needs no host round trip.
//   host, last   ALL verdicts are read before anything is written.  Then the container — the other magic, the sections in the
//                input's order, section 1, 7 and any unknown section byte for byte — and the sections come down into their places.
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "device_call.h"
#include "pack_device.h"
#include "point_pack29.h"
#include "prover_internal.h"
#include "verify_batch.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int PK_WG_G1 = 256, PK_WG_G2 = 64;
constexpr int MAX_SECTIONS = 8; // 2 … 5 and 12 … 15 (section 6 is the host's)

typedef pv::PackTally Tally; // min over the faulty lanes of (index << 3 | kind), NO_FAULT without one; their number
using pv::NO_FAULT;
using pv::POINT_FAULT;
using pv::tally_fault; // pack_device.h

// One lane per point, pts[i] → out[i], i < n.  A faulty point leaves a zero word (never a valid one: the identity has its flag).
template <bool G2>
__global__ __launch_bounds__(G2 ? PK_WG_G2 : PK_WG_G1) void pk_pack_kernel(const fe* __restrict__ pts, uint64_t n, fe* __restrict__ out, Tally* __restrict__ tally)
{
  const uint64_t i = (uint64_t)blockIdx.x * (G2 ? PK_WG_G2 : PK_WG_G1) + threadIdx.x;
  if (i >= n) return;
  if (G2) {
    const fe2 p[2] = {{ld(pts + 4 * i), ld(pts + 4 * i + 1)}, {ld(pts + 4 * i + 2), ld(pts + 4 * i + 3)}};
    fe2 w = {pk29::pk_zero_word(), pk29::pk_zero_word()};
    const int kind = p29::classify_g2(p);
    if (kind) tally_fault(tally, i, kind);
    else pk29::pk_pack_g2(p, &w);
    st(out + 2 * i, w.c0);
    st(out + 2 * i + 1, w.c1);
  } else {
    const fe p[2] = {ld(pts + 2 * i), ld(pts + 2 * i + 1)};
    fe w = pk29::pk_zero_word();
    const int kind = p29::classify_g1(p);
    if (kind) tally_fault(tally, i, kind);
    else pk29::pk_pack_g1(p, &w);
    st(out + i, w);
  }
}

// One lane per packed word, words[i] → out[i] in the file's form, i < n.  A faulty word leaves all-zero words and its tally.
template <bool G2>
__global__ __launch_bounds__(G2 ? PK_WG_G2 : PK_WG_G1) void pk_unpack_kernel(const fe* __restrict__ words, uint64_t n, fe* __restrict__ out, Tally* __restrict__ tally)
{
  const uint64_t i = (uint64_t)blockIdx.x * (G2 ? PK_WG_G2 : PK_WG_G1) + threadIdx.x;
  if (i >= n) return;
  if (G2) {
    const fe2 w = {ld(words + 2 * i), ld(words + 2 * i + 1)};
    fe2 p[2] = {{pk29::pk_zero_word(), pk29::pk_zero_word()}, {pk29::pk_zero_word(), pk29::pk_zero_word()}};
    const int kind = pk29::pk_unpack_g2(w, p);
    if (kind) tally_fault(tally, i, kind);
    st(out + 4 * i, p[0].c0);
    st(out + 4 * i + 1, p[0].c1);
    st(out + 4 * i + 2, p[1].c0);
    st(out + 4 * i + 3, p[1].c1);
  } else {
    const fe w = ld(words + i);
    fe p[2] = {pk29::pk_zero_word(), pk29::pk_zero_word()};
    const int kind = pk29::pk_unpack_g1(w, p);
    if (kind) tally_fault(tally, i, kind);
    st(out + 2 * i, p[0]);
    st(out + 2 * i + 1, p[1]);
  }
}

constexpr size_t FILE_BYTES[2] = {64, 128}, PACKED_BYTES[2] = {32, 64}; // [g2]

} // namespace

namespace isnark {
namespace prover {
// n packed words at d_words → n file-form points at d_out, both on the device; the faults into *d_tally (reset by the caller).
// (prover_internal.h: the packed proving key, zkey_pack.hip and cache.cpp, runs its point sections through the same two.)
int unpack_on_device(hipStream_t st, const uint8_t* d_words, uint64_t n, bool g2, uint8_t* d_out, Tally* d_tally)
{
  if (!n) return 0;
  if (g2) DEV_LAUNCH("unpack kernel launch", pk_unpack_kernel<true>, dim3((uint32_t)((n + PK_WG_G2 - 1) / PK_WG_G2)), dim3(PK_WG_G2), st, (const fe*)d_words, n, (fe*)d_out, d_tally);
  else DEV_LAUNCH("unpack kernel launch", pk_unpack_kernel<false>, dim3((uint32_t)((n + PK_WG_G1 - 1) / PK_WG_G1)), dim3(PK_WG_G1), st, (const fe*)d_words, n, (fe*)d_out, d_tally);
  return 0;
}
int pack_on_device(hipStream_t st, const uint8_t* d_points, uint64_t n, bool g2, uint8_t* d_out, Tally* d_tally)
{
  if (!n) return 0;
  if (g2) DEV_LAUNCH("pack kernel launch", pk_pack_kernel<true>, dim3((uint32_t)((n + PK_WG_G2 - 1) / PK_WG_G2)), dim3(PK_WG_G2), st, (const fe*)d_points, n, (fe*)d_out, d_tally);
  else DEV_LAUNCH("pack kernel launch", pk_pack_kernel<false>, dim3((uint32_t)((n + PK_WG_G1 - 1) / PK_WG_G1)), dim3(PK_WG_G1), st, (const fe*)d_points, n, (fe*)d_out, d_tally);
  return 0;
}
int enqueue_point_ranges(vb::DeviceSession& ds, int dev, bool unpack, PointRange* ranges, size_t count, Tally* d_tally, double* upload_ms)
{
  const hipStream_t st = ds.stream(0);
  for (size_t k = 0; k < count; k++) {
    PointRange& r = ranges[k];
    const size_t in_elem = (unpack ? PACKED_BYTES : FILE_BYTES)[r.g2], out_elem = (unpack ? FILE_BYTES : PACKED_BYTES)[r.g2];
    if (!r.n) continue;
    r.d_in = ds.buf.alloc<uint8_t>((size_t)(r.n * in_elem));
    r.d_out = ds.buf.alloc<uint8_t>((size_t)(r.n * out_elem));
    if (!r.d_in || !r.d_out) return dev_fail("hipMalloc", hipErrorOutOfMemory);
    if (int rc = timed_upload(dev, r.d_in, r.src, (size_t)(r.n * in_elem), upload_ms)) return rc;
    if (int rc = unpack ? unpack_on_device(st, r.d_in, r.n, r.g2, r.d_out, d_tally + k) : pack_on_device(st, r.d_in, r.n, r.g2, r.d_out, d_tally + k)) return rc;
  }
  return 0;
}
} // namespace prover
} // namespace isnark

namespace {
typedef pv::PointRange Range;

// ranges up and through their kernels; tallies[k] is range k's.  Every upload has landed and every kernel has run on return.
int run_ranges_on_device(vb::DeviceSession& ds, int dev, bool unpack, std::vector<Range>& ranges, Tally* tallies, double* upload_ms)
{
  const hipStream_t st = ds.stream(0);
  const size_t nr = ranges.size();
  Tally* const d_tally = ds.buf.alloc<Tally>(nr);
  if (!d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  if (int rc = pv::reset_tallies(tallies, d_tally, nr, st)) return rc;
  if (int rc = pv::enqueue_point_ranges(ds, dev, unpack, ranges.data(), nr, d_tally, upload_ms)) return rc;
  DEV_TRY("download", hipMemcpyAsync(tallies, d_tally, nr * sizeof(Tally), hipMemcpyDeviceToHost, st));
  DEV_TRY("pack kernels", hipStreamSynchronize(st));
  return 0;
}
int download_ranges(int dev, bool unpack, const std::vector<Range>& ranges)
{
  std::vector<isnark::CopyJob> jobs;
  for (const Range& r : ranges)
    if (r.n) jobs.push_back({r.dst, r.d_out, (size_t)(r.n * (unpack ? FILE_BYTES : PACKED_BYTES)[r.g2])});
  if (!jobs.empty()) DEV_TRY("device to host download", isnark::staged_copy(dev, jobs.data(), jobs.size(), false));
  return 0;
}

using pv::parse_device;

// ---- groth16_points_pack / groth16_points_unpack
int points_impl(bool unpack, const void* in, uint64_t n, int g2, void* out, const char* device, Groth16PointsPackReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  rep->n = n;
  int dev;
  if (int rc = parse_device(device, &dev)) return rc;
  if (n && (!in || !out)) return pv::fail(pv::ERR_ARG, "null buffer");
  if (n > ((uint64_t)1 << 32)) return pv::fail(pv::ERR_ARG, "points: %llu points in one call, 2^32 is the most", (unsigned long long)n);
  if (!n) return 0;
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  std::vector<Range> ranges(1);
  ranges[0] = {0, g2 != 0, n, (const uint8_t*)in, (uint8_t*)out, nullptr, nullptr};
  Tally t;
  if (int rc = run_ranges_on_device(ds, dev, unpack, ranges, &t, &rep->upload_ms)) return rc;
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;
  if (t.first != NO_FAULT) {
    rep->fault_index = t.first >> 3, rep->fault_kind = (int32_t)(t.first & 7), rep->fault_count = t.count;
    return pv::fail(pv::ERR_FORMAT, "points: element %llu: %s", (unsigned long long)rep->fault_index, POINT_FAULT[rep->fault_kind & 3]);
  }
  const auto t_down = std::chrono::steady_clock::now();
  if (int rc = download_ranges(dev, unpack, ranges)) return rc;
  rep->download_ms = pv::ms_since(t_down);
  return 0;
}

// ---- groth16_ptau_pack / groth16_ptau_unpack
bool is_point_section(uint32_t id, bool prepared) { return (id >= 2 && id <= 6) || (prepared && id >= 12 && id <= 15); }
bool is_g2_section(uint32_t id) { return id == 3 || id == 6 || id == 13; }

using pv::Sink;

int file_impl(bool unpack, const uint8_t* data, size_t len, const char* device, Groth16PtauPackReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  pv::PtauLayout L;
  bool prepared = false;
  if (int rc = unpack ? pv::ptau_packed_layout(data, len, secs, &L, &prepared) : pv::ptau_either_layout(data, len, secs, &L, &prepared)) return rc;
  rep->power = L.power;
  rep->prepared = prepared ? 1 : 0;
  rep->in_bytes = len;

  // the ranges and the output's size, before anything else is done: the layout has tied every section to its element count
  std::vector<Range> ranges;
  uint64_t total = len;
  for (uint32_t id = 2; id < 16; id++) {
    if (!is_point_section(id, prepared)) continue;
    const bool g2 = is_g2_section(id);
    const uint64_t n = L.sec[id]->size / (unpack ? PACKED_BYTES : FILE_BYTES)[g2];
    rep->points[g2] += n;
    if (unpack) total += n * PACKED_BYTES[g2];
    else total -= n * PACKED_BYTES[g2];
    if (id != 6) ranges.push_back({(int)id, g2, n, L.sec[id]->p, nullptr, nullptr, nullptr});
  }
  rep->out_bytes = total;
  uint8_t* out = nullptr;
  if (int rc = sink(total, &out)) return rc;
  auto fault = [&](int section, uint64_t element, int kind, uint64_t count) {
    pv::set_point_fault(rep, section, element, kind), rep->fault_count = count;
    return pv::ptau_point_fail(section, element, kind);
  };
  // section 6 on the host, through the same lane code
  fe2 beta2_in[2], beta2_out[2];
  if (unpack) {
    memcpy(beta2_in, L.sec[6]->p, 64);
    if (const int kind = pk29::pk_unpack_g2(beta2_in[0], beta2_out)) return fault(6, 0, kind, 1);
  } else {
    memcpy(beta2_in, L.sec[6]->p, 128);
    if (const int kind = p29::classify_g2(beta2_in)) return fault(6, 0, kind, 1);
    pk29::pk_pack_g2(beta2_in, &beta2_out[0]);
  }

  pv::StageTrace trace(unpack ? "ptau-unpack" : "ptau-pack", "ICICLE_SNARK_TRACE_PTAU_PACK");
  trace.lap("layout, section 6");
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  Tally tallies[MAX_SECTIONS];
  if (int rc = run_ranges_on_device(ds, dev, unpack, ranges, tallies, &rep->upload_ms)) return rc;
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;
  trace.lap("sections up, kernels");
  // every verdict is in; nothing has been written
  for (size_t k = 0; k < ranges.size(); k++)
    if (tallies[k].first != NO_FAULT) return fault(ranges[k].section, tallies[k].first >> 3, (int)(tallies[k].first & 7), tallies[k].count);

  // ---- the container: the other magic, the sections in the input's order
  uint8_t* w = out;
  const std::vector<pv::SectionEntry> order = pv::sections_in_order(data);
  pv::put_container_head(w, unpack ? "ptau" : "ptaz", 1, (uint32_t)order.size());
  for (const pv::SectionEntry& e : order) {
    const bool point = is_point_section(e.id, prepared);
    const uint64_t size = !point ? e.size : unpack ? 2 * e.size : e.size / 2;
    pv::put_section(w, e.id, size);
    if (!point) memcpy(w, e.p, (size_t)e.size);
    else if (e.id == 6) memcpy(w, beta2_out, (size_t)size);
    else
      for (Range& r : ranges)
        if (r.section == (int)e.id) r.dst = w;
    w += size;
  }
  trace.lap("container, copied sections");
  const auto t_down = std::chrono::steady_clock::now();
  if (int rc = download_ranges(dev, unpack, ranges)) return rc;
  rep->download_ms = pv::ms_since(t_down);
  trace.lap("sections downloaded");
  return 0;
}

int buffer_entry(bool unpack, const void* in, size_t len, void* out, size_t cap, const char* device, Groth16PtauPackReport* report)
{
  return file_impl(unpack, (const uint8_t*)in, len, device, report, pv::buffer_sink("file", out, cap));
}

// a _file entry: the report zeroed before the paths are judged
int file_entry(bool unpack, const char* in_path, const char* out_path, const char* device, Groth16PtauPackReport* report)
{
  if (report) memset(report, 0, sizeof *report);
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr,
                          [&](const uint8_t* data, size_t len, const Sink& sink) { return file_impl(unpack, data, len, device, report, sink); });
}

} // namespace

ISNARK_API int groth16_points_pack(const void* points, uint64_t n, int g2, void* out, const char* device, Groth16PointsPackReport* report)
{
  return points_impl(false, points, n, g2, out, device, report);
}
ISNARK_API int groth16_points_unpack(const void* packed, uint64_t n, int g2, void* out, const char* device, Groth16PointsPackReport* report)
{
  return points_impl(true, packed, n, g2, out, device, report);
}
ISNARK_API int groth16_ptau_pack(const void* ptau, size_t len, void* out, size_t cap, const char* device, Groth16PtauPackReport* report)
{
  return buffer_entry(false, ptau, len, out, cap, device, report);
}
ISNARK_API int groth16_ptau_unpack(const void* packed, size_t len, void* out, size_t cap, const char* device, Groth16PtauPackReport* report)
{
  return buffer_entry(true, packed, len, out, cap, device, report);
}
ISNARK_API int groth16_ptau_pack_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPackReport* report)
{
  return file_entry(false, in_path, out_path, device, report);
}
ISNARK_API int groth16_ptau_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16PtauPackReport* report)
{
  return file_entry(true, in_path, out_path, device, report);
}
