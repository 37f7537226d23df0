// wtns_pack.hip — a witness PACKED ("wtnz"): groth16_wtns_packed_size / _pack / _unpack_host (host only: they never initialise a
// GPU), groth16_wtns_unpack (one device) and wtnz_decode_on_device, the decode groth16_prove_packed (prover.cpp) and
// groth16_witness_check_packed (r1cs_check.hip) put in front of their unchanged device work.  include/groth16_prover.h has the
// contract and the container; wtns_pack.h the value's form and its lane code; containers.cpp the reader; pack_device.h the block
// codec's pieces (scan, span test, aligned load, word read), which zkey_pack.hip's kernels share; DESIGN.md §7k.
//
//   host, first  wtnz_layout bounds every section and the whole directory before a byte goes up: block b's payload
//                [dir[b], dir[b + 1]) lies inside section 4 and is at most 8192 bytes, whatever the codes say.
//   device       sections 2 … 4 go up and through ONE launch: a 256-lane workgroup per block, a lane per value.  The lane's code
//                gives its length; an exclusive scan of the 256 lengths — wave scans, four wave sums through LDS — gives its
//                offset, and the block's sum is compared with the directory span BEFORE any payload byte is read (a block whose
//                sum differs tallies DIRECTORY at its first element, writes zeros and reads nothing).  The block's payload comes
//                into LDS in aligned 16-byte loads (the buffer is padded and zeroed to the load width: the aligned over-read at
//                either end stays inside the allocation); each lane assembles its eight words from LDS, runs wz_decode_value and
//                stores its 32 bytes — consecutive lanes, consecutive rows.  A faulty lane writes zeros and tallies: the lowest
//                (element << 3 | kind) and a count.
//   host, last   ALL verdicts are read before the result is used or anything is written.
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "device_call.h"
#include "pack_device.h"
#include "prover_internal.h"
#include "verify_batch.h"
#include "wtns_pack.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;

constexpr int WZ_WG = (int)wz::WZ_BLOCK;
static_assert(WZ_WG == pv::PACK_WG, "pack_device.h's block codec is a 256-lane workgroup's");
typedef pv::PackTally Tally;
using pv::pad16;

// Block blockIdx.x of a packed witness → out[256·b … 256·b + 255] (standard form), i < n.  `payload` is 16-byte aligned and the
// allocation reaches the next multiple of 16 behind its last byte; `dir` has passed wz_check_directory.
__global__ __launch_bounds__(WZ_WG) void wz_unpack_kernel(const uint8_t* __restrict__ codes, const unsigned long long* __restrict__ dir, const uint8_t* __restrict__ payload, uint32_t n,
                                                          fe* __restrict__ out, Tally* __restrict__ tally)
{
  __shared__ uint4 s_pay[pv::PACK_LDS_VEC];
  __shared__ uint32_t s_wave[WZ_WG / 64];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * WZ_WG + t;
  const bool live = i < n;
  const uint8_t code = live ? codes[i] : wz::WZ_CODE_ZERO;
  const int cl = wz::wz_code_len(code);
  const uint32_t len = cl > 0 ? (uint32_t)cl : 0;
  uint32_t off, total;
  pv::block_scan(len, s_wave, &off, &total);

  unsigned long long lo;
  uint32_t head;
  fe row;
#pragma unroll
  for (int k = 0; k < 8; k++) row.l[k] = 0;
  if (!pv::block_span(dir, total, &lo, &head)) { // nothing of the payload is read
    if (t == 0) pv::tally_fault(tally, i, wz::WZ_DIRECTORY);
    if (live) out[i] = row;
    return;
  }
  pv::block_payload_to_lds(payload, lo, head, total, s_pay);
  __syncthreads();
  if (!live) return;
  uint32_t pay[8] = {};
  pv::lane_payload_words(s_pay, head + off, len, pay);
  if (const int kind = wz::wz_decode_value(code, pay, row.l)) pv::tally_fault(tally, i, kind);
  out[i] = row;
}

struct DeviceLayout { // of d_buf
  size_t tally = 0, dir, codes, payload, total;
  explicit DeviceLayout(const pv::WtnzLayout& L)
  {
    dir = 16;
    codes = dir + pad16((size_t)(L.n_blocks + 1) * 8);
    payload = codes + pad16(L.n_witness) + 16;
    total = payload + pad16((size_t)L.payload_bytes) + 16;
  }
};

} // namespace

namespace isnark {
namespace prover {

int wtnz_fail(const WtnzFault& f) { return fail(ERR_FORMAT, "wtnz: element %llu: %s", (unsigned long long)f.element, wz::wz_fault_text(f.kind)); }

size_t wtnz_device_bytes(const WtnzLayout& L) { return DeviceLayout(L).total; }

int wtnz_decode_on_device(int dev, hipStream_t st, const WtnzLayout& L, uint8_t* d_buf, fe* d_out, WtnzFault* fault, double* upload_ms, double* kernel_ms)
{
  *fault = WtnzFault();
  if (kernel_ms) *kernel_ms = 0;
  if (!L.n_witness) return 0;
  const DeviceLayout D(L);
  Tally t;
  if (int rc = reset_tallies(&t, (Tally*)(d_buf + D.tally), 1, st)) return rc;
  // the padding behind the codes and behind the payload: what an aligned over-read sees is zero
  DEV_TRY("hipMemsetAsync", hipMemsetAsync(d_buf + D.codes + L.n_witness, 0, D.payload - D.codes - L.n_witness, st));
  DEV_TRY("hipMemsetAsync", hipMemsetAsync(d_buf + D.payload + L.payload_bytes, 0, D.total - D.payload - (size_t)L.payload_bytes, st));
  const auto t_up = std::chrono::steady_clock::now();
  const CopyJob jobs[3] = {{d_buf + D.codes, L.codes, L.n_witness}, {d_buf + D.dir, L.dir, (size_t)(L.n_blocks + 1) * 8}, {d_buf + D.payload, L.payload, (size_t)L.payload_bytes}};
  if (hipError_t he = staged_copy(dev, jobs, L.payload_bytes ? 3 : 2, true)) return dev_fail("host to device upload", he);
  if (upload_ms) *upload_ms += ms_since(t_up);
  hipEvent_t ev[2] = {nullptr, nullptr};
  struct DestroyEvents {
    hipEvent_t* e;
    ~DestroyEvents()
    {
      for (int k = 0; k < 2; k++)
        if (e[k]) (void)hipEventDestroy(e[k]);
    }
  } destroy{ev};
  if (kernel_ms) {
    DEV_TRY("hipEventCreate", hipEventCreate(&ev[0]));
    DEV_TRY("hipEventCreate", hipEventCreate(&ev[1]));
    DEV_TRY("hipEventRecord", hipEventRecord(ev[0], st));
  }
  DEV_LAUNCH("unpack kernel launch", wz_unpack_kernel, dim3((uint32_t)L.n_blocks), dim3(WZ_WG), st, (const uint8_t*)(d_buf + D.codes), (const unsigned long long*)(d_buf + D.dir),
             (const uint8_t*)(d_buf + D.payload), L.n_witness, d_out, (Tally*)(d_buf + D.tally));
  if (kernel_ms) DEV_TRY("hipEventRecord", hipEventRecord(ev[1], st));
  DEV_TRY("download", hipMemcpyAsync(&t, d_buf + D.tally, sizeof t, hipMemcpyDeviceToHost, st));
  DEV_TRY("unpack kernel", hipStreamSynchronize(st));
  if (kernel_ms) {
    float ms = 0;
    DEV_TRY("hipEventElapsedTime", hipEventElapsedTime(&ms, ev[0], ev[1]));
    *kernel_ms = ms;
  }
  if (t.first != NO_FAULT) fault->kind = (int)(t.first & 7), fault->element = t.first >> 3, fault->count = t.count;
  return 0;
}

} // namespace prover
} // namespace isnark

namespace {

constexpr uint64_t WTNS_HEAD = 12 + (12 + 40) + 12;  // a .wtns of sections 1 and 2 up to its first value
constexpr uint64_t WTNZ_HEAD = 12 + 4 * 12 + 40;     // a packed witness without its codes, directory and payload

using pv::put_section;
using pv::Sink;

// ---- pack (host)
// the codes, the directory and the payload's size of a .wtns' values; a value >= r is ERR_FORMAT naming the lowest
int pack_scan(const pv::Wtns& w, std::vector<uint8_t>* codes, std::vector<uint64_t>& dir, Groth16WtnsPackReport* rep)
{
  const uint64_t n = w.n_witness, nb = (n + wz::WZ_BLOCK - 1) / wz::WZ_BLOCK;
  if (!Fr::eq(w.q, Fr::modulus())) return pv::fail(pv::ERR_FORMAT, "wtns: the prime is not the BN254 scalar field's");
  if (codes) codes->resize((size_t)n);
  dir.assign((size_t)nb + 1, 0);
  uint64_t pos = 0, bad = 0, first_bad = 0;
  for (uint64_t e = 0; e < n; e++) {
    if (e % wz::WZ_BLOCK == 0) dir[(size_t)(e / wz::WZ_BLOCK)] = pos;
    uint8_t code = 0, pay[32];
    const int len = wz::wz_encode_value(w.values + 32 * e, &code, pay);
    if (len < 0) {
      if (!bad++) first_bad = e;
      continue;
    }
    if (codes) (*codes)[(size_t)e] = code;
    pos += (uint64_t)len;
  }
  dir[(size_t)nb] = pos;
  if (bad) {
    if (rep) rep->fault_kind = GROTH16_WTNZ_RANGE, rep->fault_index = first_bad, rep->fault_count = bad;
    return pv::fail(pv::ERR_FORMAT, "wtns: element %llu is not below r", (unsigned long long)first_bad);
  }
  return 0;
}

int pack_impl(const uint8_t* data, size_t len, Groth16WtnsPackReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!data) return pv::fail(pv::ERR_ARG, "null wtns");
  pv::Wtns w;
  if (int rc = pv::parse_wtns(data, len, w)) return rc;
  rep->n_witness = w.n_witness;
  rep->in_bytes = len;
  std::vector<uint8_t> codes;
  std::vector<uint64_t> dir;
  if (int rc = pack_scan(w, &codes, dir, rep)) return rc;
  const uint64_t payload = dir.back();
  rep->out_bytes = WTNZ_HEAD + codes.size() + 8 * dir.size() + payload;
  uint8_t* out = nullptr;
  if (int rc = sink(rep->out_bytes, &out)) return rc;
  uint8_t* p = out;
  pv::put_container_head(p, "wtnz", 1, 4);
  put_section(p, 1, 40); // the .wtns header byte for byte (parse_wtns has demanded exactly these 40 bytes)
  memcpy(p, &w.n8, 4);
  memcpy(p + 4, w.q.l, 32);
  memcpy(p + 36, &w.n_witness, 4);
  p += 40;
  put_section(p, 2, codes.size());
  if (!codes.empty()) memcpy(p, codes.data(), codes.size());
  p += codes.size();
  put_section(p, 3, 8 * dir.size());
  memcpy(p, dir.data(), 8 * dir.size());
  p += 8 * dir.size();
  put_section(p, 4, payload);
  for (uint64_t e = 0; e < w.n_witness; e++) {
    uint8_t code, pay[32];
    const int l = wz::wz_encode_value(w.values + 32 * e, &code, pay);
    memcpy(p, pay, (size_t)l);
    p += l;
  }
  return 0;
}

// ---- unpack: the .wtns a packed witness came from, sections 1 and 2 under version 2
void put_wtns_head(uint8_t* p, const pv::WtnzLayout& L)
{
  pv::put_container_head(p, "wtns", 2, 2);
  put_section(p, 1, 40);
  memcpy(p, L.header, 40);
  p += 40;
  put_section(p, 2, (uint64_t)L.n_witness * 32);
}

int unpack_prologue(const uint8_t* data, size_t len, Groth16WtnsPackReport* rep, pv::WtnzLayout* L)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (int rc = pv::wtnz_layout(data, len, L)) return rc;
  if (int rc = pv::wtnz_is_bn254(*L)) return rc;
  rep->n_witness = L->n_witness;
  rep->in_bytes = len;
  rep->out_bytes = WTNS_HEAD + (uint64_t)L->n_witness * 32;
  return 0;
}
int report_fault(Groth16WtnsPackReport* rep, const pv::WtnzFault& f)
{
  rep->fault_kind = f.kind, rep->fault_index = f.element, rep->fault_count = f.count;
  return pv::wtnz_fail(f);
}

int unpack_host_impl(const uint8_t* data, size_t len, Groth16WtnsPackReport* rep, const Sink& sink)
{
  pv::WtnzLayout L;
  if (int rc = unpack_prologue(data, len, rep, &L)) return rc;
  uint8_t* out = nullptr;
  if (int rc = sink(rep->out_bytes, &out)) return rc;
  // (decoded apart: a fault must leave the caller's buffer as it was)
  std::vector<uint8_t> values((size_t)L.n_witness * 32);
  wz::WzView view;
  view.n = L.n_witness, view.codes = L.codes, view.dir = L.dir, view.payload = L.payload;
  pv::WtnzFault f;
  f.kind = wz::wz_decode_host(view, 0, L.n_witness, values.data(), &f.element, &f.count);
  if (f.kind) return report_fault(rep, f);
  put_wtns_head(out, L);
  if (!values.empty()) memcpy(out + WTNS_HEAD, values.data(), values.size());
  return 0;
}

int unpack_device_impl(const uint8_t* data, size_t len, const char* device, Groth16WtnsPackReport* rep, const Sink& sink)
{
  pv::WtnzLayout L;
  if (int rc = unpack_prologue(data, len, rep, &L)) return rc;
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  uint8_t* out = nullptr;
  if (int rc = sink(rep->out_bytes, &out)) return rc;
  if (L.n_witness) {
    const auto t_dev = std::chrono::steady_clock::now();
    vb::DeviceSession ds;
    if (int rc = pv::open_session(ds, dev, 1)) return rc;
    uint8_t* d_buf = ds.buf.alloc<uint8_t>(pv::wtnz_device_bytes(L));
    fe* d_out = ds.buf.alloc<fe>(L.n_witness);
    if (!d_buf || !d_out) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
    pv::WtnzFault f;
    if (int rc = pv::wtnz_decode_on_device(dev, ds.stream(0), L, d_buf, d_out, &f, &rep->upload_ms, &rep->kernel_ms)) return rc;
    rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;
    // the verdict is in; nothing has been written
    if (f.kind) return report_fault(rep, f);
    const auto t_down = std::chrono::steady_clock::now();
    const isnark::CopyJob job = {out + WTNS_HEAD, d_out, (size_t)L.n_witness * 32};
    DEV_TRY("device to host download", isnark::staged_copy(dev, &job, 1, false));
    rep->download_ms = pv::ms_since(t_down);
  }
  put_wtns_head(out, L);
  return 0;
}

Sink buffer_sink(void* out, size_t cap) { return pv::buffer_sink("file", out, cap); }

// a _file entry: the report zeroed before the paths are judged
int file_entry(const char* in_path, const char* out_path, Groth16WtnsPackReport* report, const std::function<int(const uint8_t*, size_t, const Sink&)>& impl)
{
  if (report) memset(report, 0, sizeof *report);
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr, impl);
}

} // namespace

// ---- host only: never initialise a GPU
ISNARK_API int groth16_wtns_packed_size(const void* wtns, size_t len, uint64_t* packed_bytes)
{
  if (!packed_bytes) return pv::fail(pv::ERR_ARG, "null output");
  *packed_bytes = 0;
  if (!wtns) return pv::fail(pv::ERR_ARG, "null wtns");
  pv::Wtns w;
  if (int rc = pv::parse_wtns((const uint8_t*)wtns, len, w)) return rc;
  std::vector<uint64_t> dir;
  if (int rc = pack_scan(w, nullptr, dir, nullptr)) return rc;
  *packed_bytes = WTNZ_HEAD + w.n_witness + 8 * dir.size() + dir.back();
  return 0;
}
ISNARK_API int groth16_wtns_pack(const void* wtns, size_t len, void* out, size_t cap, Groth16WtnsPackReport* report)
{
  return pack_impl((const uint8_t*)wtns, len, report, buffer_sink(out, cap));
}
ISNARK_API int groth16_wtns_pack_file(const char* in_path, const char* out_path, Groth16WtnsPackReport* report)
{
  return file_entry(in_path, out_path, report, [&](const uint8_t* d, size_t l, const Sink& s) { return pack_impl(d, l, report, s); });
}
ISNARK_API int groth16_wtns_unpack_host(const void* packed, size_t len, void* out, size_t cap, Groth16WtnsPackReport* report)
{
  return unpack_host_impl((const uint8_t*)packed, len, report, buffer_sink(out, cap));
}
ISNARK_API int groth16_wtns_unpack_host_file(const char* in_path, const char* out_path, Groth16WtnsPackReport* report)
{
  return file_entry(in_path, out_path, report, [&](const uint8_t* d, size_t l, const Sink& s) { return unpack_host_impl(d, l, report, s); });
}

// ---- one HIP device
ISNARK_API int groth16_wtns_unpack(const void* packed, size_t len, void* out, size_t cap, const char* device, Groth16WtnsPackReport* report)
{
  return unpack_device_impl((const uint8_t*)packed, len, device, report, buffer_sink(out, cap));
}
ISNARK_API int groth16_wtns_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16WtnsPackReport* report)
{
  return file_entry(in_path, out_path, report, [&](const uint8_t* d, size_t l, const Sink& s) { return unpack_device_impl(d, l, device, report, s); });
}
