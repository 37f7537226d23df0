// zkey_pack.hip — groth16_zkey_pack / groth16_zkey_unpack: a proving key with every point as x and one bit of y and every
// coefficient as a code byte and its significant bytes ("zkez"), and back; groth16_zkey_coefs_pack / _unpack: the coefficient codec
// over a plain buffer of records; and the decode the packed load (cache.cpp: ingest_packed) puts in front of its unchanged device
// work.  include/groth16_prover.h has the contract and the container; zkey_pack29.h the coefficient's form and its lane code;
// point_pack29.h the packed point; containers.cpp the reader (zkez_layout); pack_device.h the block codec's pieces, which
// wz_unpack_kernel shares; DESIGN.md §7l.
//
//   host, first  the container — a .zkey through zkey_layout(need_ic) for pack, a packed key through zkez_layout for unpack: every
//                point section is tied to its element count, section 4 to the sum of its parts and the whole directory is bounded
//                before a byte goes up.
//   device       points: ONE launch per section through ptau_pack.hip's enqueue_point_ranges (pack_on_device / unpack_on_device).
//                coefficients, pack: kernel 1 (a 256-lane workgroup per block of 256 records, a lane per record) tests the value
//                below r, takes it through from_mont twice, writes the code, copies the triple and writes the block's length sum;
//                the HOST turns the sums into the directory; kernel 2 derives the value again, scans the block's lengths (wave
//                scans, four wave sums through LDS), stages the block's payload in LDS at its position mod 16 and stores whole
//                16-byte vectors in the block's interior only — the bytes in front of the first and behind the last 16-byte
//                boundary, which a neighbouring block's payload shares a vector with, go out as single bytes.
//                coefficients, unpack: ONE kernel with wz_unpack_kernel's structure — the length scan, the block sum against the
//                directory span BEFORE any payload byte is read, the payload into LDS in aligned 16-byte loads — then
//                wz_decode_value, to_mont twice, the block's 44-byte records assembled in LDS (256 · 44 = 11264 bytes, a multiple
//                of 16: block b begins at a 16-byte boundary) and stored as 16-byte vectors.  A faulty lane writes a zero record
//                and tallies: the lowest (element << 3 | kind) and a count.
//   host, last   ALL verdicts are read before anything is written.  Then the container — the other magic, the sections in the
//                input's order, sections 1, 2, 10 and any unknown one byte for byte — and the sections come down into their places.
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "device_call.h"
#include "pack_device.h"
#include "prover_internal.h"
#include "verify_batch.h"
#include "zkey_pack29.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;
namespace vb = isnark::vb;
typedef pv::PackTally Tally;
using pv::block_scan; // pack_device.h: the block codec's pieces
using pv::NO_FAULT;
using pv::pad16;
using pv::tally_fault;

constexpr int ZP_WG = (int)zp::ZP_BLOCK;
static_assert(ZP_WG == pv::PACK_WG, "pack_device.h's block codec is a 256-lane workgroup's");
constexpr int ZP_REC_VEC = (int)(zp::ZP_BLOCK_BYTES / 16); // 704

// record i of `rec` (11 words each): its value through zp_encode.  The payload's length, 0 for a value not below r (*bad set).
__device__ __forceinline__ uint32_t encode_record(const uint32_t* __restrict__ rec, uint64_t i, uint8_t* code, uint32_t pay[8], bool* bad)
{
  const uint32_t* e = rec + i * zp::ZP_RECORD_WORDS;
  fe f;
#pragma unroll
  for (int k = 0; k < 8; k++) f.l[k] = e[3 + k];
  const int len = zp::zp_encode(f, code, pay);
  *bad = len < 0;
  if (len < 0) *code = wz::WZ_CODE_ZERO;
  return len > 0 ? (uint32_t)len : 0;
}

// pack, kernel 1.  Block blockIdx.x of n records: codes[i], triples[3i … 3i + 2], sums[block] = the block's payload bytes.
__global__ __launch_bounds__(ZP_WG) void zp_scan_kernel(const uint32_t* __restrict__ rec, uint32_t n, uint8_t* __restrict__ codes, uint32_t* __restrict__ triples,
                                                        uint32_t* __restrict__ sums, Tally* __restrict__ tally)
{
  __shared__ uint32_t s_wave[ZP_WG / 64];
  const uint64_t i = (uint64_t)blockIdx.x * ZP_WG + threadIdx.x;
  uint32_t len = 0;
  if (i < n) {
    uint8_t code;
    uint32_t pay[8];
    bool bad;
    len = encode_record(rec, i, &code, pay, &bad);
    if (bad) tally_fault(tally, i, wz::WZ_RANGE);
    codes[i] = code;
#pragma unroll
    for (int k = 0; k < 3; k++) triples[3 * i + k] = rec[i * zp::ZP_RECORD_WORDS + k];
  }
  uint32_t off, total;
  block_scan(len, s_wave, &off, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// pack, kernel 2.  Block blockIdx.x: its lanes' significant bytes to payload[dir[block] …).  `payload` is 16-byte aligned.  A
// vector store never covers a byte outside [dir[block], dir[block + 1]): the neighbours' payloads abut at any byte.
__global__ __launch_bounds__(ZP_WG) void zp_emit_kernel(const uint32_t* __restrict__ rec, uint32_t n, const unsigned long long* __restrict__ dir, uint8_t* __restrict__ payload)
{
  __shared__ uint4 s_pay[pv::PACK_LDS_VEC];
  __shared__ uint32_t s_wave[ZP_WG / 64];
  const uint32_t t = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * ZP_WG + t;
  uint32_t len = 0, pay[8];
  if (i < n) {
    uint8_t code;
    bool bad;
    len = encode_record(rec, i, &code, pay, &bad);
  }
  uint32_t off, total;
  block_scan(len, s_wave, &off, &total);
  unsigned long long lo;
  uint32_t head;
  if (!pv::block_span(dir, total, &lo, &head) || !total) return; // (the host made the directory from kernel 1's sums: they agree)
  uint8_t* const s_bytes = (uint8_t*)s_pay;
  if (len) {
    const uint32_t p = head + off;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++)
#pragma unroll
      for (uint32_t b = 0; b < 4; b++)
        if (4 * k + b < len) s_bytes[p + 4 * k + b] = (uint8_t)(pay[k] >> (8 * b));
  }
  __syncthreads();
  // LDS byte j is payload byte lo − head + j, and lo − head is a multiple of 16
  uint8_t* const g = payload + (lo - head);
  const uint32_t end = head + total, a0 = head ? 16u : 0u, a1 = end & ~15u; // whole vectors: [a0, a1)
  if (a0 < a1)
    for (uint32_t v = (a0 >> 4) + t; v < (a1 >> 4); v += ZP_WG) ((uint4*)g)[v] = s_pay[v];
  const uint32_t h1 = a0 < end ? a0 : end, t0 = h1 > a1 ? h1 : a1; // single bytes: [head, h1) and [t0, end), fewer than 16 each
  if (t < 16) {
    if (head + t < h1) g[head + t] = s_bytes[head + t];
    if (t0 + t < end) g[t0 + t] = s_bytes[t0 + t];
  }
}

// unpack.  Block blockIdx.x of a packed section 4 → records 256·b … 256·b + 255 in the file's form at out (16-byte aligned).
// `payload` is 16-byte aligned and the allocation reaches the next multiple of 16 behind its last byte; `dir` has passed
// wz_check_directory.
__global__ __launch_bounds__(ZP_WG) void zp_unpack_kernel(const uint8_t* __restrict__ codes, const uint32_t* __restrict__ triples, const unsigned long long* __restrict__ dir,
                                                          const uint8_t* __restrict__ payload, uint32_t n, uint32_t* __restrict__ out, Tally* __restrict__ tally)
{
  __shared__ uint4 s_pay[pv::PACK_LDS_VEC];
  __shared__ uint4 s_rec[ZP_REC_VEC];
  __shared__ uint32_t s_wave[ZP_WG / 64];
  const uint32_t t = threadIdx.x;
  const uint64_t first = (uint64_t)blockIdx.x * ZP_WG, i = first + t;
  const bool live = i < n;
  const uint8_t code = live ? codes[i] : wz::WZ_CODE_ZERO;
  const int cl = wz::wz_code_len(code);
  const uint32_t len = cl > 0 ? (uint32_t)cl : 0;
  uint32_t off, total;
  block_scan(len, s_wave, &off, &total);

  unsigned long long lo;
  uint32_t head;
  const bool dir_ok = pv::block_span(dir, total, &lo, &head);
  if (!dir_ok && t == 0) tally_fault(tally, i, wz::WZ_DIRECTORY);
  // nothing of the payload is read when the lengths do not sum to the span
  if (dir_ok) pv::block_payload_to_lds(payload, lo, head, total, s_pay);
  __syncthreads();
  uint32_t* const s_words = (uint32_t*)s_rec;
  if (live) {
    uint32_t pay[8] = {};
    if (dir_ok) pv::lane_payload_words(s_pay, head + off, len, pay);
    fe f;
#pragma unroll
    for (int k = 0; k < 8; k++) f.l[k] = 0;
    int kind = wz::WZ_DIRECTORY; // (tallied above, once for the block)
    if (dir_ok) {
      kind = zp::zp_decode(code, pay, &f);
      if (kind) tally_fault(tally, i, kind);
    }
    // the record in LDS: 11 words a lane, an odd stride
#pragma unroll
    for (int k = 0; k < 3; k++) s_words[t * zp::ZP_RECORD_WORDS + k] = kind ? 0u : triples[3 * i + k];
#pragma unroll
    for (int k = 0; k < 8; k++) s_words[t * zp::ZP_RECORD_WORDS + 3 + k] = f.l[k];
  }
  __syncthreads();
  // the block's records begin at byte 11264·b: whole vectors, and the last block's odd words one by one
  const uint32_t n_live = n - first < (uint64_t)ZP_WG ? (uint32_t)(n - first) : (uint32_t)ZP_WG, n_words = n_live * zp::ZP_RECORD_WORDS;
  uint32_t* const g = out + first * zp::ZP_RECORD_WORDS;
  for (uint32_t v = t; v < (n_words >> 2); v += ZP_WG) ((uint4*)g)[v] = s_rec[v];
  if (t < (n_words & 3)) g[(n_words & ~3u) + t] = s_words[(n_words & ~3u) + t];
}

struct DeviceLayout { // of zkez_coefs_decode's d_buf
  size_t dir = 0, triples, codes, payload, total;
  explicit DeviceLayout(const pv::ZkezCoefs& C)
  {
    triples = dir + pad16((size_t)(C.n_blocks + 1) * 8);
    codes = triples + pad16((size_t)C.n_coef * 12);
    payload = codes + pad16(C.n_coef);
    total = payload + pad16((size_t)C.payload_bytes) + 16;
  }
};

} // namespace

namespace isnark {
namespace prover {

size_t zkez_coefs_device_bytes(const ZkezCoefs& C) { return DeviceLayout(C).total; }

void zkez_coefs_jobs(const ZkezCoefs& C, uint8_t* d_buf, std::vector<UploadJob>& jobs)
{
  const DeviceLayout D(C);
  jobs.push_back({d_buf + D.dir, C.dir, (size_t)(C.n_blocks + 1) * 8});
  if (C.n_coef) jobs.push_back({d_buf + D.triples, C.triples, (size_t)C.n_coef * 12});
  if (C.n_coef) jobs.push_back({d_buf + D.codes, C.codes, (size_t)C.n_coef});
  if (C.payload_bytes) jobs.push_back({d_buf + D.payload, C.payload, (size_t)C.payload_bytes});
}

int zkez_coefs_decode(hipStream_t st, const ZkezCoefs& C, uint8_t* d_buf, uint32_t* d_records, PackTally* d_tally)
{
  if (!C.n_coef) return 0;
  const DeviceLayout D(C);
  // the padding behind the payload: what an aligned over-read sees is zero
  DEV_TRY("hipMemsetAsync", hipMemsetAsync(d_buf + D.payload + C.payload_bytes, 0, D.total - D.payload - (size_t)C.payload_bytes, st));
  DEV_LAUNCH("coefficient unpack kernel launch", zp_unpack_kernel, dim3((uint32_t)C.n_blocks), dim3(ZP_WG), st, (const uint8_t*)(d_buf + D.codes), (const uint32_t*)(d_buf + D.triples),
             (const unsigned long long*)(d_buf + D.dir), (const uint8_t*)(d_buf + D.payload), C.n_coef, d_records, d_tally);
  return 0;
}

int packed_point_fail(const char* form, int section, const PackTally& t)
{
  return fail(ERR_FORMAT, "%s: section %d, element %llu: %s", form, section, (unsigned long long)(t.first >> 3), POINT_FAULT[t.first & 3]);
}
int packed_coef_fail(const char* form, const PackTally& t)
{
  const int kind = (int)(t.first & 7);
  if (kind == wz::WZ_RANGE && strcmp(form, "zkey") == 0) return fail(ERR_FORMAT, "zkey: coefficient %llu: not below r", (unsigned long long)(t.first >> 3));
  return fail(ERR_FORMAT, "%s: coefficient %llu: %s", form, (unsigned long long)(t.first >> 3), wz::wz_fault_text(kind));
}

} // namespace prover
} // namespace isnark

namespace {

using pv::parse_device;
using pv::reset_tallies;
using pv::Sink;

// ---- the coefficients of a pack, on their way through the two kernels
struct CoefPack {
  uint32_t n = 0;
  uint64_t n_blocks = 0;
  uint32_t *d_records = nullptr, *d_triples = nullptr, *d_sums = nullptr;
  uint8_t *d_codes = nullptr, *d_payload = nullptr;
  unsigned long long* d_dir = nullptr;
  std::vector<uint32_t> sums;
  std::vector<uint64_t> dir; // n_blocks + 1, after make_directory
  uint64_t payload_bytes() const { return dir.back(); }
};
// the records up, kernel 1, the block sums on their way down: complete once `st` has been synchronised
int coef_pack_scan(vb::DeviceSession& ds, int dev, hipStream_t st, const uint8_t* records, uint32_t n, CoefPack& cp, Tally* d_tally, double* upload_ms)
{
  cp.n = n;
  cp.n_blocks = ((uint64_t)n + zp::ZP_BLOCK - 1) / zp::ZP_BLOCK;
  cp.sums.assign((size_t)cp.n_blocks, 0);
  if (!n) return 0;
  cp.d_records = ds.buf.alloc<uint32_t>((size_t)n * zp::ZP_RECORD_WORDS);
  cp.d_triples = ds.buf.alloc<uint32_t>((size_t)n * 3);
  cp.d_codes = ds.buf.alloc<uint8_t>(n);
  cp.d_sums = ds.buf.alloc<uint32_t>((size_t)cp.n_blocks);
  cp.d_dir = ds.buf.alloc<unsigned long long>((size_t)cp.n_blocks + 1);
  if (!cp.d_records || !cp.d_triples || !cp.d_codes || !cp.d_sums || !cp.d_dir) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  if (int rc = pv::timed_upload(dev, cp.d_records, records, (size_t)n * zp::ZP_RECORD_BYTES, upload_ms)) return rc;
  DEV_LAUNCH("coefficient scan kernel launch", zp_scan_kernel, dim3((uint32_t)cp.n_blocks), dim3(ZP_WG), st, (const uint32_t*)cp.d_records, n, cp.d_codes, cp.d_triples, cp.d_sums, d_tally);
  DEV_TRY("download", hipMemcpyAsync(cp.sums.data(), cp.d_sums, cp.sums.size() * 4, hipMemcpyDeviceToHost, st));
  return 0;
}
void make_directory(CoefPack& cp)
{
  cp.dir.assign((size_t)cp.n_blocks + 1, 0);
  for (size_t b = 0; b < cp.sums.size(); b++) cp.dir[b + 1] = cp.dir[b] + cp.sums[b];
}
// the directory up, kernel 2: the payload is complete on return
int coef_pack_emit(vb::DeviceSession& ds, hipStream_t st, CoefPack& cp)
{
  if (!cp.n || !cp.payload_bytes()) return 0;
  cp.d_payload = ds.buf.alloc<uint8_t>(pad16((size_t)cp.payload_bytes()));
  if (!cp.d_payload) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  DEV_TRY("directory upload", hipMemcpyAsync(cp.d_dir, cp.dir.data(), cp.dir.size() * 8, hipMemcpyHostToDevice, st));
  DEV_LAUNCH("coefficient emit kernel launch", zp_emit_kernel, dim3((uint32_t)cp.n_blocks), dim3(ZP_WG), st, (const uint32_t*)cp.d_records, cp.n, (const unsigned long long*)cp.d_dir, cp.d_payload);
  DEV_TRY("coefficient emit kernel", hipStreamSynchronize(st));
  return 0;
}
// the body's counts and directory at w; its triples, codes and payload as downloads into their places
void coef_pack_body(const CoefPack& cp, uint32_t declared, uint8_t* w, std::vector<isnark::CopyJob>& down)
{
  const uint64_t payload = cp.payload_bytes();
  memcpy(w, &declared, 4);
  memcpy(w + 4, &cp.n, 4);
  memcpy(w + 8, &payload, 8);
  uint8_t* const triples = w + pv::ZKEZ_COEFS_HEAD;
  uint8_t* const codes = triples + 12 * (size_t)cp.n;
  uint8_t* const dir = codes + cp.n;
  memcpy(dir, cp.dir.data(), cp.dir.size() * 8);
  if (cp.n) down.push_back({triples, cp.d_triples, 12 * (size_t)cp.n});
  if (cp.n) down.push_back({codes, cp.d_codes, (size_t)cp.n});
  if (payload) down.push_back({dir + cp.dir.size() * 8, cp.d_payload, (size_t)payload});
}

// ---- groth16_zkey_coefs_pack / groth16_zkey_coefs_unpack
int coefs_fault(Groth16ZkeyCoefsReport* rep, const char* form, const Tally& t)
{
  rep->fault_kind = (int32_t)(t.first & 7), rep->fault_index = t.first >> 3, rep->fault_count = t.count;
  return pv::packed_coef_fail(form, t);
}

int coefs_pack_impl(const void* records, uint64_t n, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  rep->n = n;
  rep->in_bytes = n * zp::ZP_RECORD_BYTES;
  int dev;
  if (int rc = parse_device(device, &dev)) return rc;
  if (n && !records) return pv::fail(pv::ERR_ARG, "null buffer");
  if (n > 0xffffffffull) return pv::fail(pv::ERR_ARG, "coefficients: %llu records in one call, 2^32 - 1 is the most", (unsigned long long)n);
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  Tally* const d_tally = ds.buf.alloc<Tally>(1);
  if (!d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  Tally t;
  if (int rc = reset_tallies(&t, d_tally, 1, st)) return rc;
  CoefPack cp;
  if (int rc = coef_pack_scan(ds, dev, st, (const uint8_t*)records, (uint32_t)n, cp, d_tally, &rep->upload_ms)) return rc;
  DEV_TRY("download", hipMemcpyAsync(&t, d_tally, sizeof t, hipMemcpyDeviceToHost, st));
  DEV_TRY("coefficient scan kernel", hipStreamSynchronize(st));
  if (t.first != NO_FAULT) return coefs_fault(rep, "zkey", t);
  make_directory(cp);
  rep->out_bytes = pv::zkez_coefs_bytes(n, cp.payload_bytes());
  uint8_t* w = nullptr;
  if (int rc = pv::buffer_sink("output", out, cap)(rep->out_bytes, &w)) return rc;
  if (int rc = coef_pack_emit(ds, st, cp)) return rc;
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;
  const auto t_down = std::chrono::steady_clock::now();
  std::vector<isnark::CopyJob> down;
  coef_pack_body(cp, (uint32_t)n, w, down);
  if (!down.empty()) DEV_TRY("device to host download", isnark::staged_copy(dev, down.data(), down.size(), false));
  rep->download_ms = pv::ms_since(t_down);
  return 0;
}

int coefs_unpack_impl(const void* body, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = parse_device(device, &dev)) return rc;
  if (!body) return pv::fail(pv::ERR_ARG, "null buffer");
  pv::ZkezCoefs C;
  if (int rc = pv::zkez_coefs_layout((const uint8_t*)body, len, &C)) return rc;
  rep->n = C.n_coef;
  rep->in_bytes = len;
  rep->out_bytes = (uint64_t)C.n_coef * zp::ZP_RECORD_BYTES;
  uint8_t* w = nullptr;
  if (C.n_coef)
    if (int rc = pv::buffer_sink("output", out, cap)(rep->out_bytes, &w)) return rc;
  if (!C.n_coef) return 0;
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  Tally* const d_tally = ds.buf.alloc<Tally>(1);
  uint8_t* const d_buf = ds.buf.alloc<uint8_t>(pv::zkez_coefs_device_bytes(C));
  uint32_t* const d_records = ds.buf.alloc<uint32_t>((size_t)C.n_coef * zp::ZP_RECORD_WORDS);
  if (!d_tally || !d_buf || !d_records) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  Tally t;
  if (int rc = reset_tallies(&t, d_tally, 1, st)) return rc;
  std::vector<pv::UploadJob> jobs;
  pv::zkez_coefs_jobs(C, d_buf, jobs);
  const auto t_up = std::chrono::steady_clock::now();
  DEV_TRY("host to device upload", isnark::staged_copy(dev, jobs.data(), jobs.size(), true));
  rep->upload_ms = pv::ms_since(t_up);
  if (int rc = pv::zkez_coefs_decode(st, C, d_buf, d_records, d_tally)) return rc;
  DEV_TRY("download", hipMemcpyAsync(&t, d_tally, sizeof t, hipMemcpyDeviceToHost, st));
  DEV_TRY("coefficient unpack kernel", hipStreamSynchronize(st));
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;
  // the verdict is in; nothing has been written
  if (t.first != NO_FAULT) return coefs_fault(rep, "zkez", t);
  const auto t_down = std::chrono::steady_clock::now();
  const isnark::CopyJob job = {w, d_records, (size_t)rep->out_bytes};
  DEV_TRY("device to host download", isnark::staged_copy(dev, &job, 1, false));
  rep->download_ms = pv::ms_since(t_down);
  return 0;
}

// ---- groth16_zkey_pack / groth16_zkey_unpack
constexpr int POINT_SECTIONS[6] = {3, 5, 6, 7, 8, 9};
constexpr int COEF_TALLY = 6; // the tallies: one per point section, then section 4's
bool is_point_section(uint32_t id) { return id == 3 || (id >= 5 && id <= 9); }

int file_fault(Groth16ZkeyPackReport* rep, const char* form, int section, const Tally& t)
{
  rep->fault_section = section, rep->fault_kind = (int32_t)(t.first & 7), rep->fault_index = t.first >> 3, rep->fault_count = t.count;
  return section == 4 ? pv::packed_coef_fail(form, t) : pv::packed_point_fail(form, section, t);
}
// the lowest faulty section, then its lowest faulty element
int first_fault(Groth16ZkeyPackReport* rep, const char* form, const Tally* tallies)
{
  for (int id = 3; id <= 9; id++) {
    int k = COEF_TALLY;
    for (int j = 0; j < 6; j++)
      if (POINT_SECTIONS[j] == id) k = j;
    if (tallies[k].first != NO_FAULT) return file_fault(rep, form, id, tallies[k]);
  }
  return 0;
}

int file_impl(bool unpack, const uint8_t* data, size_t len, const char* device, Groth16ZkeyPackReport* rep, const Sink& sink)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  int dev;
  if (int rc = parse_device(device, &dev)) return rc;
  std::vector<pv::Section> secs;
  pv::ZkeyLayout L;
  pv::PackedZkey P;
  if (int rc = unpack ? pv::zkez_layout(data, len, secs, &L, &P) : pv::zkey_layout(data, len, secs, &L, /*need_ic=*/true)) return rc;
  rep->n_vars = L.n_vars, rep->n_public = L.n_public, rep->domain = L.domain, rep->n_coef = L.n_coef;
  rep->in_bytes = len;
  const char* const form = unpack ? "zkez" : "zkey";
  pv::PointRange ranges[6];
  uint64_t packed_points = 0;
  for (int k = 0; k < 6; k++) {
    const int id = POINT_SECTIONS[k];
    const bool g2 = id == 7;
    const size_t in_elem = (unpack ? 32u : 64u) * (g2 ? 2u : 1u);
    ranges[k] = {id, g2, L.sec[id]->size / in_elem, L.sec[id]->p, nullptr, nullptr, nullptr};
    rep->points[g2] += ranges[k].n;
    packed_points += ranges[k].n * (g2 ? 64 : 32);
  }
  rep->point_bytes = packed_points;
  uint8_t* out = nullptr;
  if (unpack) {
    rep->coef_bytes = L.sec[4]->size;
    rep->out_bytes = P.unpacked_bytes;
    if (int rc = sink(rep->out_bytes, &out)) return rc;
  }

  pv::StageTrace trace(unpack ? "zkey-unpack" : "zkey-pack", "ICICLE_SNARK_TRACE_ZKEY_PACK");
  trace.lap("layout");
  const auto t_dev = std::chrono::steady_clock::now();
  vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 1)) return rc;
  const hipStream_t st = ds.stream(0);
  Tally tallies[COEF_TALLY + 1];
  Tally* const d_tally = ds.buf.alloc<Tally>(COEF_TALLY + 1);
  if (!d_tally) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  if (int rc = reset_tallies(tallies, d_tally, COEF_TALLY + 1, st)) return rc;
  // the point sections: up, one launch each
  if (int rc = pv::enqueue_point_ranges(ds, dev, unpack, ranges, 6, d_tally, &rep->upload_ms)) return rc;
  // section 4
  CoefPack cp;
  uint32_t* d_records = nullptr;
  if (unpack) {
    if (L.n_coef) {
      uint8_t* const d_buf = ds.buf.alloc<uint8_t>(pv::zkez_coefs_device_bytes(P.coefs));
      d_records = ds.buf.alloc<uint32_t>((size_t)L.n_coef * zp::ZP_RECORD_WORDS);
      if (!d_buf || !d_records) return pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
      std::vector<pv::UploadJob> jobs;
      pv::zkez_coefs_jobs(P.coefs, d_buf, jobs);
      const auto t_up = std::chrono::steady_clock::now();
      DEV_TRY("host to device upload", isnark::staged_copy(dev, jobs.data(), jobs.size(), true));
      rep->upload_ms += pv::ms_since(t_up);
      if (int rc = pv::zkez_coefs_decode(st, P.coefs, d_buf, d_records, d_tally + COEF_TALLY)) return rc;
    }
  } else if (int rc = coef_pack_scan(ds, dev, st, L.records(), L.n_coef, cp, d_tally + COEF_TALLY, &rep->upload_ms))
    return rc;
  DEV_TRY("download", hipMemcpyAsync(tallies, d_tally, sizeof tallies, hipMemcpyDeviceToHost, st));
  DEV_TRY("pack kernels", hipStreamSynchronize(st));
  trace.lap("sections up, kernels");
  // every verdict is in; nothing has been written
  if (int rc = first_fault(rep, form, tallies)) return rc;
  if (!unpack) {
    // the packed size is known now: the room is tested before the payload is made
    make_directory(cp);
    rep->coef_bytes = pv::zkez_coefs_bytes(L.n_coef, cp.payload_bytes());
    uint64_t total = 12;
    for (const pv::SectionEntry& e : pv::sections_in_order(data)) total += 12 + (e.id == 4 ? rep->coef_bytes : is_point_section(e.id) ? e.size / 2 : e.size);
    rep->out_bytes = total;
    if (int rc = sink(total, &out)) return rc;
    if (int rc = coef_pack_emit(ds, st, cp)) return rc;
    trace.lap("directory, payload");
  }
  rep->device_ms = pv::ms_since(t_dev) - rep->upload_ms;

  // ---- the container: the other magic, the sections in the input's order
  std::vector<isnark::CopyJob> down;
  uint8_t* w = out;
  const std::vector<pv::SectionEntry> order = pv::sections_in_order(data);
  pv::put_container_head(w, unpack ? "zkey" : "zkez", 1, (uint32_t)order.size());
  for (const pv::SectionEntry& e : order) {
    const bool point = is_point_section(e.id);
    const uint64_t size = e.id == 4 ? (unpack ? 4 + (uint64_t)L.n_coef * zp::ZP_RECORD_BYTES : rep->coef_bytes) : !point ? e.size : unpack ? 2 * e.size : e.size / 2;
    pv::put_section(w, e.id, size);
    if (e.id == 4 && unpack) {
      memcpy(w, &P.coefs.declared, 4);
      if (L.n_coef) down.push_back({w + 4, d_records, (size_t)L.n_coef * zp::ZP_RECORD_BYTES});
    } else if (e.id == 4) {
      uint32_t declared;
      memcpy(&declared, e.p, 4);
      coef_pack_body(cp, declared, w, down);
    } else if (!point) {
      memcpy(w, e.p, (size_t)e.size);
    } else {
      for (pv::PointRange& r : ranges)
        if (r.section == (int)e.id && r.n) down.push_back({w, r.d_out, (size_t)size});
    }
    w += size;
  }
  trace.lap("container, copied sections");
  const auto t_down = std::chrono::steady_clock::now();
  if (!down.empty()) DEV_TRY("device to host download", isnark::staged_copy(dev, down.data(), down.size(), false));
  rep->download_ms = pv::ms_since(t_down);
  trace.lap("sections downloaded");
  return 0;
}

// a _file entry: the report zeroed before the paths are judged
int file_entry(bool unpack, const char* in_path, const char* out_path, const char* device, Groth16ZkeyPackReport* report)
{
  if (report) memset(report, 0, sizeof *report);
  return pv::rewrite_file(in_path, out_path, report ? &report->write_ms : nullptr,
                          [&](const uint8_t* data, size_t len, const Sink& sink) { return file_impl(unpack, data, len, device, report, sink); });
}

} // namespace

ISNARK_API int groth16_zkey_coefs_pack(const void* records, uint64_t n, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* report)
{
  return coefs_pack_impl(records, n, out, cap, device, report);
}
ISNARK_API int groth16_zkey_coefs_unpack(const void* body, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyCoefsReport* report)
{
  return coefs_unpack_impl(body, len, out, cap, device, report);
}
ISNARK_API int groth16_zkey_pack(const void* zkey, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyPackReport* report)
{
  return file_impl(false, (const uint8_t*)zkey, len, device, report, pv::buffer_sink("output", out, cap));
}
ISNARK_API int groth16_zkey_unpack(const void* zkez, size_t len, void* out, size_t cap, const char* device, Groth16ZkeyPackReport* report)
{
  return file_impl(true, (const uint8_t*)zkez, len, device, report, pv::buffer_sink("output", out, cap));
}
ISNARK_API int groth16_zkey_pack_file(const char* in_path, const char* out_path, const char* device, Groth16ZkeyPackReport* report)
{
  return file_entry(false, in_path, out_path, device, report);
}
ISNARK_API int groth16_zkey_unpack_file(const char* in_path, const char* out_path, const char* device, Groth16ZkeyPackReport* report)
{
  return file_entry(true, in_path, out_path, device, report);
}
