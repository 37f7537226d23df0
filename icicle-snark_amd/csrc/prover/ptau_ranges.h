// ptau_ranges.h — reading a prepared .ptau's blocks on the device, shared by groth16_zkey_verify_ptau (zkey_verify.hip) and
// groth16_zkey_new (zkey_new.hip): which five ranges a circuit of domain 2^k needs, the procedure that stages them (PtauRanges:
// bound, allocate, upload, lane test where each lands), the lane tests every uploaded range goes through before anything else reads
// it and their launch (enqueue_lane_test: ptau_prepare.hip and ptau_contribute.hip send their sections through it too;
// ptau_verify.hip still launches the two kernels from a lambda of its own), and the gather of the odd elements of section 12's block k + 1 (NO_FAULT and the text of a faulting element are
// prover_internal.h's).  The kernels are in an unnamed namespace, so every translation unit that includes this compiles its own copy
// of them — include it where they are launched, nowhere else; the host procedure is one text.
#pragma once
#include "device_call.h"
#include "prover_internal.h"
#include "zkey_check29.h"

namespace {

using namespace bn254;

#if defined(__HIPCC__)
// out point i < cnt (64-byte rows) = in point 2i + 1.  One lane per 16 bytes of the output: the stores of a wave are 1 KB
// contiguous, its loads sixteen 64-byte rows at a stride of 128 bytes.
__global__ __launch_bounds__(256) void odd_gather_kernel(const uint4* __restrict__ in, uint64_t cnt, uint4* __restrict__ out)
{
  const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= 4 * cnt) return;
  out[q] = in[(q >> 2) * 8 + 4 + (q & 3)];
}

// membership of the ptau ranges that are read, zkey_check29.h's tests: min over the faulting lanes of (index << 3 | kind)
__global__ __launch_bounds__(256) void ptau_g1_kernel(const fe* __restrict__ pts, uint32_t cnt, unsigned long long* __restrict__ first)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cnt) return;
  const fe p[2] = {ld(pts + 2 * (size_t)i), ld(pts + 2 * (size_t)i + 1)};
  const int kind = p29::classify_g1(p);
  if (kind) atomicMin(first, (unsigned long long)i << 3 | (unsigned long long)kind);
}
__global__ __launch_bounds__(64) void ptau_g2_kernel(const fe2* __restrict__ pts, uint32_t cnt, unsigned long long* __restrict__ first)
{
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= cnt) return;
  const fe2 p[2] = {pts[2 * (size_t)i], pts[2 * (size_t)i + 1]};
  const int kind = p29::classify_g2(p);
  if (kind) atomicMin(first, (unsigned long long)i << 3 | (unsigned long long)kind);
}
// the lane test of n uploaded points (g2: 128-byte points, with the subgroup test) enqueued on `stream`; *d_first was set to NO_FAULT
inline int enqueue_lane_test(hipStream_t stream, bool g2, const uint8_t* d_pts, uint64_t n, unsigned long long* d_first)
{
  if (g2) DEV_LAUNCH("ptau membership kernel launch", ptau_g2_kernel, dim3((uint32_t)((n + 63) / 64)), dim3(64), stream, (const fe2*)d_pts, (uint32_t)n, d_first);
  else DEV_LAUNCH("ptau membership kernel launch", ptau_g1_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), stream, (const fe*)d_pts, (uint32_t)n, d_first);
  return 0;
}
#endif

using isnark::prover::NO_FAULT; // prover_internal.h
using isnark::prover::POINT_FAULT;

// The five ranges of a circuit with domain 2^k: block k of sections 12 [L]₁, 13 [L]₂, 14 [αL]₁, 15 [βL]₁ and block k + 1 of section
// 12.  The caller decides the streams, and downloads d_first (sizeof first[N]) at a synchronisation point of its own — behind both
// streams — before it asks for the verdict.
struct PtauRanges {
  enum { N = 5 };
  static int section(int i) { return i == 4 ? 12 : 12 + i; }
  uint32_t power(int i) const { return i == 4 ? k + 1 : k; }

  uint32_t k = 0;
  uint8_t* d_blk[N] = {};
  unsigned long long* d_first = nullptr; // [i]: min over range i's faulting lanes of (element << 3 | kind), NO_FAULT without one

  // d_first on the device, cleared on `stream`.  Apart from stage(): a caller whose second stream waits for its first by an event
  // records that event after this.
  int reset(isnark::vb::DeviceSession& session, hipStream_t stream);
  // every range: bounded by ptau_block, allocated in the session, uploaded (it has landed on return, its time added to *upload_ms)
  // and sent through its lane test — the G1 ranges on stream_g1, the G2 range on stream_g2
  int stage(const isnark::prover::PtauLayout& PL, uint32_t log_n, isnark::vb::DeviceSession& session, int dev, hipStream_t stream_g1, hipStream_t stream_g2, double* upload_ms);
  const uint8_t* l1() const { return d_blk[0]; }       // [L_j]₁, j < 2^k
  const uint8_t* l2() const { return d_blk[1]; }       // [L_j]₂
  const uint8_t* alpha_l1() const { return d_blk[2]; } // [α·L_j]₁
  const uint8_t* beta_l1() const { return d_blk[3]; }  // [β·L_j]₁
  const uint8_t* next() const { return d_blk[4]; }     // [L'_j]₁, j < 2^(k+1): block k + 1
  // out[i] = [L'_{2i+1}]₁, i < n (64-byte rows)
  int gather_odd(hipStream_t stream, uint64_t n, uint8_t* out) const;
  // 0 when no lane faulted, else ERR_FORMAT naming the first range at fault and its lowest faulting element
  int verdict(const unsigned long long first[N]) const
  {
    for (int i = 0; i < N; i++)
      if (first[i] != NO_FAULT)
        return isnark::prover::fail(isnark::prover::ERR_FORMAT, "ptau: section %d, block %u, element %llu: %s", section(i), power(i), (unsigned long long)(first[i] >> 3),
                                    POINT_FAULT[first[i] & 3]);
    return 0;
  }
};

#if defined(__HIPCC__)
inline int PtauRanges::reset(isnark::vb::DeviceSession& session, hipStream_t stream)
{
  d_first = session.buf.alloc<unsigned long long>(N);
  if (!d_first) return isnark::prover::dev_fail("hipMalloc", hipErrorOutOfMemory);
  DEV_TRY("hipMemset", hipMemsetAsync(d_first, 0xff, N * sizeof *d_first, stream));
  return 0;
}
inline int PtauRanges::stage(const isnark::prover::PtauLayout& PL, uint32_t log_n, isnark::vb::DeviceSession& session, int dev, hipStream_t stream_g1, hipStream_t stream_g2,
                             double* upload_ms)
{
  k = log_n;
  for (int i = 0; i < N; i++) {
    const size_t elem = section(i) == 13 ? 128 : 64;
    const uint64_t cnt = (uint64_t)1 << power(i);
    const uint8_t* src;
    if (int rc = isnark::prover::ptau_block(PL, section(i), power(i), elem, &src)) return rc;
    d_blk[i] = session.buf.alloc<uint8_t>((size_t)(cnt * elem));
    if (!d_blk[i]) return isnark::prover::dev_fail("hipMalloc", hipErrorOutOfMemory);
    if (int rc = isnark::prover::timed_upload(dev, d_blk[i], src, (size_t)(cnt * elem), upload_ms)) return rc;
    if (int rc = enqueue_lane_test(elem == 64 ? stream_g1 : stream_g2, elem == 128, d_blk[i], cnt, d_first + i)) return rc;
  }
  return 0;
}
inline int PtauRanges::gather_odd(hipStream_t stream, uint64_t n, uint8_t* out) const
{
  DEV_LAUNCH("gather kernel launch", odd_gather_kernel, dim3((uint32_t)((4 * n + 255) / 256)), dim3(256), stream, (const uint4*)d_blk[4], n, (uint4*)out);
  return 0;
}
#endif

} // namespace
