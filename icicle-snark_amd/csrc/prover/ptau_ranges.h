// ptau_ranges.h — the device side of reading a prepared .ptau's blocks, shared by groth16_zkey_verify_ptau (zkey_verify.hip) and
// groth16_zkey_new (zkey_new.hip): the lane tests every uploaded range goes through before anything else reads it, and the gather
// of the odd elements of section 12's block k + 1.  Each including translation unit gets its own copy of the kernels.
#pragma once
#include "prover_internal.h"
#include "zkey_check29.h"

namespace {

using namespace bn254;

__device__ __forceinline__ fe ld(const fe* p)
{
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  fe v;
  v.l[0] = lo.x, v.l[1] = lo.y, v.l[2] = lo.z, v.l[3] = lo.w;
  v.l[4] = hi.x, v.l[5] = hi.y, v.l[6] = hi.z, v.l[7] = hi.w;
  return v;
}

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

constexpr unsigned long long NO_FAULT = ~0ull;
const char* const POINT_FAULT[4] = {"", "a coordinate is not below q", "the point is not on the curve", "the point is outside the subgroup"};

} // namespace
