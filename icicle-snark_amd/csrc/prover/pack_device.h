// pack_device.h — what the kernels of the packed forms share (ptau_pack.hip, wtns_pack.hip, zkey_pack.hip): the tally of a faulty
// lane and its reset, and the pieces of the block codec of a packed witness and of a packed key's coefficients (wtns_pack.h has the
// value's form) — a 256-lane workgroup per block of 256 values, a lane per value: the exclusive scan of the code lengths, the block's
// directory span, the aligned load of the span into LDS and the read of a lane's eight words out of it.  One text for each piece;
// the kernels keep their own control flow.  PackTally, NO_FAULT and POINT_FAULT are prover_internal.h's: the host reads them too.
#pragma once
#include "device_call.h"
#include "prover_internal.h"

namespace isnark {
namespace prover {

constexpr int PACK_WG = 256; // = wz::WZ_BLOCK = zp::ZP_BLOCK
// a block's payload in LDS: 8192 bytes, up to 15 in front of it (its position mod 16: the aligned load begins below the span) and the
// word behind a lane's last one (the funnel shift reads it): byte 15 + 8192 + 7 at the most
constexpr int PACK_LDS_VEC = 516;

inline size_t pad16(size_t x) { return (x + 15) & ~(size_t)15; }

// host[k] = {NO_FAULT, 0} for k < count, and their upload to d_tally enqueued on `st`: `host` lives until the stream has passed it
inline int reset_tallies(PackTally* host, PackTally* d_tally, size_t count, hipStream_t st)
{
  for (size_t k = 0; k < count; k++) host[k] = {NO_FAULT, 0};
  DEV_TRY("tally upload", hipMemcpyAsync(d_tally, host, count * sizeof(PackTally), hipMemcpyHostToDevice, st));
  return 0;
}

__device__ __forceinline__ void tally_fault(PackTally* t, uint64_t i, int kind)
{
  atomicAdd(&t->count, 1ull);
  atomicMin(&t->first, (unsigned long long)i << 3 | (unsigned long long)kind);
}

// exclusive scan of the workgroup's 256 lengths: inclusive inside each wave, the four wave sums through LDS.  EVERY lane calls it.
__device__ __forceinline__ void block_scan(uint32_t len, uint32_t* s_wave, uint32_t* off, uint32_t* total)
{
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t incl = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += y;
  }
  if (lane == 63) s_wave[wv] = incl;
  __syncthreads();
  uint32_t base = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < PACK_WG / 64; w++) {
    const uint32_t sw = s_wave[w];
    if (w < wv) base += sw;
    sum += sw;
  }
  *off = base + incl - len;
  *total = sum;
}

// Block blockIdx.x's span of the payload, [*lo, dir[block + 1]), and *head = lo mod 16.  True when the lengths' sum `total` IS the
// span — the same in every lane of the workgroup; a kernel reads or writes nothing of the payload otherwise.
__device__ __forceinline__ bool block_span(const unsigned long long* __restrict__ dir, uint32_t total, unsigned long long* lo, uint32_t* head)
{
  const unsigned long long l = dir[blockIdx.x], h = dir[blockIdx.x + 1];
  *lo = l;
  *head = (uint32_t)(l & 15);
  return (unsigned long long)total == h - l;
}

// A span that block_span has passed into s_pay[PACK_LDS_VEC], from the 16-byte boundary at or below its first byte to the one at or
// above its last: LDS byte j is payload byte lo − head + j.  `payload` is 16-byte aligned and the allocation reaches the next multiple
// of 16 behind its last byte.  The caller synchronises.
__device__ __forceinline__ void block_payload_to_lds(const uint8_t* __restrict__ payload, unsigned long long lo, uint32_t head, uint32_t total, uint4* s_pay)
{
  if (!total) return;
  const uint4* src = (const uint4*)(payload + (lo - head));
  const uint32_t nvec = (head + total + 15) >> 4; // ≤ 513
  for (uint32_t v = threadIdx.x; v < nvec; v += PACK_WG) s_pay[v] = src[v];
}

// the `len` bytes (≤ 32) at byte p of s_pay into the low words of pay, little-endian: a funnel shift of two words each, the last
// word masked.  The words above them are left as they are: the caller has zeroed pay.
__device__ __forceinline__ void lane_payload_words(const uint4* s_pay, uint32_t p, uint32_t len, uint32_t pay[8])
{
  if (!len) return;
  const uint32_t* words = (const uint32_t*)s_pay;
  const uint32_t w0 = p >> 2, sh = (p & 3) * 8;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++)
    if (4 * k < len) {
      const uint32_t a = words[w0 + k], b = words[w0 + k + 1];
      uint32_t w = sh ? (a >> sh) | (b << (32 - sh)) : a;
      const uint32_t rem = len - 4 * k;
      if (rem < 4) w &= (1u << (8 * rem)) - 1;
      pay[k] = w;
    }
}

} // namespace prover
} // namespace isnark
