// shard_ranges.h — which part of a key's five base arrays shard `rank` of `count` holds (build_cache, cache.cpp).
// Host only: plain integers in, plain integers out — no device, no ZKeyCache (tests/shard_ranges_check.cpp prints a grid of them).
#pragma once
#include <stdint.h>

namespace isnark {
namespace prover {

// elements per rank when the witness is uploaded in shard_count slices
inline uint64_t witness_slice_elems(uint32_t n_vars, int count) { return ((uint64_t)n_vars + count - 1) / count; }

struct ShardRanges {
  uint32_t wlo, whi; // A, B1, B2: the witness range [wlo, whi) of [0, n_vars)
  uint32_t clo, chi; // C (= witness[n_public + 1 ..]): the part of that SAME witness range it covers, in C's own indices
  uint32_t hlo, hhi; // H: [hlo, hhi) of [0, domain) — or, strided, the h_count = hhi elements h_first + k·h_stride (hlo = 0)
  uint32_t h_stride, h_first;
  bool slice_aligned, h_strided;
};

// A, B1, B2 share the witness range [wlo, whi); C takes the part of that same range it covers, so that one digit sort of
// witness[wlo:whi] serves all four MSMs.
// The range of shard `rank` is the witness SLICE that rank uploads itself (witness_slice_elems: ⌈n_vars / count⌉ wires from
// rank·slice; groth16_upload_witness_slice, multi.cpp) whenever that leaves no shard empty: its digit sort and its four witness
// accumulations then need nothing from the other devices and run while the in-place all-gather, the distributed front end and its
// two all-to-alls are still under way (prover.cpp: own_slice_first).  Otherwise the even split ⌊n_vars·rank / count⌋.
// H: a power-of-two shard count takes the residue class k ≡ rank (mod count) instead of a contiguous range — the rank then needs
// the coset evaluations only at those k, which the folded forward transform delivers at 1/count of the cost (qap.h: qap_coset_fold3).
inline ShardRanges shard_ranges(uint32_t n_vars, uint32_t n_public, uint32_t domain, int rank, int count)
{
  ShardRanges r;
  const uint64_t slice = witness_slice_elems(n_vars, count);
  r.slice_aligned = count > 1 && slice * (uint64_t)(count - 1) < n_vars;
  r.wlo = r.slice_aligned ? (uint32_t)(slice * (uint64_t)rank) : (uint32_t)((uint64_t)n_vars * rank / count);
  const uint64_t slice_end = slice * (uint64_t)(rank + 1);
  r.whi = r.slice_aligned ? (uint32_t)(slice_end < n_vars ? slice_end : n_vars) : (uint32_t)((uint64_t)n_vars * (rank + 1) / count);
  const uint32_t skip = n_public + 1;
  r.clo = (r.wlo > skip ? r.wlo : skip) - skip;
  r.chi = (r.whi > skip ? r.whi : skip) - skip;
  r.h_strided = count > 1 && (count & (count - 1)) == 0 && domain / (uint32_t)count >= 1024;
  r.hlo = r.h_strided ? 0 : (uint32_t)((uint64_t)domain * rank / count);
  r.hhi = r.h_strided ? domain / (uint32_t)count : (uint32_t)((uint64_t)domain * (rank + 1) / count);
  r.h_stride = r.h_strided ? (uint32_t)count : 1;
  r.h_first = r.h_strided ? (uint32_t)rank : 0;
  return r;
}

} // namespace prover
} // namespace isnark
