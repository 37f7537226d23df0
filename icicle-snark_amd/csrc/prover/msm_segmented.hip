// msm_segmented.hip — many small G1 multi-scalar sums in one launch.
//
//   icicle_snark_msm_segmented   out[s] = Σ_{k ∈ [offsets[s], offsets[s+1])} scalars[k]·points[k], canonical affine, (0, 0) = O
//
// bn254_msm's sort → accumulate → reduce chain is sized for 2^20 points; the mixed-key verifier (verify_mixed.hip) needs 3·K sums
// of 1 … n entries each.  Here a sum is a workgroup's: a lane strides over the entries of its piece and walks their scalars'
// bits together — one doubling per bit for all of the lane's entries, one mixed addition per set bit (Straus, as
// p29::public_input) — on ec29.h's XYZZ layer, the lanes' sums are added through an LDS tree, and lane 0 writes the result.
// A segment longer than `cut` entries is cut into pieces, one workgroup each, whose XYZZ sums a second launch adds per segment
// (zkey_columns.h's heavy columns, with the plan made on the host: the offsets are the host's).  The result leaves as canonical
// affine coordinates, so it does not depend on cut, on the piece order or on the shape of the tree; nothing is accumulated with
// atomics.  Degenerate operands take ec29.h's exact branches: an identity point is skipped, a zero scalar adds nothing, and
// x_madd / x_add decide P + P and P + (−P) on canonical values.
#include <string.h>
#include <vector>

#include "../common.h"
#include "../pairing29.h"

using namespace bn254;

namespace {

constexpr uint32_t DEFAULT_SEGMENT_CUT = 1024; // entries per piece; the sweep is profiles/verify_mixed_sweep.txt
constexpr int PIECE_WG = 256;                  // lanes of a piece's workgroup
constexpr int JOIN_WG = 64;                    // lanes of a cut segment's workgroup in the second launch

struct Piece { // entries [lo, lo + n) of the caller's arrays
  uint64_t lo;
  uint32_t n, bits;
  uint32_t dst;     // the segment (out[dst]) when the piece is its whole segment, else the slot of its XYZZ sum
  uint32_t partial; // 1: a piece of a cut segment
};
struct Join { // a cut segment: out[seg] = Σ slots [first, first + count)
  uint32_t seg, first, count;
};

// the lanes' sums added in LDS; every lane of the workgroup calls it, the sum comes back in lane 0
template <int WG>
__device__ G1L::X workgroup_sum(const G1L::X& mine, G1L::X* sh)
{
  const int t = threadIdx.x;
  sh[t] = mine;
  __syncthreads();
  for (int h = WG / 2; h >= 1; h >>= 1) {
    if (t < h) sh[t] = G1L::x_add(sh[t], sh[t + h]);
    __syncthreads();
  }
  return sh[0];
}

// XYZZ → canonical standard-form affine, (0, 0) for the identity
__device__ void store_affine_std(const G1L::X& p, fe* out)
{
  if (G1L::x_is_zero(p)) {
    fe z;
    for (int i = 0; i < 8; i++) z.l[i] = 0;
    out[0] = out[1] = z;
    return;
  }
  fe9 x, y;
  p29::g1_to_affine(p, x, y);
  out[0] = f29::pack(f29::canon(f29::mul(x, f29::one_std())));
  out[1] = f29::pack(f29::canon(f29::mul(y, f29::one_std())));
}

// one workgroup per piece
__global__ __launch_bounds__(PIECE_WG) void msm_segmented_kernel(const fe* __restrict__ points, const fe* __restrict__ scalars, const Piece* __restrict__ pieces,
                                                                 G1::X* __restrict__ partials, fe* __restrict__ out)
{
  __shared__ G1L::X sh[PIECE_WG];
  const Piece pc = pieces[blockIdx.x];
  const uint32_t t = threadIdx.x;
  G1L::X acc = G1L::x_zero();
  if (t < pc.n) {
    for (int i = (int)pc.bits - 1; i >= 0; i--) {
      acc = G1L::x_dbl(acc);
      for (uint32_t k = t; k < pc.n; k += PIECE_WG) {
        const uint64_t e = pc.lo + k;
        if (!((scalars[e].l[i >> 5] >> (i & 31)) & 1u)) continue;
        const fe P[2] = {points[2 * e], points[2 * e + 1]};
        if (p29::g1_std_is_zero(P)) continue;
        G1L::x_madd(acc, {f29::from_std(P[0]), f29::from_std(P[1])});
      }
    }
  }
  const G1L::X sum = workgroup_sum<PIECE_WG>(acc, sh);
  if (t) return;
  if (pc.partial) partials[pc.dst] = G1L::x_store_internal(sum);
  else store_affine_std(sum, out + 2 * (size_t)pc.dst);
}

// one workgroup per cut segment
__global__ __launch_bounds__(JOIN_WG) void msm_segmented_join_kernel(const G1::X* __restrict__ partials, const Join* __restrict__ joins, fe* __restrict__ out)
{
  __shared__ G1L::X sh[JOIN_WG];
  const Join j = joins[blockIdx.x];
  G1L::X acc = G1L::x_zero();
  for (uint32_t k = threadIdx.x; k < j.count; k += JOIN_WG) acc = G1L::x_add(acc, G1L::x_load_internal(partials[j.first + k]));
  const G1L::X sum = workgroup_sum<JOIN_WG>(acc, sh);
  if (threadIdx.x == 0) store_affine_std(sum, out + 2 * (size_t)j.seg);
}

void free_plan(void* p) { delete[] (uint8_t*)p; }

} // namespace

ISNARK_API eIcicleError icicle_snark_msm_segmented(const bn254_affine_t* points, const bn254_scalar_t* scalars, const uint64_t* offsets, uint32_t n_segments,
                                                   const uint8_t* bits, uint32_t cut, icicleStreamHandle stream, bn254_affine_t* out)
{
  if (n_segments == 0) return ICICLE_SUCCESS;
  if (!offsets || !bits || !out) return ICICLE_INVALID_POINTER;
  if (cut == 0) cut = DEFAULT_SEGMENT_CUT;
  std::vector<Piece> pieces;
  std::vector<Join> joins;
  uint32_t slots = 0;
  for (uint32_t s = 0; s < n_segments; s++) {
    if (offsets[s + 1] < offsets[s] || (bits[s] != 128 && bits[s] != 254)) {
      isnark::set_last_error("msm_segmented: segment %u: offsets must not decrease and bits must be 128 or 254", s);
      return ICICLE_INVALID_ARGUMENT;
    }
    const uint64_t len = offsets[s + 1] - offsets[s];
    if (len <= cut) {
      pieces.push_back({offsets[s], (uint32_t)len, bits[s], s, 0});
      continue;
    }
    const uint64_t count = (len + cut - 1) / cut;
    if (count > UINT32_MAX - slots) {
      isnark::set_last_error("msm_segmented: more than 2^32 pieces");
      return ICICLE_INVALID_ARGUMENT;
    }
    joins.push_back({s, slots, (uint32_t)count});
    for (uint64_t lo = offsets[s]; lo < offsets[s + 1]; lo += cut)
      pieces.push_back({lo, (uint32_t)std::min<uint64_t>(cut, offsets[s + 1] - lo), bits[s], slots++, 1});
  }
  if (offsets[n_segments] > offsets[0] && (!points || !scalars)) return ICICLE_INVALID_POINTER;

  // the plan goes up in one copy from a block that a host function on the stream frees behind it
  const hipStream_t st = (hipStream_t)stream;
  const size_t piece_bytes = pieces.size() * sizeof(Piece), plan_bytes = piece_bytes + joins.size() * sizeof(Join);
  isnark::WsScoped<uint8_t> d_plan;
  isnark::WsScoped<G1::X> d_partials;
  if (d_plan.alloc(plan_bytes, st) != hipSuccess || d_partials.alloc(slots, st) != hipSuccess) return ICICLE_ALLOCATION_FAILED;
  uint8_t* h_plan = new (std::nothrow) uint8_t[plan_bytes];
  if (!h_plan) return ICICLE_ALLOCATION_FAILED;
  memcpy(h_plan, pieces.data(), piece_bytes);
  if (!joins.empty()) memcpy(h_plan + piece_bytes, joins.data(), joins.size() * sizeof(Join));
  if (hipMemcpyAsync(d_plan.p, h_plan, plan_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
    delete[] h_plan;
    return ICICLE_COPY_FAILED;
  }
  if (hipLaunchHostFunc(st, free_plan, h_plan) != hipSuccess) {
    (void)hipStreamSynchronize(st);
    delete[] h_plan;
  }
  hipLaunchKernelGGL(msm_segmented_kernel, dim3((uint32_t)pieces.size()), dim3(PIECE_WG), 0, st, (const fe*)points, (const fe*)scalars, (const Piece*)d_plan.p,
                     d_partials.p, (fe*)out);
  if (!joins.empty())
    hipLaunchKernelGGL(msm_segmented_join_kernel, dim3((uint32_t)joins.size()), dim3(JOIN_WG), 0, st, (const G1::X*)d_partials.p,
                       (const Join*)(d_plan.p + piece_bytes), (fe*)out);
  return isnark::check_launch("msm_segmented");
}
