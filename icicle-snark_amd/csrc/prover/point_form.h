// point_form.h — projective sums back to the file's form, for the tools that write points (ptau_prepare.hip, ptau_contribute.hip,
// ptau_truncate.hip, zkey_contribute.hip, zkey_new.hip, zkey_setup.hip), and the trait their per-curve kernels read the lazy field from.  A header
// of its own beside device_call.h, not part of msm_impl.h: it reports through DEV_LAUNCH, and msm_impl.h — which the MSM's own
// translation units compile — stays as it is.  The kernels are msm_impl.h's.
#pragma once
#include "../msm_impl.h"
#include "device_call.h"

namespace isnark {
namespace prover {

// the lazy field (ec29.h's CurveL<F>) and the field operations of ec.h's two curves
template <class C>
struct Group;
template <>
struct Group<bn254::G1> {
  typedef bn254::Fq29 F;
  typedef bn254::FqOps Fo;
};
template <>
struct Group<bn254::G2> {
  typedef bn254::Fq2_29 F;
  typedef bn254::Fq2Ops Fo;
};

// d_proj[i], i < n (Montgomery projective, the identity (0, 1, 0)) → d_aff[i] in the file's form: affine, Montgomery, the identity
// all zero.  batch_to_affine_kernel inverts in chunks of 32 with one scratch element a point, affine_to_mont_kernel walks the
// coordinates; both enqueued on `st`, nothing synchronised.
template <class C>
int to_file_form(hipStream_t st, const typename C::P* d_proj, uint64_t n, typename C::A* d_aff, typename Group<C>::Fo::T* d_scratch)
{
  typedef typename C::A A;
  const int chunk = 32;
  const uint64_t threads = (n + chunk - 1) / chunk, ncoord = n * (sizeof(A) / sizeof(bn254::fe));
  DEV_LAUNCH("batch_to_affine launch", (batch_to_affine_kernel<C, typename Group<C>::Fo>), dim3((uint32_t)((threads + 63) / 64)), dim3(64), st, d_proj, n, chunk, d_aff, d_scratch);
  DEV_LAUNCH("affine_to_mont launch", (affine_to_mont_kernel<A>), dim3((uint32_t)((ncoord + 255) / 256)), dim3(256), st, d_aff, ncoord);
  return 0;
}

// d_scalars[i]·G for i < n (standard-form scalars on the device, 0 ↦ the identity) → d_aff[i] in the file's form: generator_mul's
// three kernels on device operands.  d_table: FIXED_BASE_TABLE_POINTS entries; d_proj, d_scratch: n entries each.  Enqueued on `st`.
constexpr size_t FIXED_BASE_TABLE_POINTS = 32 * 255;
template <class C>
int generator_mul_to_file_form(hipStream_t st, const bn254::fe* d_scalars, uint64_t n, const typename C::A& gen_mont, typename C::X* d_table, typename C::P* d_proj,
                               typename C::A* d_aff, typename Group<C>::Fo::T* d_scratch)
{
  if (!n) return 0;
  DEV_LAUNCH("fixed_base_table launch", (fixed_base_table_kernel<C>), dim3(1), dim3(256), st, gen_mont, d_table);
  DEV_LAUNCH("fixed_base_mul launch", (fixed_base_mul_kernel<C>), dim3((uint32_t)((n + 255) / 256)), dim3(256), st, d_scalars, n, d_table, d_proj);
  return to_file_form<C>(st, d_proj, n, d_aff, d_scratch);
}

} // namespace prover
} // namespace isnark
