// arith_probe.hip — test-only probes of the lane-level arithmetic (csrc/ff.h, ec.h, ff29.h, fr29.h, ec29.h).
//
// One `lane_*` function per operation applies ONE primitive to inputs read from a flat array of packed 32-byte words
// and writes packed outputs; nothing here is linked into the product library.  The file is compiled
//   * by hipcc for gfx950 (Makefile: libisnark_arith_probe.so): every operation becomes a __global__ kernel, one lane
//     per element, and an extern "C" launcher `probe_<op><suffix>(in, out, n)` that returns the first HIP error;
//   * twice for the Fq2 / G2 operations, with and without -DISNARK_FQ2_INLINE (-DPROBE_FQ2_ONLY -DPROBE_SUFFIX=_inline),
//     the two instantiations of Fq2Ops::mul / sqr the product uses;
//   * by g++ at test time (tests/arith_probe_cases.py): the `probe_<op>_host` runners loop the same lane functions on
//     the CPU, optionally with -DF29_CHECK, where every bound stated in ff29.h / ec29.h is asserted.
// Layout: lane i reads words [i·NIN, (i+1)·NIN) and writes words [i·NOUT, (i+1)·NOUT).  An Fq2 element is two words
// (c0, c1), an affine point (x, y), XYZZ (x, y, zz, zzz), projective (X, Y, Z).  Expected values: tests/arith_probe_model.py.
#include <stddef.h>
#include <stdint.h>

#include "ec29.h"
#include "fr29.h"

#ifndef PROBE_SUFFIX
#define PROBE_SUFFIX
#endif
#define PROBE_CAT3_(a, b, c) a##b##c
#define PROBE_CAT3(a, b, c) PROBE_CAT3_(a, b, c)
#define PROBE_EXPORT extern "C" __attribute__((visibility("default")))

using namespace bn254;

namespace {

// ------------------------------------------------------------------------------------------------ loads / stores
FF_HD void get(const fe* p, fe& v) { v = p[0]; }
FF_HD void get(const fe* p, fe2& v) { v.c0 = p[0], v.c1 = p[1]; }
FF_HD void put(fe* p, const fe& v) { p[0] = v; }
FF_HD void put(fe* p, const fe2& v) { p[0] = v.c0, p[1] = v.c1; }
template <class F>
FF_HD Affine<F> get_a(const fe* p)
{
  Affine<F> a;
  get(p, a.x), get(p + F::NFE, a.y);
  return a;
}
template <class F>
FF_HD XYZZ<F> get_x(const fe* p)
{
  XYZZ<F> a;
  get(p, a.x), get(p + F::NFE, a.y), get(p + 2 * F::NFE, a.zz), get(p + 3 * F::NFE, a.zzz);
  return a;
}
template <class F>
FF_HD Projective<F> get_p(const fe* p)
{
  Projective<F> a;
  get(p, a.x), get(p + F::NFE, a.y), get(p + 2 * F::NFE, a.z);
  return a;
}
template <class F>
FF_HD void put_a(fe* p, const Affine<F>& a) { put(p, a.x), put(p + F::NFE, a.y); }
template <class F>
FF_HD void put_x(fe* p, const XYZZ<F>& a) { put(p, a.x), put(p + F::NFE, a.y), put(p + 2 * F::NFE, a.zz), put(p + 3 * F::NFE, a.zzz); }
template <class F>
FF_HD void put_p(fe* p, const Projective<F>& a) { put(p, a.x), put(p + F::NFE, a.y), put(p + 2 * F::NFE, a.z); }
FF_HD fe flag(uint32_t bits)
{
  fe r = Fq::zero();
  r.l[0] = bits;
  return r;
}

#if !defined(PROBE_FQ2_ONLY)
// ------------------------------------------------------------------------------------------------ Fp<FrP>, Fp<FqP>
template <class F> FF_HD void lane_add(const fe* in, fe* out) { out[0] = F::add(in[0], in[1]); }
template <class F> FF_HD void lane_sub(const fe* in, fe* out) { out[0] = F::sub(in[0], in[1]); }
template <class F> FF_HD void lane_neg(const fe* in, fe* out) { out[0] = F::neg(in[0]); }
template <class F> FF_HD void lane_dbl(const fe* in, fe* out) { out[0] = F::dbl(in[0]); }
template <class F> FF_HD void lane_mul3(const fe* in, fe* out) { out[0] = F::mul3(in[0]); }
template <class F> FF_HD void lane_mul(const fe* in, fe* out) { out[0] = F::mul(in[0], in[1]); }
template <class F> FF_HD void lane_sqr(const fe* in, fe* out) { out[0] = F::sqr(in[0]); }
template <class F> FF_HD void lane_mul2sum(const fe* in, fe* out) { out[0] = F::mul2sum(in[0], in[1], in[2], in[3]); }
template <class F> FF_HD void lane_to_mont(const fe* in, fe* out) { out[0] = F::to_mont(in[0]); }
template <class F> FF_HD void lane_from_mont(const fe* in, fe* out) { out[0] = F::from_mont(in[0]); }
template <class F> FF_HD void lane_inv(const fe* in, fe* out) { out[0] = F::inv(in[0]); }
template <class F> FF_HD void lane_reduce_once(const fe* in, fe* out) { out[0] = F::reduce_once(in[0]); }
template <class F> FF_HD void lane_is_canonical(const fe* in, fe* out) { out[0] = flag(F::is_canonical(in[0]) ? 1u : 0u); }

// ------------------------------------------------------------------------------------------------ f29 over Fq
// inputs: canonical standard-form words, brought into the lazy Montgomery-261 form with from_std as f29_check_field does
FF_HD void lane_f29_from_std(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::from_std(in[0])); }
FF_HD void lane_f29_from_mont256(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::from_mont256(in[0])); }
FF_HD void lane_f29_pack_canon_unpack(const fe* in, fe* out) { out[0] = f29::pack(f29::canon(f29::unpack(in[0]))); } // any 256-bit word (< 6p)
FF_HD void lane_f29_mul(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::mul(f29::from_std(in[0]), f29::from_std(in[1]))); }
FF_HD void lane_f29_sqr(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::sqr(f29::from_std(in[0]))); }
FF_HD void lane_f29_mul2(const fe* in, fe* out)
{
  out[0] = f29::to_mont256(f29::mul2(f29::from_std(in[0]), f29::from_std(in[1]), f29::from_std(in[2]), f29::from_std(in[3])));
}
FF_HD void lane_f29_mul4(const fe* in, fe* out) // a·b + c·d + a·c + b·d
{
  const fe9 a = f29::from_std(in[0]), b = f29::from_std(in[1]), c = f29::from_std(in[2]), d = f29::from_std(in[3]);
  out[0] = f29::to_mont256(f29::mul4(a, b, c, d, a, c, b, d));
}
FF_HD void lane_f29_sub31(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::norm(f29::sub<3, 1>(f29::from_std(in[0]), f29::from_std(in[1])))); }
FF_HD void lane_f29_sub53(const fe* in, fe* out) // a − (b + 2c)
{
  const fe9 a = f29::from_std(in[0]), b = f29::from_std(in[1]), c = f29::from_std(in[2]);
  out[0] = f29::to_mont256(f29::reduce_lt2p(f29::norm(f29::sub<5, 3>(a, f29::add(b, f29::dbl(c))))));
}
FF_HD void lane_f29_sqr_lazy(const fe* in, fe* out) // square of a lazy difference (N, < 5p)
{
  out[0] = f29::to_mont256(f29::sqr(f29::norm(f29::sub<3, 1>(f29::from_std(in[0]), f29::from_std(in[1])))));
}
FF_HD void lane_f29_inv(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::inv(f29::from_std(in[0]))); }
FF_HD void lane_f29_inv_ds(const fe* in, fe* out) { out[0] = f29::to_mont256(f29::inv_ds(f29::from_std(in[0]))); }
FF_HD void lane_f29_inv_ds_lazy(const fe* in, fe* out) // inverse of a lazy sum (N, < 4p)
{
  const fe9 a = f29::from_std(in[0]), b = f29::mul(f29::from_std(in[1]), f29::one_m());
  out[0] = f29::to_mont256(f29::inv_ds(f29::norm(f29::add(a, b))));
}
// bit 0: maybe_zero_mod_p(a − a), bit 1: is_zero_canon(canon(a − a)), bit 2 / 3: the same on a − b
FF_HD void lane_f29_zero_tests(const fe* in, fe* out)
{
  const fe9 a = f29::from_std(in[0]), b = f29::from_std(in[1]);
  const fe9 z = f29::norm(f29::sub<3, 1>(a, a)), w = f29::norm(f29::sub<3, 1>(a, b));
  out[0] = flag((f29::maybe_zero_mod_p(z) ? 1u : 0u) | (f29::is_zero_canon(f29::canon(z)) ? 2u : 0u) | (f29::maybe_zero_mod_p(w) ? 4u : 0u) |
                (f29::is_zero_canon(f29::canon(w)) ? 8u : 0u));
}

// ------------------------------------------------------------------------------------------------ fr29 over Fr
// (the NTT's arithmetic: data in standard form, the second factor a canonical Montgomery-261 "twiddle")
FF_HD fe9 fr29_twiddle(const fe& w) { return fr29::canon(fr29::mul(fr29::unpack(w), fr29::r2())); }
FF_HD void lane_fr29_from_std(const fe* in, fe* out) // std → Montgomery-261 → std
{
  fe9 one;
  for (int i = 0; i < 9; i++) one.l[i] = i == 0 ? 1u : 0u;
  out[0] = fr29::pack(fr29::canon(fr29::mul(fr29_twiddle(in[0]), one)));
}
FF_HD void lane_fr29_from_mont256(const fe* in, fe* out) { out[0] = fr29::pack(fr29::canon(fr29::mul(fr29::unpack(in[0]), fr29::c256_to_261()))); } // x ↦ 32·x
FF_HD void lane_fr29_pack_canon_unpack(const fe* in, fe* out) { out[0] = fr29::pack(fr29::canon(fr29::unpack(in[0]))); } // any 256-bit word
FF_HD void lane_fr29_mul(const fe* in, fe* out) { out[0] = fr29::pack(fr29::canon(fr29::mul(fr29::unpack(in[0]), fr29_twiddle(in[1])))); }
FF_HD void lane_fr29_mul_lazy(const fe* in, fe* out) // (a + b + 2r − c)·w: limbs < 2^31, not normalised, as inside a butterfly
{
  const fe9 s = fr29::add(fr29::unpack(in[0]), fr29::sub<2>(fr29::unpack(in[1]), fr29::unpack(in[2])));
  out[0] = fr29::pack(fr29::canon(fr29::mul(s, fr29_twiddle(in[3]))));
}
FF_HD void lane_fr29_sub2(const fe* in, fe* out) { out[0] = fr29::pack(fr29::canon4(fr29::norm(fr29::sub<2>(fr29::unpack(in[0]), fr29::unpack(in[1]))))); }
FF_HD void lane_fr29_sub1300(const fe* in, fe* out) // a + 1300r − b through canon, and through shrink (→ < 319) then canon
{
  const fe9 t = fr29::norm(fr29::sub<1300>(fr29::unpack(in[0]), fr29::unpack(in[1])));
  out[0] = fr29::pack(fr29::canon(t));
  out[1] = fr29::pack(fr29::canon(fr29::shrink(t)));
}
#endif // !PROBE_FQ2_ONLY

// ------------------------------------------------------------------------------------------------ FqOps / Fq2Ops
template <class F> FF_HD void lane_f_add(const fe* in, fe* out) { typename F::T a, b; get(in, a), get(in + F::NFE, b); put(out, F::add(a, b)); }
template <class F> FF_HD void lane_f_sub(const fe* in, fe* out) { typename F::T a, b; get(in, a), get(in + F::NFE, b); put(out, F::sub(a, b)); }
template <class F> FF_HD void lane_f_neg(const fe* in, fe* out) { typename F::T a; get(in, a); put(out, F::neg(a)); }
template <class F> FF_HD void lane_f_dbl(const fe* in, fe* out) { typename F::T a; get(in, a); put(out, F::dbl(a)); }
template <class F> FF_HD void lane_f_mul(const fe* in, fe* out) { typename F::T a, b; get(in, a), get(in + F::NFE, b); put(out, F::mul(a, b)); }
template <class F> FF_HD void lane_f_sqr(const fe* in, fe* out) { typename F::T a; get(in, a); put(out, F::sqr(a)); }
template <class F> FF_HD void lane_f_inv(const fe* in, fe* out) { typename F::T a; get(in, a); put(out, F::inv(a)); }
template <class F> FF_HD void lane_f_mul_sub_mul(const fe* in, fe* out)
{
  typename F::T a, b, c, d;
  get(in, a), get(in + F::NFE, b), get(in + 2 * F::NFE, c), get(in + 3 * F::NFE, d);
  put(out, F::mul_sub_mul(a, b, c, d));
}

// ------------------------------------------------------------------------------------------------ Curve<F> (ec.h)
// Montgomery-form coordinates in and out, raw.  x_madd's contract excludes the affine identity: the callers skip it, so does the lane.
template <class F> FF_HD void lane_x_madd(const fe* in, fe* out)
{
  XYZZ<F> acc = get_x<F>(in);
  const Affine<F> q = get_a<F>(in + 4 * F::NFE);
  if (!Curve<F>::aff_is_zero(q)) Curve<F>::x_madd(acc, q);
  put_x<F>(out, acc);
}
template <class F> FF_HD void lane_x_add(const fe* in, fe* out) { put_x<F>(out, Curve<F>::x_add(get_x<F>(in), get_x<F>(in + 4 * F::NFE))); }
template <class F> FF_HD void lane_x_dbl(const fe* in, fe* out) { put_x<F>(out, Curve<F>::x_dbl(get_x<F>(in))); }
template <class F> FF_HD void lane_x_dbl_affine(const fe* in, fe* out) { put_x<F>(out, Curve<F>::x_dbl_affine(get_a<F>(in))); }
template <class F> FF_HD void lane_x_proj_roundtrip(const fe* in, fe* out) { put_p<F>(out, Curve<F>::x_to_projective(Curve<F>::x_from_projective(get_p<F>(in)))); }
// p_add / p_dbl: the last input element is 3·b in Montgomery form
template <class F> FF_HD void lane_p_add(const fe* in, fe* out)
{
  typename F::T b3;
  get(in + 6 * F::NFE, b3);
  put_p<F>(out, Curve<F>::p_add(get_p<F>(in), get_p<F>(in + 3 * F::NFE), b3));
}
template <class F> FF_HD void lane_p_dbl(const fe* in, fe* out)
{
  typename F::T b3;
  get(in + 3 * F::NFE, b3);
  put_p<F>(out, Curve<F>::p_dbl(get_p<F>(in), b3));
}
template <class F> FF_HD void lane_p_to_affine(const fe* in, fe* out) { put_a<F>(out, Curve<F>::p_to_affine(get_p<F>(in))); }
template <class F> FF_HD void lane_p_eq(const fe* in, fe* out) { out[0] = flag(Curve<F>::p_eq(get_p<F>(in), get_p<F>(in + 3 * F::NFE)) ? 1u : 0u); }


#if !defined(PROBE_FQ2_ONLY)
// ------------------------------------------------------------------------------------------------ CurveL<F> (ec29.h)
// Packed inputs as the kernels find them in memory: affine bases in one of the three encodings, XYZZ accumulators as ec.h's
// canonical Montgomery-256 tuples (x_from_old).  Results leave through x_store / store_mont256, the packed exits of ec29.h.
template <class F> FF_HD Affine<typename F::Old> get_la(const fe* p) { return get_a<typename F::Old>(p); }
template <class F, int FORM, int NEG> FF_HD void lane_l_load_affine(const fe* in, fe* out)
{
  constexpr int NFE = F::Old::NFE;
  const typename CurveL<F>::A a = CurveL<F>::load_affine(get_la<F>(in), FORM, NEG != 0);
  put(out, F::store_mont256(a.x)), put(out + NFE, F::store_mont256(a.y));
}
template <class F> FF_HD void lane_l_x_madd(const fe* in, fe* out)
{
  typedef typename F::Old O;
  typename CurveL<F>::X acc = CurveL<F>::x_from_old(get_x<O>(in));
  const Affine<O> q = get_la<F>(in + 4 * O::NFE);
  if (!Curve<O>::aff_is_zero(q)) CurveL<F>::x_madd(acc, CurveL<F>::load_affine(q, CurveL<F>::MONT256, false));
  put_x<O>(out, CurveL<F>::x_store(acc));
}
template <class F> FF_HD void lane_l_x_add(const fe* in, fe* out)
{
  typedef typename F::Old O;
  put_x<O>(out, CurveL<F>::x_store(CurveL<F>::x_add(CurveL<F>::x_from_old(get_x<O>(in)), CurveL<F>::x_from_old(get_x<O>(in + 4 * O::NFE)))));
}
template <class F> FF_HD void lane_l_x_dbl(const fe* in, fe* out)
{
  typedef typename F::Old O;
  put_x<O>(out, CurveL<F>::x_store(CurveL<F>::x_dbl(CurveL<F>::x_from_old(get_x<O>(in)))));
}
template <class F> FF_HD void lane_l_x_dbl_affine_exact(const fe* in, fe* out)
{
  typedef typename F::Old O;
  put_x<O>(out, CurveL<F>::x_store(CurveL<F>::x_dbl_affine_exact(CurveL<F>::load_affine(get_la<F>(in), CurveL<F>::MONT256, false))));
}
template <class F> FF_HD void lane_l_x_from_old(const fe* in, fe* out)
{
  typedef typename F::Old O;
  put_x<O>(out, CurveL<F>::x_store(CurveL<F>::x_from_old(get_x<O>(in))));
}
template <class F> FF_HD void lane_l_x_internal_roundtrip(const fe* in, fe* out) // second output: the internal encoding itself
{
  typedef typename F::Old O;
  const XYZZ<O> enc = CurveL<F>::x_store_internal(CurveL<F>::x_from_old(get_x<O>(in)));
  put_x<O>(out, CurveL<F>::x_store(CurveL<F>::x_load_internal(enc)));
  put_x<O>(out + 4 * O::NFE, enc);
}
// a bucket's life: CHAIN x_madd steps on one lane, in both arithmetics.  Per step one affine base (Montgomery-256) and one
// word whose bit 0 is the sign.  Outputs: ec.h's accumulator, then ec29.h's through x_store.
constexpr int CHAIN = 200;
template <class F> FF_HD void lane_l_chain(const fe* in, fe* out)
{
  typedef typename F::Old O;
  constexpr int STEP = 2 * O::NFE + 1;
  XYZZ<O> ref = Curve<O>::x_zero();
  typename CurveL<F>::X acc = CurveL<F>::x_zero();
  for (int s = 0; s < CHAIN; s++) {
    const Affine<O> q = get_la<F>(in + s * STEP);
    const bool negate = (in[s * STEP + 2 * O::NFE].l[0] & 1u) != 0;
    Curve<O>::x_madd(ref, negate ? Curve<O>::aff_neg(q) : q);
    CurveL<F>::x_madd(acc, CurveL<F>::load_affine(q, CurveL<F>::MONT256, negate));
  }
  put_x<O>(out, ref);
  put_x<O>(out + 4 * O::NFE, CurveL<F>::x_store(acc));
}
#endif // !PROBE_FQ2_ONLY

} // namespace

// ------------------------------------------------------------------------------------------------ runners
#if defined(__HIPCC__)
namespace {
template <class K>
int probe_launch(K kernel, int nin, int nout, int block, const void* in, void* out, int n)
{
  if (n <= 0) return 0;
  fe *din = nullptr, *dout = nullptr;
  const size_t bin = (size_t)n * nin * sizeof(fe), bout = (size_t)n * nout * sizeof(fe);
  hipError_t e = hipMalloc((void**)&din, bin);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, bout);
  if (e == hipSuccess) e = hipMemcpy(din, in, bin, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    kernel<<<dim3((unsigned)((n + block - 1) / block)), dim3((unsigned)block)>>>(din, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}
} // namespace
#define PROBE_DEVICE(name, NIN, NOUT, BLOCK, ...)                                                                      \
  namespace {                                                                                                          \
  __global__ void PROBE_CAT3(k_, name, PROBE_SUFFIX)(const fe* in, fe* out, int n)                                     \
  {                                                                                                                    \
    const int i = blockIdx.x * blockDim.x + threadIdx.x;                                                               \
    if (i >= n) return;                                                                                                \
    __VA_ARGS__(in + (size_t)i * (NIN), out + (size_t)i * (NOUT));                                                     \
  }                                                                                                                    \
  }                                                                                                                    \
  PROBE_EXPORT int PROBE_CAT3(probe_, name, PROBE_SUFFIX)(const void* in, void* out, int n)                            \
  {                                                                                                                    \
    return probe_launch(PROBE_CAT3(k_, name, PROBE_SUFFIX), NIN, NOUT, BLOCK, in, out, n);                             \
  }
#else
#define PROBE_DEVICE(name, NIN, NOUT, BLOCK, ...)
#endif

// host twin: the same lane function, looped on the CPU
#if defined(PROBE_NO_HOST)
#define PROBE_HOST(name, NIN, NOUT, ...)
#else
#define PROBE_HOST(name, NIN, NOUT, ...)                                                                               \
  PROBE_EXPORT int PROBE_CAT3(probe_, name, PROBE_CAT3(PROBE_SUFFIX, _, host))(const void* in, void* out, int n)       \
  {                                                                                                                    \
    for (int i = 0; i < n; i++) __VA_ARGS__((const fe*)in + (size_t)i * (NIN), (fe*)out + (size_t)i * (NOUT));         \
    return 0;                                                                                                          \
  }
#endif
// PROBE(name, words in, words out, block size, lane function)
#define PROBE(name, NIN, NOUT, BLOCK, ...) PROBE_DEVICE(name, NIN, NOUT, BLOCK, __VA_ARGS__) PROBE_HOST(name, NIN, NOUT, __VA_ARGS__)

#if defined(F29_CHECK)
PROBE_EXPORT const char* probe_check_failure() { return f29::g_check_failure; }
PROBE_EXPORT void probe_check_reset() { f29::g_check_failure = nullptr; }
#endif

#if !defined(PROBE_FQ2_ONLY)
#define PROBE_FIELD(pfx, F)                                                                                            \
  PROBE(pfx##_add, 2, 1, 256, lane_add<F>)                                                                             \
  PROBE(pfx##_sub, 2, 1, 256, lane_sub<F>)                                                                             \
  PROBE(pfx##_neg, 1, 1, 256, lane_neg<F>)                                                                             \
  PROBE(pfx##_dbl, 1, 1, 256, lane_dbl<F>)                                                                             \
  PROBE(pfx##_mul3, 1, 1, 256, lane_mul3<F>)                                                                           \
  PROBE(pfx##_mul, 2, 1, 256, lane_mul<F>)                                                                             \
  PROBE(pfx##_sqr, 1, 1, 256, lane_sqr<F>)                                                                             \
  PROBE(pfx##_mul2sum, 4, 1, 256, lane_mul2sum<F>)                                                                     \
  PROBE(pfx##_to_mont, 1, 1, 256, lane_to_mont<F>)                                                                     \
  PROBE(pfx##_from_mont, 1, 1, 256, lane_from_mont<F>)                                                                 \
  PROBE(pfx##_inv, 1, 1, 64, lane_inv<F>)                                                                              \
  PROBE(pfx##_reduce_once, 1, 1, 256, lane_reduce_once<F>)                                                             \
  PROBE(pfx##_is_canonical, 1, 1, 256, lane_is_canonical<F>)
PROBE_FIELD(fr, Fr)
PROBE_FIELD(fq, Fq)

PROBE(f29_from_std, 1, 1, 256, lane_f29_from_std)
PROBE(f29_from_mont256, 1, 1, 256, lane_f29_from_mont256)
PROBE(f29_pack_canon_unpack, 1, 1, 256, lane_f29_pack_canon_unpack)
PROBE(f29_mul, 2, 1, 256, lane_f29_mul)
PROBE(f29_sqr, 1, 1, 256, lane_f29_sqr)
PROBE(f29_mul2, 4, 1, 256, lane_f29_mul2)
PROBE(f29_mul4, 4, 1, 256, lane_f29_mul4)
PROBE(f29_sub31, 2, 1, 256, lane_f29_sub31)
PROBE(f29_sub53, 3, 1, 256, lane_f29_sub53)
PROBE(f29_sqr_lazy, 2, 1, 256, lane_f29_sqr_lazy)
PROBE(f29_inv, 1, 1, 64, lane_f29_inv)
PROBE(f29_inv_ds, 1, 1, 64, lane_f29_inv_ds)
PROBE(f29_inv_ds_lazy, 2, 1, 64, lane_f29_inv_ds_lazy)
PROBE(f29_zero_tests, 2, 1, 256, lane_f29_zero_tests)

PROBE(fr29_from_std, 1, 1, 256, lane_fr29_from_std)
PROBE(fr29_from_mont256, 1, 1, 256, lane_fr29_from_mont256)
PROBE(fr29_pack_canon_unpack, 1, 1, 256, lane_fr29_pack_canon_unpack)
PROBE(fr29_mul, 2, 1, 256, lane_fr29_mul)
PROBE(fr29_mul_lazy, 4, 1, 256, lane_fr29_mul_lazy)
PROBE(fr29_sub2, 2, 1, 256, lane_fr29_sub2)
PROBE(fr29_sub1300, 2, 2, 256, lane_fr29_sub1300)
#endif

// field-interface and curve operations of ec.h: W = words per coordinate
#define PROBE_FOPS(pfx, F, W)                                                                                          \
  PROBE(pfx##_add, 2 * W, W, 256, lane_f_add<F>)                                                                       \
  PROBE(pfx##_sub, 2 * W, W, 256, lane_f_sub<F>)                                                                       \
  PROBE(pfx##_neg, W, W, 256, lane_f_neg<F>)                                                                           \
  PROBE(pfx##_dbl, W, W, 256, lane_f_dbl<F>)                                                                           \
  PROBE(pfx##_mul, 2 * W, W, 256, lane_f_mul<F>)                                                                       \
  PROBE(pfx##_sqr, W, W, 256, lane_f_sqr<F>)                                                                           \
  PROBE(pfx##_inv, W, W, 64, lane_f_inv<F>)                                                                            \
  PROBE(pfx##_mul_sub_mul, 4 * W, W, 256, lane_f_mul_sub_mul<F>)
#define PROBE_CURVE(pfx, F, W)                                                                                         \
  PROBE(pfx##_x_madd, 6 * W, 4 * W, 64, lane_x_madd<F>)                                                                \
  PROBE(pfx##_x_add, 8 * W, 4 * W, 64, lane_x_add<F>)                                                                  \
  PROBE(pfx##_x_dbl, 4 * W, 4 * W, 64, lane_x_dbl<F>)                                                                  \
  PROBE(pfx##_x_dbl_affine, 2 * W, 4 * W, 64, lane_x_dbl_affine<F>)                                                    \
  PROBE(pfx##_x_proj_roundtrip, 3 * W, 3 * W, 64, lane_x_proj_roundtrip<F>)                                            \
  PROBE(pfx##_p_add, 7 * W, 3 * W, 64, lane_p_add<F>)                                                                  \
  PROBE(pfx##_p_dbl, 4 * W, 3 * W, 64, lane_p_dbl<F>)                                                                  \
  PROBE(pfx##_p_to_affine, 3 * W, 2 * W, 64, lane_p_to_affine<F>)                                                      \
  PROBE(pfx##_p_eq, 6 * W, 1, 64, lane_p_eq<F>)
#if !defined(PROBE_FQ2_ONLY)
PROBE_FOPS(fqops, FqOps, 1)
PROBE_CURVE(g1, FqOps, 1)
#endif
PROBE_FOPS(fq2, Fq2Ops, 2)
PROBE_CURVE(g2, Fq2Ops, 2)

#if !defined(PROBE_FQ2_ONLY)
#define PROBE_CURVEL(pfx, F, W)                                                                                        \
  PROBE(pfx##_load_affine_std, 2 * W, 2 * W, 64, lane_l_load_affine<F, 0, 0>)                                          \
  PROBE(pfx##_load_affine_std_neg, 2 * W, 2 * W, 64, lane_l_load_affine<F, 0, 1>)                                      \
  PROBE(pfx##_load_affine_mont256, 2 * W, 2 * W, 64, lane_l_load_affine<F, 1, 0>)                                      \
  PROBE(pfx##_load_affine_mont256_neg, 2 * W, 2 * W, 64, lane_l_load_affine<F, 1, 1>)                                  \
  PROBE(pfx##_load_affine_internal, 2 * W, 2 * W, 64, lane_l_load_affine<F, 2, 0>)                                     \
  PROBE(pfx##_load_affine_internal_neg, 2 * W, 2 * W, 64, lane_l_load_affine<F, 2, 1>)                                 \
  PROBE(pfx##_x_madd, 6 * W, 4 * W, 64, lane_l_x_madd<F>)                                                              \
  PROBE(pfx##_x_add, 8 * W, 4 * W, 64, lane_l_x_add<F>)                                                                \
  PROBE(pfx##_x_dbl, 4 * W, 4 * W, 64, lane_l_x_dbl<F>)                                                                \
  PROBE(pfx##_x_dbl_affine_exact, 2 * W, 4 * W, 64, lane_l_x_dbl_affine_exact<F>)                                      \
  PROBE(pfx##_x_from_old, 4 * W, 4 * W, 64, lane_l_x_from_old<F>)                                                      \
  PROBE(pfx##_x_internal_roundtrip, 4 * W, 8 * W, 64, lane_l_x_internal_roundtrip<F>)                                  \
  PROBE(pfx##_chain, CHAIN * (2 * W + 1), 8 * W, 64, lane_l_chain<F>)
PROBE_CURVEL(g1l, Fq29, 1)
PROBE_CURVEL(g2l, Fq2_29, 2)
#endif
