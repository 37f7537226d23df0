// zkey_check29.h — membership tests of one proving-key point in the form the .zkey holds it (affine, packed Montgomery-256,
// (0, 0) = the identity), host and device: groth16_zkey_check's kernels (zkey_check.hip) run one lane per point through them, its
// host side the six header points, and the F29_CHECK host build (tests/zkey_check29_check.cpp) compiles the same text.
//
//   classify_g1(mont[2])   0 sound (the identity included), else the first of  1 a coordinate ≥ q,  2 not on y² = x³ + 3
//   classify_g2(mont[2])   0 sound (the identity included), else the first of  1 a coordinate ≥ q,  2 not on y² = x³ + 3/ξ,
//                          3 on the twist but outside the order-r subgroup
// (the values of GROTH16_ZKEY_NONCANONICAL / OFF_CURVE / OFF_SUBGROUP in include/groth16_prover.h).
//
// ORDER AND BOUNDS.  A coordinate read from a file is any 256-bit pattern, and the lazy bounds of ff29.h hold only for values
// below q: f29::from_mont256 is a mul whose value bound (product < 147·p²) is stated for a canonical operand.  So the canonical
// test comes first and is a plain integer comparison of the eight 32-bit words with q (Fq::is_canonical: a borrow chain, no field
// operation); a point that fails it returns before any lazy operation has seen its coordinates.  Then, per coordinate
//   X = from_mont256(x)     unpack (N, canonical, < p) times 2^266 mod p (canonical): p² < 147 p²                → N, < 1.01p  (I2)
// G1:
//   yy  = sqr(Y)            Y N, < 2p: 4 p²                                                                     → N, < 1.03p
//   xxx = mul(sqr(X), X)    sqr: 4 p² → N, < 1.03p; mul: 2.1 p²                                                 → N, < 1.02p
//   rhs = xxx + 3           three_m = dbl(one_m) + one_m, built limb-wise from a canonical constant: limbs < 3·2^29, < 3p;
//                           the sum has limbs < 2^31, value < 4.1p → norm → N, < 4.1p → canon (takes N, < 16p)    → canonical
//   the comparison is between canon(yy) and canon(rhs), limb by limb.
// G2: the coordinates are I2 (N, < 2p) as pairing29.h's g2_on_twist and g2_in_subgroup_fast take them; both state their own
// bounds there.  g2_in_subgroup_fast wants a point ON the twist and not the identity: it runs only behind both tests.
#pragma once
#include <stddef.h>

#include "../pairing29.h"

namespace bn254 {
namespace p29 {

enum ZkeyPointKind { ZK_SOUND = 0, ZK_NONCANONICAL = 1, ZK_OFF_CURVE = 2, ZK_OFF_SUBGROUP = 3 };

FF_HD bool mont_is_zero(const fe& a) { return std_is_zero(a); } // the all-zero words: 0 in any form

// y² = x³ + 3 for lazy Montgomery-261 coordinates (N, < 2p)
P29_HD bool g1_on_curve(const fe9& x, const fe9& y)
{
  const fe9 three = f29::add(f29::dbl(f29::one_m()), f29::one_m());                           // limbs < 3·2^29, < 3p
  const fe9 l = f29::canon(f29::sqr(y));                                                      // N, < 1.03p → canonical
  const fe9 r = f29::canon(f29::norm(f29::add(f29::mul(f29::sqr(x), x), three)));             // limbs < 2^31, < 4.1p → N → canonical
  bool eq = true;
  for (int j = 0; j < 9; j++) eq = eq && l.l[j] == r.l[j];
  return eq;
}

P29_HD int classify_g1(const fe mont[2])
{
  if (!Fq::is_canonical(mont[0]) || !Fq::is_canonical(mont[1])) return ZK_NONCANONICAL;
  if (mont_is_zero(mont[0]) && mont_is_zero(mont[1])) return ZK_SOUND;
  return g1_on_curve(f29::from_mont256(mont[0]), f29::from_mont256(mont[1])) ? ZK_SOUND : ZK_OFF_CURVE;
}

P29_HD int classify_g2(const fe2 mont[2])
{
  if (!Fq::is_canonical(mont[0].c0) || !Fq::is_canonical(mont[0].c1) || !Fq::is_canonical(mont[1].c0) || !Fq::is_canonical(mont[1].c1))
    return ZK_NONCANONICAL;
  if (mont_is_zero(mont[0].c0) && mont_is_zero(mont[0].c1) && mont_is_zero(mont[1].c0) && mont_is_zero(mont[1].c1)) return ZK_SOUND;
  const F2 x = Fq2_29::load_mont256(mont[0]), y = Fq2_29::load_mont256(mont[1]); // I2
  if (!g2_on_twist(x, y)) return ZK_OFF_CURVE;
  return g2_in_subgroup_fast(x, y) ? ZK_SOUND : ZK_OFF_SUBGROUP;
}

} // namespace p29
} // namespace bn254
