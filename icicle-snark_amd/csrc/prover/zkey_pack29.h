// zkey_pack29.h — the PACKED form of a proving key's coefficient ("zkez", version 1, section 4): the wtnz value code over the key's
// own v·R² form, host and device from one text.  The pack and unpack kernels of groth16_zkey_pack / _unpack / _coefs_pack /
// _coefs_unpack and of the packed load (zkey_pack.hip) and the stand-alone host check (tests/zkey_pack29_check.cpp) compile this
// text.  include/groth16_prover.h has the container; wtns_pack.h the value code; DESIGN.md §7l.
//
// THE VALUE.  Section 4 of a .zkey stores a coefficient as file = v·R² mod r, R = 2^256, 32 bytes little-endian (csr.hip: one
// from_mont leaves v·R, the Montgomery form the prover multiplies with; a second one leaves v).  The value CODED is the standard-form
// coefficient v = file·R⁻² mod r — in a real key almost always 1 or r − 1 — by wtns_pack.h's rules 1 … 4, unchanged: zero, one,
// the negated form where it is shorter, else the positive form.
//
// THE BIJECTION.  Packing demands file < r (a value not below r is the fault RANGE: Montgomery multiplication is defined on
// residues below r only, and a .zkey holds nothing else).  v ↦ v·R² mod r is a bijection on [0, r) and so is its inverse, and the
// value code is a bijection between [0, r) and its valid (code, payload) pairs: pack and unpack are inverse byte for byte.
//
//   zp_encode (file, &code, pay)   −1: file is not below r (nothing written).  Else the payload's length, the code, and the payload
//                                  as eight little-endian words, the bytes beyond the length ZERO.
//   zp_decode (code, pay, &file)   wz_decode_value's verdict (WZ_OK, or CODE / NONCANONICAL / RANGE and file all zero); on WZ_OK
//                                  file = v·R² mod r.  `code` is defined (wz_code_len >= 0) and pay is zero beyond its length.
#pragma once
#include "../ff.h"
#include "wtns_pack.h"

namespace bn254 {
namespace zp {

constexpr uint32_t ZP_RECORD_BYTES = 12 + 32, ZP_RECORD_WORDS = 11; // {m:u32 c:u32 s:u32 value[32]}, prover_internal.h's COEF_RECORD_BYTES
constexpr uint32_t ZP_BLOCK = wz::WZ_BLOCK;                         // records a block, a lane each
constexpr uint32_t ZP_BLOCK_BYTES = ZP_BLOCK * ZP_RECORD_BYTES;     // 11264, a multiple of 16

WZ_HD int zp_encode(const fe& file, uint8_t* code, uint32_t pay[8])
{
  if (!wz::wz_below_r(file.l)) return -1;
  const fe v = Fr::from_mont(Fr::from_mont(file)); // canonical: below r
  for (int i = 0; i < 8; i++) pay[i] = 0;
  const int nv = wz::wz_bytes(v.l);
  if (nv == 0) {
    *code = wz::WZ_CODE_ZERO;
    return 0;
  }
  if (nv == 1 && v.l[0] == 1) {
    *code = wz::WZ_CODE_ONE;
    return 0;
  }
  uint32_t m[8];
  wz::wz_r_minus(v.l, m);
  const int nm = wz::wz_bytes(m);
  const bool neg = nm < nv;
  for (int i = 0; i < 8; i++) pay[i] = neg ? m[i] : v.l[i];
  *code = neg ? (uint8_t)(wz::WZ_NEG | nm) : (uint8_t)nv;
  return neg ? nm : nv;
}

WZ_HD int zp_decode(uint8_t code, const uint32_t pay[8], fe* file)
{
  fe v;
  const int kind = wz::wz_decode_value(code, pay, v.l);
  *file = v; // all zero on a fault
  if (kind == wz::WZ_OK) *file = Fr::to_mont(Fr::to_mont(v));
  return kind;
}

} // namespace zp
} // namespace bn254
