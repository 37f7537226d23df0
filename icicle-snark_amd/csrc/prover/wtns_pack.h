// wtns_pack.h — the PACKED form of a witness ("wtnz", version 1): a code byte per value and only the value's significant bytes,
// host and device from one text.  groth16_wtns_pack / _unpack_host (wtns_pack.hip, host only), the decode kernel of
// groth16_wtns_unpack, groth16_prove_packed and groth16_witness_check_packed (wz_unpack_kernel, wtns_pack.hip), the container
// reader (wtnz_layout, containers.cpp) and the stand-alone host check (tests/wtns_pack_check.cpp) compile this text.  DESIGN.md §7k.
//
// THE VALUE.  v is an element of Fr in standard form, 0 ≤ v < r, 32 bytes little-endian as a .wtns stores it.  bytes(x) = the number
// of significant bytes of x, bytes(0) = 0.  The first rule that applies:
//      1  v = 0                               code 0x00          no payload
//      2  v = 1                               code 0x40          no payload
//      3  m = r − v, bytes(m) < bytes(v)      code 0x80 | bytes(m)   (0x81 … 0x9f)   payload m, bytes(m) bytes little-endian
//      4  otherwise                           code bytes(v)          (0x01 … 0x20)   payload v, bytes(v) bytes little-endian
// Every other code byte is undefined.  The encoding is unique: pack and unpack are inverse bijections.
//
// THE FAULTS of a decoder (wz_decode_value; the kinds are include/groth16_prover.h's GROTH16_WTNZ_*):
//      CODE          an undefined code byte (its length counts as 0 in a block's sum)
//      NONCANONICAL  a payload whose top byte is 0; code 0x01 with payload 01 (rule 2's value); a positive form of 32 bytes whose
//                    negated form would be shorter: v > r − 2^248.  (Below 32 bytes no positive form has a shorter negation:
//                    r − v > r − 2^248 has 32 bytes.  A negated form's value r − m ≥ r − 2^248 + 1 always has 32 bytes > bytes(m).)
//      RANGE         32 bytes that are not below r — tested before the rule above, which needs r − v
//      DIRECTORY     a block's 256 lengths do not sum to its directory span; named at the block's first element, and the ONLY
//                    fault such a block reports: without the sum no lane knows where its payload begins
//
// THE BOUNDS.  A block is WZ_BLOCK = 256 consecutive values, its payload at most WZ_MAX_SPAN = 256 · 32 bytes.  wz_check_directory
// (host) demands entry 0 = 0, no entry below its predecessor, no span above WZ_MAX_SPAN and the last entry = the payload's size —
// with that, block b's payload [dir[b], dir[b + 1]) lies inside section 4 whatever the codes say, and a lane whose block's lengths
// sum to the span reads [off, off + len) inside it.  A block whose sum differs reads nothing.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WZ_HD __host__ __device__ inline
#else
#define WZ_HD inline
#endif

namespace bn254 {
namespace wz {

constexpr uint32_t WZ_BLOCK = 256, WZ_MAX_SPAN = WZ_BLOCK * 32;
constexpr uint8_t WZ_CODE_ZERO = 0x00, WZ_CODE_ONE = 0x40, WZ_NEG = 0x80;
enum { WZ_OK = 0, WZ_CODE = 1, WZ_NONCANONICAL = 2, WZ_RANGE = 3, WZ_DIRECTORY = 4 };

// r of BN254, little-endian words (a switch, not a table: the same text serves host and device without a constant object)
WZ_HD uint32_t wz_r(int i)
{
  switch (i) {
  case 0: return 0xf0000001u;
  case 1: return 0x43e1f593u;
  case 2: return 0x79b97091u;
  case 3: return 0x2833e848u;
  case 4: return 0x8181585du;
  case 5: return 0xb85045b6u;
  case 6: return 0xe131a029u;
  default: return 0x30644e72u;
  }
}

// payload bytes of a code; −1: undefined
WZ_HD int wz_code_len(uint8_t c)
{
  if (c == WZ_CODE_ZERO || c == WZ_CODE_ONE) return 0;
  if (c >= 0x01 && c <= 0x20) return c;
  if (c >= 0x81 && c <= 0x9f) return c & 0x7f;
  return -1;
}

WZ_HD bool wz_below_r(const uint32_t w[8])
{
  for (int i = 7; i >= 0; i--) {
    if (w[i] < wz_r(i)) return true;
    if (w[i] > wz_r(i)) return false;
  }
  return false;
}

// out = r − w for 0 ≤ w ≤ r
WZ_HD void wz_r_minus(const uint32_t w[8], uint32_t out[8])
{
  uint32_t borrow = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)wz_r(i) - w[i] - borrow;
    out[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
}

// significant bytes of a 256-bit little-endian word array
WZ_HD int wz_bytes(const uint32_t w[8])
{
  for (int i = 7; i >= 0; i--)
    if (w[i]) return 4 * i + (w[i] >> 24 ? 4 : w[i] >> 16 ? 3 : w[i] >> 8 ? 2 : 1);
  return 0;
}

// One value: `code` (defined: wz_code_len >= 0) and its payload as eight little-endian words, the bytes beyond the code's length
// ZERO.  WZ_OK and the standard-form value in out, or the kind of fault and out all zero.
WZ_HD int wz_decode_value(uint8_t code, const uint32_t pay[8], uint32_t out[8])
{
  for (int i = 0; i < 8; i++) out[i] = 0;
  if (code == WZ_CODE_ZERO) return WZ_OK;
  if (code == WZ_CODE_ONE) {
    out[0] = 1;
    return WZ_OK;
  }
  const int len = wz_code_len(code);
  if (len < 0) return WZ_CODE;
  // the top byte: a shorter payload would have said the same
  if (((pay[(len - 1) >> 2] >> (8 * ((len - 1) & 3))) & 0xff) == 0) return WZ_NONCANONICAL;
  if (code & WZ_NEG) {
    wz_r_minus(pay, out); // 0 < m < 2^248 < r
    return WZ_OK;
  }
  if (len == 1 && pay[0] == 1) return WZ_NONCANONICAL; // rule 2's value
  if (len == 32) {
    if (!wz_below_r(pay)) return WZ_RANGE;
    uint32_t m[8];
    wz_r_minus(pay, m);
    if (wz_bytes(m) < 32) return WZ_NONCANONICAL; // rule 3's value
  }
  for (int i = 0; i < 8; i++) out[i] = pay[i];
  return WZ_OK;
}

// ---- host only from here ------------------------------------------------------------------------------------------------------
inline const char* wz_fault_text(int kind) // of WZ_CODE … WZ_DIRECTORY, as the messages name them
{
  static const char* const text[5] = {"", "an undefined code byte", "the value's form is not canonical", "32 bytes that are not below r", "the block's lengths do not sum to its directory span"};
  return text[kind >= 0 && kind < 5 ? kind : 0];
}
inline void wz_load_words(const uint8_t* bytes, int len, uint32_t w[8]) // len ≤ 32 little-endian bytes, zero-extended
{
  uint8_t b[32] = {0};
  memcpy(b, bytes, (size_t)len);
  for (int i = 0; i < 8; i++) w[i] = (uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 | (uint32_t)b[4 * i + 3] << 24;
}
inline void wz_store_words(const uint32_t w[8], int len, uint8_t* bytes)
{
  for (int k = 0; k < len; k++) bytes[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}

// the host encoder: 32 bytes of a .wtns → the code and the payload (room for 32 bytes); the payload's length, or −1 for a value >= r
inline int wz_encode_value(const uint8_t value[32], uint8_t* code, uint8_t* payload)
{
  uint32_t v[8], m[8];
  wz_load_words(value, 32, v);
  if (!wz_below_r(v)) return -1;
  const int nv = wz_bytes(v);
  if (nv == 0) {
    *code = WZ_CODE_ZERO;
    return 0;
  }
  if (nv == 1 && v[0] == 1) {
    *code = WZ_CODE_ONE;
    return 0;
  }
  wz_r_minus(v, m);
  const int nm = wz_bytes(m);
  if (nm < nv) {
    *code = (uint8_t)(WZ_NEG | nm);
    wz_store_words(m, nm, payload);
    return nm;
  }
  *code = (uint8_t)nv;
  wz_store_words(v, nv, payload);
  return nv;
}

// The directory of n_blocks + 1 little-endian u64 values (unaligned) against the payload's size.  0, or the rule broken:
// 1 entry 0 is not 0 · 2 entry *at is below its predecessor · 3 block *at spans more than WZ_MAX_SPAN · 4 the last entry is not
// payload_bytes.  The first broken rule in this order of entries.
inline uint64_t wz_dir_entry(const uint8_t* dir, uint64_t i)
{
  uint64_t v;
  memcpy(&v, dir + 8 * i, 8);
  return v;
}
inline int wz_check_directory(const uint8_t* dir, uint64_t n_blocks, uint64_t payload_bytes, uint64_t* at)
{
  *at = 0;
  if (wz_dir_entry(dir, 0) != 0) return 1;
  for (uint64_t b = 0; b < n_blocks; b++) {
    const uint64_t lo = wz_dir_entry(dir, b), hi = wz_dir_entry(dir, b + 1);
    if (hi < lo) {
      *at = b + 1;
      return 2;
    }
    if (hi - lo > WZ_MAX_SPAN) {
      *at = b;
      return 3;
    }
  }
  *at = n_blocks;
  return wz_dir_entry(dir, n_blocks) == payload_bytes ? 0 : 4;
}

// A packed witness whose container and directory have passed (wtnz_layout): decode values [first, first + count) to out (32 bytes
// each) on the host.  WZ_OK, or the kind of the LOWEST faulty element of the blocks touched and *element its index; a faulty
// element's row is zero.  *faults (may be null) counts them.
struct WzView {
  uint32_t n = 0;
  const uint8_t *codes = nullptr, *dir = nullptr, *payload = nullptr;
};
inline int wz_decode_host(const WzView& z, uint64_t first, uint64_t count, uint8_t* out, uint64_t* element, uint64_t* faults)
{
  int kind = WZ_OK;
  uint64_t n_faults = 0;
  auto fault = [&](uint64_t e, int k) {
    if (!n_faults) kind = k, *element = e;
    n_faults++;
  };
  const uint64_t end = first + count;
  for (uint64_t b = first / WZ_BLOCK; b * WZ_BLOCK < end; b++) {
    const uint64_t e0 = b * WZ_BLOCK, e1 = e0 + WZ_BLOCK < z.n ? e0 + WZ_BLOCK : z.n;
    const uint64_t lo = wz_dir_entry(z.dir, b), span = wz_dir_entry(z.dir, b + 1) - lo;
    uint64_t sum = 0;
    for (uint64_t e = e0; e < e1; e++) {
      const int len = wz_code_len(z.codes[e]);
      sum += len > 0 ? (uint64_t)len : 0;
    }
    const bool dir_ok = sum == span;
    if (!dir_ok) fault(e0, WZ_DIRECTORY);
    uint64_t off = lo;
    for (uint64_t e = e0; e < e1; e++) {
      const int len = wz_code_len(z.codes[e]);
      if (e >= first && e < end) {
        uint32_t pay[8], v[8] = {0};
        if (dir_ok) {
          wz_load_words(z.payload + off, len > 0 ? len : 0, pay);
          if (const int k = wz_decode_value(z.codes[e], pay, v)) fault(e, k);
        }
        wz_store_words(v, 32, out + 32 * (e - first));
      }
      off += len > 0 ? (uint64_t)len : 0;
    }
  }
  if (faults) *faults = n_faults;
  return kind;
}

} // namespace wz
} // namespace bn254
