// zkey_pack29_check.cpp — host build of csrc/prover/zkey_pack29.h (the lane codec of a packed key's coefficient: the value code over
// the key's v·R² form).  Test infrastructure: compiled with g++ by tests/test_zkey_pack29.py and compared with
// tests/zkey_pack_model.py's Python integers.  The kernels of zkey_pack.hip compile the same text.
#include <stddef.h>
#include <stdint.h>

#include "../icicle-snark_amd/csrc/prover/zkey_pack29.h"

using namespace bn254;

// 32 little-endian bytes as section 4 stores them → the code and the payload (32 bytes, zero beyond the length); the length, −1 for
// a value not below r (code and payload untouched)
extern "C" int zp29_encode(const uint8_t* file, uint8_t* code, uint8_t* payload)
{
  fe f;
  wz::wz_load_words(file, 32, f.l);
  uint32_t pay[8];
  const int len = zp::zp_encode(f, code, pay);
  if (len >= 0) wz::wz_store_words(pay, 32, payload);
  return len;
}

// a code byte and its payload (len = the code's length, 0 for an undefined code) → the kind of fault (0: none) and the 32 file bytes
extern "C" int zp29_decode(uint8_t code, const uint8_t* payload, int len, uint8_t* file)
{
  if (wz::wz_code_len(code) < 0) {
    for (int i = 0; i < 32; i++) file[i] = 0;
    return wz::WZ_CODE; // (the kernel's lanes never hand an undefined code to the decoder's length rules)
  }
  uint32_t pay[8];
  wz::wz_load_words(payload, len, pay);
  fe f;
  const int kind = zp::zp_decode(code, pay, &f);
  wz::wz_store_words(f.l, 32, file);
  return kind;
}
