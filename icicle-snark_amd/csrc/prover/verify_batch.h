// verify_batch.h — host-side pieces of the batched Groth16 verifier (verify_batch.hip) that live in pairing.cpp: the JSON
// checks of groth16_verify_json, split into the verification key's (once per call) and each item's.
#pragma once
#include <stddef.h>
#include <vector>

#include "../ec.h"

namespace isnark {
namespace vb {

struct VbKey {                   // standard form, canonical; (0, 0) = identity
  bn254::fe alpha[2];
  bn254::fe2 beta[2], gamma[2], delta[2];
  std::vector<bn254::fe> ic;     // (n_public + 1) affine points, x then y
  size_t n_public = 0;
};
struct VbItem {                  // one proof's points, standard form, canonical, on their curves (pi_b not yet subgroup-checked)
  bn254::fe a[2];
  bn254::fe2 b[2];
  bn254::fe c[2];
};

// 0, or what groth16_verify_json returns for the same text (−2 format, −3 null); the message goes to
// groth16_verify_last_error() of the calling thread
int parse_vk(const char* vk_json, VbKey* out);
int parse_item(const char* proof_json, const char* public_json, size_t n_public, VbItem* item, bn254::fe* pub);
int fail(int code, const char* msg);

} // namespace vb
} // namespace isnark
