// verify_batch.h — host-side pieces of the batched Groth16 verifiers.  In pairing.cpp: the JSON checks of groth16_verify_json,
// split into the verification key's (once per call) and each item's.  In verify_batch.hip: the stages of a batch call (argument
// checks, parse, per-item device stage), which groth16_verify_batch runs in a row and groth16_verify_batch_combined
// (verify_combined.hip) shares: the same parser, and the per-item stage as its fallback.
#pragma once
#include <chrono>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <functional>
#include <vector>

#include "../ec29.h"

namespace bn254 {
namespace p29 {
struct VerifyKey29;
}
} // namespace bn254

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

struct Parsed {                  // what the parse stage leaves: items[i] / pub[i·n_public + j] are valid where verdicts[i] == 0
  VbKey key;
  std::vector<VbItem> items;
  std::vector<bn254::fe> pub;
  std::vector<int> live;         // the indices the parser let through, ascending
};
struct DeviceKey {               // the key as verify_batch_kernel reads it (p29::make_verify_key and the lazy form of IC)
  std::vector<bn254::p29::VerifyKey29> vk;
  std::vector<bn254::G1L::A> ic;
  std::vector<uint8_t> icz;
};
int parse_one_device(const char* s);
// the argument checks every batch entry point starts with; *done: return the result at once (an error, or n = 0)
int batch_prologue(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, const char* device,
                   const int32_t* verdicts, int* dev, bool* done);
// vk and items (items on the worker pool, `meanwhile(key)` on the calling thread while they run): verdicts[i] = 0 for a live item,
// its negative code otherwise.  Non-zero: the key's error.  Sets the thread's parse time.
int parse_stage(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, int32_t* verdicts, Parsed* out,
                const std::function<void(const VbKey&)>& meanwhile);
void make_device_key(const VbKey& key, DeviceKey* dk);
// every live item through verify_batch_kernel in chunks; adds its device time to the thread's
int per_item_stage(const Parsed& pz, const DeviceKey& dk, int dev, int32_t* verdicts);
void set_last_timings(double parse_ms, double device_ms);

// small helpers of the two device stages
inline double ms_since(std::chrono::steady_clock::time_point t0)
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
inline int device_fail(int code, const char* what, hipError_t e)
{
  char msg[200];
  snprintf(msg, sizeof msg, "device: %s: %s", what, hipGetErrorString(e));
  return fail(code, msg);
}
struct DevBuf { // device allocations of one call, freed on every exit path
  std::vector<void*> ptrs;
  ~DevBuf()
  {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <class T>
  T* alloc(size_t count)
  {
    void* p = nullptr;
    if (hipMalloc(&p, count * sizeof(T) + 16) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return (T*)p;
  }
};

} // namespace vb
} // namespace isnark
