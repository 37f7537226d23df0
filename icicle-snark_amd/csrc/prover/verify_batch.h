// verify_batch.h — what the two batched Groth16 verifiers share and that needs HIP: the stages of a batch call in
// verify_batch.hip (argument checks, parse, per-item device stage), which groth16_verify_batch runs in a row and
// groth16_verify_batch_combined (verify_combined.hip) shares — the same parser, and the per-item stage as its fallback — and the
// device session both device stages work in.  The host-only pieces (parsed key and items, the prepared key, the combined sums) are
// in verify_host.h.
#pragma once
#include <chrono>
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/random.h>
#include <functional>
#include <vector>

#include "../common.h"
#include "verify_host.h"

namespace isnark {
namespace vb {

struct Parsed {                  // what the parse stage leaves: items[i] / pub[i·n_public + j] are valid where verdicts[i] == 0
  VbKey key;
  std::vector<VbItem> items;     // (pi_b not yet subgroup-checked)
  std::vector<bn254::fe> pub;
  std::vector<int> live;         // the indices the parser let through, ascending
};
int parse_one_device(const char* s);
// the argument checks every batch entry point starts with; *done: return the result at once (an error, or n = 0)
int batch_prologue(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, const char* device,
                   const int32_t* verdicts, int* dev, bool* done);
// vk and items (items on the worker pool, `meanwhile(key)` on the calling thread while they run): verdicts[i] = 0 for a live item,
// its negative code otherwise.  Non-zero: the key's error.  Sets the thread's parse time.
int parse_stage(const char* const* proof_jsons, const char* const* public_jsons, int n, const char* vk_json, int32_t* verdicts, Parsed* out,
                const std::function<void(const VbKey&)>& meanwhile);
// every live item through verify_batch_kernel in chunks (pk prepared from pz.key; its target is made here when it is not yet);
// adds its device time to the thread's
int per_item_stage(const Parsed& pz, PreparedKey& pk, int dev, int32_t* verdicts);
void set_last_timings(double parse_ms, double device_ms);
// the combined verifier's kernels (verify_combined.hip), enqueued on `st` for another caller — the mixed-key verifier:
//   combined_lane_kernel     lane i < m: f[i] = the Miller value of ([zᵢ](−Aᵢ), Bᵢ), ok[i] = 0 for a pi_b outside the subgroup
//   miller_strided_kernel    lane i < lanes: f[i] = Π of the Miller values of the pairs i, i + lanes, … below n; a pair with (0, 0) on
//                            either side contributes 1
//   the product passes       f[0] ← Π f[0 … n), n ≥ 1 (in place: the other slots are spent)
hipError_t enqueue_combined_lanes(const VbItem* items, const uint32_t* z, uint32_t m, bn254::p29::F12* f, uint8_t* ok, hipStream_t st);
hipError_t enqueue_miller_strided(const bn254::fe* p, const bn254::fe2* q, uint64_t n, uint32_t lanes, bn254::p29::F12* f, hipStream_t st);
hipError_t enqueue_product(bn254::p29::F12* f, uint32_t n, hipStream_t st);

// small helpers of the two device stages
using isnark::ms_since; // common.h
// the one text of a failed device call; the key tools' dev_fail (device_call.h) reports it through the prover's error channel
struct DeviceErrorText {
  char msg[200];
  DeviceErrorText(const char* what, hipError_t e) { snprintf(msg, sizeof msg, "device: %s: %s", what, hipGetErrorString(e)); }
};
// the batch verifiers' own: their return codes are ICICLE's
inline int device_fail(int code, const char* what, hipError_t e) { return fail(code, DeviceErrorText(what, e).msg); }
// n bytes from the operating system (getrandom, else /dev/urandom): the secret seeds of the randomised checks
inline bool os_random(uint8_t* out, size_t n)
{
  size_t got = 0;
  while (got < n) {
    const ssize_t r = getrandom(out + got, n - got, 0);
    if (r < 0) {
      if (errno == EINTR) continue;
      break;
    }
    got += (size_t)r;
  }
  if (got == n) return true;
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f) return false;
  const size_t rd = fread(out, 1, n, f);
  fclose(f);
  return rd == n;
}
struct DevBuf { // device allocations of one call, freed on every exit path
  std::vector<void*> ptrs;
  ~DevBuf() { free_all(); }
  void free_all()
  {
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
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

// One call's stay on a device: selects it through the library (icicle_set_device), takes one or two of the library's pooled
// streams — the MSM's workspace follows its stream's life, so the MSM must get a stream of the library's own — and owns the call's
// device buffers.  On every exit path the buffers are freed, the streams drained and handed back, and the calling thread gets back
// what it had: the library's default device, then its HIP device.
struct DeviceSession {
  int prev_hip = -1, prev_lib = -1;
  icicleStreamHandle streams[2] = {nullptr, nullptr};
  DevBuf buf;

  // 0, or the call's error code with its "device: …" message set
  int open(int dev, int n_streams)
  {
    (void)hipGetDevice(&prev_hip);
    prev_lib = default_device_or_none();
    const IcicleDevice want = hip_device(dev);
    if (icicle_set_device(&want) != ICICLE_SUCCESS) return fail((int)ICICLE_INVALID_DEVICE, "device: hipSetDevice: invalid device ordinal");
    for (int k = 0; k < n_streams; k++)
      if (icicle_create_stream(&streams[k]) != ICICLE_SUCCESS) return fail((int)ICICLE_UNKNOWN_ERROR, "device: stream creation failed");
    return 0;
  }
  hipStream_t stream(int k) const { return (hipStream_t)streams[k]; }
  ~DeviceSession()
  {
    buf.free_all();
    for (int k = 1; k >= 0; k--)
      if (streams[k]) (void)icicle_destroy_stream(streams[k]);
    if (prev_lib >= 0) {
      const IcicleDevice back = hip_device(prev_lib);
      (void)icicle_set_device(&back);
    }
    if (prev_hip >= 0) (void)hipSetDevice(prev_hip);
  }
  static IcicleDevice hip_device(int id)
  {
    IcicleDevice d;
    memset(&d, 0, sizeof d);
    strcpy(d.type, "HIP");
    d.id = id;
    return d;
  }
};

} // namespace vb
} // namespace isnark
