// device_call.h — the host plumbing every key, file and pack tool wraps its device work in (the zkey_*.hip, ptau_*.hip, wtns_pack.hip,
// r1cs_check.hip; verify_combined.hip takes its MSM configuration from here): one error text and the checked call and launch that
// return it, the device a call names and the session it opens (open_session), stage times, the scoped file hint of the pinned
// staging, the timed upload, where an output goes once its size is known (Sink: the caller's buffer, or the temporary a _file entry
// writes and renames), the ONE _file entry of a tool that rewrites a file (rewrite_file), an event that destroys itself, the
// library's MSMs over device operands in slices, the seed and coefficients of the randomised checks, and the scalar tables of the
// ptau tools (root_of_unity, split_power_tables over ptau_contribute29.h's fill).  The device session and its buffers are
// verify_batch.h's; the host point helpers are verify_host.h's; a contribution's transcript is transcript.h's; the ptau's ranges and
// the lane test of an uploaded range are ptau_ranges.h's; the way back to the file's form is point_form.h's; what the packed forms'
// kernels share is pack_device.h's.
#pragma once
#include <algorithm>
#include <chrono>
#include <fcntl.h>
#include <functional>
#include <stdio.h>
#include <string.h>
#include <string>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../workers.h"
#include "prover_internal.h"
#include "ptau_contribute29.h"
#include "sha256.h"
#include "verify_batch.h"

namespace isnark {
namespace prover {

// ---- errors and status
inline int dev_fail(const char* what, hipError_t e) { return fail(ERR_DEVICE, "%s", vb::DeviceErrorText(what, e).msg); }
// return "device: <what>: <HIP's text>" from the calling function when a HIP call fails
#define DEV_TRY(what, call)                                                      \
  do {                                                                           \
    if (hipError_t he__ = (call)) return ::isnark::prover::dev_fail(what, he__); \
  } while (0)
// launch (no dynamic LDS) and test the launch the same way; a kernel with template arguments goes in parentheses
#define DEV_LAUNCH(what, kernel, grid, block, stream, ...)                \
  do {                                                                    \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);      \
    DEV_TRY(what, hipGetLastError());                                     \
  } while (0)

// the one HIP device a call names
inline int parse_device(const char* device, int* dev)
{
  if (!device) return fail(ERR_ARG, "null device");
  *dev = vb::parse_one_device(device);
  if (*dev < 0) return fail(ERR_ARG, "device: '%s' does not name one HIP device", device);
  return 0;
}
// the session of a call: `dev` made active, `streams` streams
inline int open_session(vb::DeviceSession& ds, int dev, int streams) { return ds.open(dev, streams) ? fail(ERR_DEVICE, "%s", groth16_verify_last_error()) : 0; }

// stage times on stderr when `env` is set (read at every call: common.h's rule for a knob an in-process caller may change), as
// ICICLE_SNARK_TRACE_COLD for a load
struct StageTrace {
  const char* const tag;
  const bool on;
  std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
  StageTrace(const char* tag_, const char* env) : tag(tag_), on(env_set(env)) {}
  void lap(const char* what)
  {
    if (!on) return;
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[%s] %-28s %8.2f ms\n", tag, what, std::chrono::duration<double, std::milli>(t - prev).count());
    prev = t;
  }
};

// ---- uploads
// A mapped file a call reads its input from (fd < 0: plain memory).
struct FileRange {
  const uint8_t* base = nullptr;
  size_t len = 0;
  int fd = -1;
  bool holds(const void* p) const { return fd >= 0 && (const uint8_t*)p >= base && (const uint8_t*)p < base + len; }
};
// While one lives, the calling thread's staged copies pread() the file instead of copying out of its mapping; the hint is cleared
// on every way out of the scope, so none is left for the thread's next call.
struct FileHint {
  FileHint(const void* base, size_t len, int fd)
  {
    if (fd >= 0) staged_copy_file_hint(base, len, fd);
  }
  explicit FileHint(const FileRange& f) : FileHint(f.base, f.len, f.fd) {}
  ~FileHint() { staged_copy_file_hint(nullptr, 0, -1); }
  FileHint(const FileHint&) = delete;
  FileHint& operator=(const FileHint&) = delete;
};
// one range up through the pinned staging (it has landed on return), its wall time added to *ms; nothing for an empty range
inline int timed_upload(int dev, void* dst, const void* src, size_t bytes, double* ms)
{
  if (!bytes) return 0;
  const auto t0 = std::chrono::steady_clock::now();
  const CopyJob job = {dst, src, bytes};
  const hipError_t he = staged_copy(dev, &job, 1, true);
  *ms += ms_since(t0);
  return he ? dev_fail("host to device upload", he) : 0;
}

// ---- outputs
// a file written as a temporary beside `path` and renamed over it by finish(0): a failed call leaves nothing there
struct TempOutput {
  std::string path, tmp;
  int fd = -1;
  uint8_t* map = nullptr;
  uint64_t map_len = 0;
  explicit TempOutput(const char* out_path) : path(out_path), tmp(std::string(out_path) + ".tmp." + std::to_string((long)getpid())) {}
  int open(uint64_t bytes, uint8_t** o)
  {
    fd = ::open(tmp.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(ERR_IO, "cannot create %s", tmp.c_str());
    if (ftruncate(fd, (off_t)bytes) != 0) return fail(ERR_IO, "cannot size %s to %llu bytes", tmp.c_str(), (unsigned long long)bytes);
    void* p = mmap(nullptr, (size_t)bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (p == MAP_FAILED) return fail(ERR_IO, "cannot mmap %s", tmp.c_str());
    map = (uint8_t*)p;
    map_len = bytes;
    *o = map;
    return 0;
  }
  // rc: the call's result so far; returns the call's result
  int finish(int rc)
  {
    if (map) {
      if (rc == 0 && msync(map, (size_t)map_len, MS_SYNC) != 0) rc = fail(ERR_IO, "cannot write %s", tmp.c_str());
      munmap(map, (size_t)map_len);
    }
    if (fd >= 0) close(fd);
    if (rc == 0 && rename(tmp.c_str(), path.c_str()) != 0) rc = fail(ERR_IO, "cannot rename %s to %s", tmp.c_str(), path.c_str());
    if (rc != 0 && fd >= 0) (void)unlink(tmp.c_str());
    return rc;
  }
};

// where a call's output goes, asked once its size is known and before anything is written
typedef std::function<int(uint64_t bytes, uint8_t** out)> Sink;
// the caller's buffer of `cap` bytes; `noun` is what the text calls the output
inline Sink buffer_sink(const char* noun, void* out, size_t cap)
{
  return [noun, out, cap](uint64_t bytes, uint8_t** o) {
    if (!out || cap < bytes)
      return fail(ERR_ARG, "the %s needs %llu bytes, the buffer holds %llu", noun, (unsigned long long)bytes, (unsigned long long)(out ? cap : 0));
    *o = (uint8_t*)out;
    return 0;
  };
}
// A _file entry that rewrites in_path as out_path: the paths are judged (null, the same, the same file under two names), the input
// is mapped and hinted to the staging workers (they pread() the file instead of copying out of the mapping), `impl` runs over the
// image with a sink that opens a TempOutput, and the temporary is renamed or unlinked.  *write_ms (may be null): msync and rename.
inline int rewrite_file(const char* in_path, const char* out_path, double* write_ms, const std::function<int(const uint8_t* data, size_t len, const Sink& sink)>& impl)
{
  if (!in_path || !out_path) return fail(ERR_ARG, "null path");
  if (strcmp(in_path, out_path) == 0) return fail(ERR_ARG, "the output path is the input's");
  MappedFile mf;
  if (int rc = mf.open_ro(in_path)) return rc;
  struct stat a, b;
  if (stat(out_path, &b) == 0 && fstat(mf.fd, &a) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino) return fail(ERR_ARG, "the output path is the input's");
  const FileHint hint(mf.data, mf.len, mf.fd);
  TempOutput to(out_path);
  int rc = impl(mf.data, mf.len, [&](uint64_t bytes, uint8_t** o) { return to.open(bytes, o); });
  const auto t_write = std::chrono::steady_clock::now();
  rc = to.finish(rc);
  if (rc == 0 && write_ms) *write_ms = ms_since(t_write);
  return rc;
}

struct Event { // ordering only: no timing
  hipEvent_t e = nullptr;
  int create()
  {
    DEV_TRY("hipEventCreate", hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
  }
  ~Event()
  {
    if (e) (void)hipEventDestroy(e);
  }
};

// ---- the library's MSMs
constexpr uint32_t MSM_SLICE = 1u << 24; // bases per MSM call (partial sums add)
inline MSMConfig msm_config(icicleStreamHandle stream, int bitsize) // host operands
{
  MSMConfig mc;
  memset(&mc, 0, sizeof mc);
  mc.stream = stream;
  mc.precompute_factor = 1;
  mc.bitsize = bitsize;
  mc.batch_size = 1;
  return mc;
}
inline MSMConfig device_msm_config(icicleStreamHandle stream, int bitsize) // scalars and Montgomery-form affine bases on the device
{
  MSMConfig mc = msm_config(stream, bitsize);
  mc.are_scalars_on_device = true;
  mc.are_points_on_device = true;
  mc.are_points_montgomery_form = true;
  return mc;
}
// Σ scalars[i]·bases[i] over `count` bases in slices of MSM_SLICE; count = 0 is the identity.  The group is out's.
template <class A, class P>
int sliced_msm_of(eIcicleError (*msm)(const bn254_scalar_t*, const A*, int, const MSMConfig*, P*), void (*add)(const P*, const P*, P*), const MSMConfig& mc,
                  const void* scalars, const void* bases, uint64_t count, P* out)
{
  memset(out, 0, sizeof *out);
  for (uint64_t off = 0; off < count; off += MSM_SLICE) {
    const int cnt = (int)std::min<uint64_t>(MSM_SLICE, count - off);
    P p;
    if (eIcicleError me = msm((const bn254_scalar_t*)scalars + off, (const A*)bases + off, cnt, &mc, &p))
      return fail(ERR_DEVICE, "device: msm (%d): %s", (int)me, icicle_snark_last_error());
    if (off) add(out, &p, out);
    else *out = p;
  }
  return 0;
}
inline int sliced_msm(const MSMConfig& mc, const void* scalars, const void* bases, uint64_t count, bn254_projective_t* out)
{
  return sliced_msm_of<bn254_affine_t>(bn254_msm, bn254_ecadd, mc, scalars, bases, count, out);
}
inline int sliced_msm(const MSMConfig& mc, const void* scalars, const void* bases, uint64_t count, bn254_g2_projective_t* out)
{
  return sliced_msm_of<bn254_g2_affine_t>(bn254_g2_msm, bn254_g2_ecadd, mc, scalars, bases, count, out);
}

// ---- the randomised checks' secrets
// the caller's 32 bytes, or the operating system's
inline int seed_or_random(const uint8_t* seed32, uint8_t out[32])
{
  if (seed32) memcpy(out, seed32, 32);
  else if (!vb::os_random(out, 32)) return fail(ERR_ARG, "no randomness from the operating system (getrandom, /dev/urandom)");
  return 0;
}
// out[i] = the combined verifier's coefficient first + i of `seed` (sha256.h): 128 bits in 32-byte standard form, on the worker pool;
// `meanwhile` (may be empty) runs on the calling thread while the pool works
inline void fill_coefficients(const uint8_t seed[32], uint64_t first, size_t count, fe* out, const std::function<void()>& meanwhile = nullptr)
{
  memset(out, 0, count * sizeof out[0]);
  run_ranges(count, 4096, [&](int, size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) combined_coefficient(seed, first + (uint64_t)i, (uint8_t*)&out[i]);
  }, meanwhile);
}


// ---- the ptau tools' scalar tables
// the root of unity of order 2^order_log2, standard form
inline int root_of_unity(uint32_t order_log2, fe* w_std)
{
  bn254_scalar_t rou;
  if (bn254_get_root_of_unity((uint64_t)1 << order_log2, &rou) != ICICLE_SUCCESS) return fail(ERR_ARG, "ptau: no root of unity of order 2^%u", order_log2);
  memcpy(w_std->l, &rou, 32);
  return 0;
}
// The two-table split of a power sequence (ptau_contribute29.h: index i = m·2^kbits + j), into the caller's 2^kbits + n_starts·n_hi
// entries at `out`: lo[j] = base^j for j < 2^kbits, then for each start c hi_c[m] = start_c·base^(m·2^kbits) for m < n_hi.
// Montgomery form in and out, filled on the worker pool; nothing is allocated, so a caller's secrets stay in its own storage.
inline void split_power_tables(const fe& base_m, uint32_t kbits, size_t n_hi, const fe* starts_m, int n_starts, fe* out)
{
  const size_t n_lo = (size_t)1 << kbits;
  const fe one_m = Fr::to_mont(Fr::one_std()), step_m = bn254::pc29::pc_pow(base_m, n_lo);
  run_ranges(n_lo, 1024, [&](int, size_t lo, size_t hi) { bn254::pc29::pc_fill_powers(base_m, one_m, lo, hi, out); });
  for (int c = 0; c < n_starts; c++) {
    fe* const hi_c = out + n_lo + (size_t)c * n_hi;
    run_ranges(n_hi, 1024, [&](int, size_t lo, size_t hi) { bn254::pc29::pc_fill_powers(step_m, starts_m[c], lo, hi, hi_c); });
  }
}

} // namespace prover
} // namespace isnark
