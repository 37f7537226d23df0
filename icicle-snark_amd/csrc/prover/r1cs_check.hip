// r1cs_check.hip — an .r1cs kept on one device, and groth16_witness_check over it  (include/groth16_prover.h has the contract;
// DESIGN.md §7c)
//
//   load     r1cs_layout + r1cs_walk (containers.cpp) on the host: every record bounded, rowptr[3m + 1] in terms.  Section 2 goes up
//            raw, in slices through the library's pinned staging (staged_copy, which returns when a slice has landed); behind each
//            slice r1cs_fill_kernel unpacks the rows that are complete by then — one lane per row — from the 4-byte-aligned 36-byte
//            records into cols[t] and 32-byte-aligned Montgomery vals[t], after wire < nWires and value < r.  A faulting lane takes
//            the minimum of (row << 1 | kind): the lowest constraint, within it A before B before C, and nothing per record comes
//            back.  The raw payload is freed; the handle keeps rowptr, cols, vals, a witness buffer, a tally block and a stream.
//   check    the witness goes up; witness_range_kernel (one lane per wire: value < r, wire 0 = 1), then — only over canonical
//            values — r1cs_constraint_kernel, one lane per constraint through r1cs_check.h.  A failing lane alone adds 1 to the
//            count and takes the minimum of the index.  Only the tally block comes back.
//   match    groth16_r1cs_match_zkey: a secret vector z takes the witness's place.  The constraint kernel in its emit mode writes
//            a_j = A_j·z and b_j = B_j·z; the zkey's section 4 goes through the prover's own qap_build_csr and qap_spmv with the
//            same z; r1cs_compare_kernel (one lane per row of the domain) compares, public-binding rows included.
//   verify   groth16_zkey_verify_ptau (zkey_verify.hip) takes the rows a, b AND c at vectors of its own: the kernel's third mode,
//            through r1cs_emit_abc.
#include <algorithm>
#include <chrono>
#include <memory>
#include <mutex>
#include <vector>

#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "r1cs_check.h"
#include "sha256.h"
#include "verify_batch.h"

using namespace bn254;

namespace {

namespace pv = isnark::prover;

constexpr size_t SLICE_BYTES = 64u << 20;      // section 2 per upload slice
constexpr unsigned long long NONE = ~0ull;

struct Tally {
  unsigned long long bad_record;               // load: min of (row << 1 | kind), kind 0 wire id, 1 coefficient
  unsigned long long noncanonical, first_noncanonical, not_one;
  unsigned long long failed, first_failed;
  unsigned long long rows_a, first_a, rows_b, first_b; // match: rows of the key's A / B that differ from the circuit's
};

// rows [row_lo, row_hi) of the raw payload (32-bit words): term t of row ρ starts at word 9·t + ρ + 1 — behind the ρ + 1 count
// words of the rows up to it.  The host walk has bounded all of these reads; this kernel bounds the wire ids and the values.
__global__ __launch_bounds__(256) void r1cs_fill_kernel(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ rowptr, uint32_t row_lo, uint32_t row_hi, uint32_t n_wires,
                                                         uint32_t* __restrict__ cols, fe* __restrict__ vals, Tally* __restrict__ t)
{
  const uint64_t r64 = (uint64_t)row_lo + (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r64 >= row_hi) return;
  const uint32_t row = (uint32_t)r64;
  uint32_t k = rowptr[row];
  const uint32_t h = rowptr[row + 1];
  const uint32_t* e = raw + (size_t)9 * k + row + 1;
  for (; k < h; k++, e += 9) {
    const uint32_t wire = e[0];
    fe v;
#pragma unroll
    for (int i = 0; i < 8; i++) v.l[i] = e[1 + i];
    const bool wire_ok = wire < n_wires;
    if (!wire_ok || !Fr::is_canonical(v)) {
      atomicMin(&t->bad_record, (unsigned long long)row << 1 | (wire_ok ? 1ull : 0ull));
      return;
    }
    cols[k] = wire;
    st(vals + k, Fr::to_mont(v));
  }
}

__global__ __launch_bounds__(256) void witness_range_kernel(const fe* __restrict__ w, uint32_t n_wires, Tally* __restrict__ t)
{
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_wires) return;
  const fe v = w[i];
  if (!isnark::r1cs_value_in_range(v)) {
    atomicAdd(&t->noncanonical, 1ull);
    atomicMin(&t->first_noncanonical, (unsigned long long)i);
  }
  if (i == 0 && !Fr::eq(v, Fr::one_std())) t->not_one = 1;
}

// MODE 0: a verdict.  MODE 1 (match): a_j to ab[j] and b_j to ab[m + j] instead.  MODE 2 (zkey verify): as 1, and c_j to ab[2m + j]
template <int MODE>
__global__ __launch_bounds__(256) void r1cs_constraint_kernel(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ cols, const fe* __restrict__ vals,
                                                               const fe* __restrict__ w, uint32_t m, Tally* __restrict__ t, fe* __restrict__ ab)
{
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const isnark::R1csRows r = isnark::r1cs_eval(rowptr, cols, vals, w, j);
  if (MODE) {
    st(ab + j, r.a);
    st(ab + (size_t)m + j, r.b);
    if (MODE == 2) st(ab + 2 * (size_t)m + j, r.c);
  } else if (!isnark::r1cs_holds(r)) {
    atomicAdd(&t->failed, 1ull);
    atomicMin(&t->first_failed, (unsigned long long)j);
  }
}

// row j < n of the key's [B | A | ·] (qap_spmv's layout) at z against the circuit's: A_j = a_j below m, z_{j − m} on the
// public-binding rows m … m + n_public (snarkjs adds them to A alone), 0 above; B_j = b_j below m, 0 above
__global__ __launch_bounds__(256) void r1cs_compare_kernel(const fe* __restrict__ vec, const fe* __restrict__ ab, const fe* __restrict__ z, uint32_t n, uint32_t m,
                                                            uint32_t n_public, Tally* __restrict__ t)
{
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const fe want_a = j < m ? ab[j] : j - m <= n_public ? z[j - m] : Fr::zero();
  const fe want_b = j < m ? ab[(size_t)m + j] : Fr::zero();
  if (!Fr::eq(vec[(size_t)n + j], want_a)) {
    atomicAdd(&t->rows_a, 1ull);
    atomicMin(&t->first_a, (unsigned long long)j);
  }
  if (!Fr::eq(vec[j], want_b)) {
    atomicAdd(&t->rows_b, 1ull);
    atomicMin(&t->first_b, (unsigned long long)j);
  }
}

using pv::dev_fail;

} // namespace

struct Groth16R1cs {
  int dev = 0;
  uint32_t n_wires = 0, n_public = 0, m = 0;
  uint64_t n_terms = 0;
  uint32_t *d_rowptr = nullptr, *d_cols = nullptr;
  fe *d_vals = nullptr, *d_w = nullptr;
  Tally* d_tally = nullptr;
  hipStream_t st = nullptr;
  Groth16R1csInfo info = {};
  std::mutex mu; // one call at a time: the witness buffer and the tally block are the handle's
  ~Groth16R1cs()
  {
    if (st) (void)hipStreamSynchronize(st);
    for (void* p : {(void*)d_rowptr, (void*)d_cols, (void*)d_vals, (void*)d_w, (void*)d_tally})
      if (p) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
  }
};

namespace {

int reset_tally(Groth16R1cs* h)
{
  const Tally z = {NONE, 0, NONE, 0, 0, NONE, 0, NONE, 0, NONE};
  DEV_TRY("upload", hipMemcpyAsync(h->d_tally, &z, sizeof z, hipMemcpyHostToDevice, h->st));
  DEV_TRY("upload", hipStreamSynchronize(h->st)); // (`z` is pageable: the copy has read it)
  return 0;
}
int read_tally(Groth16R1cs* h, Tally* out, const char* what)
{
  DEV_TRY("download", hipMemcpyAsync(out, h->d_tally, sizeof *out, hipMemcpyDeviceToHost, h->st));
  DEV_TRY(what, hipStreamSynchronize(h->st));
  return 0;
}

template <class T>
int dev_alloc(T** p, size_t count, uint64_t* total)
{
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  DEV_TRY("hipMalloc", hipMalloc((void**)p, bytes));
  *total += bytes;
  return 0;
}

int r1cs_load_impl(const uint8_t* data, size_t len, const char* device, Groth16R1cs** out)
{
  if (!out) return pv::fail(pv::ERR_ARG, "null handle pointer");
  *out = nullptr;
  int dev;
  if (int rc = pv::parse_device(device, &dev)) return rc;
  pv::R1csLayout L;
  if (int rc = pv::r1cs_layout(data, len, &L)) return rc;
  std::vector<uint32_t> rowptr;
  uint64_t n_terms = 0;
  const auto t_walk = std::chrono::steady_clock::now();
  if (int rc = pv::r1cs_walk(L, rowptr, &n_terms)) return rc;
  const double walk_ms = pv::ms_since(t_walk);

  const auto t_dev = std::chrono::steady_clock::now();
  isnark::vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, dev, 0)) return rc;
  std::unique_ptr<Groth16R1cs> h(new Groth16R1cs); // (destroyed before the session: declared after it)
  h->dev = dev;
  h->n_wires = L.n_wires;
  h->n_public = L.n_public();
  h->m = L.n_constraints;
  h->n_terms = n_terms;
  const uint32_t rows = 3 * L.n_constraints;
  uint64_t bytes = 0;
  DEV_TRY("hipStreamCreate", hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
  if (int rc = dev_alloc(&h->d_rowptr, (size_t)rows + 1, &bytes)) return rc;
  if (int rc = dev_alloc(&h->d_cols, (size_t)n_terms, &bytes)) return rc;
  if (int rc = dev_alloc(&h->d_vals, (size_t)n_terms, &bytes)) return rc;
  if (int rc = dev_alloc(&h->d_w, (size_t)L.n_wires, &bytes)) return rc;
  if (int rc = dev_alloc(&h->d_tally, 1, &bytes)) return rc;
  uint8_t* d_raw = ds.buf.alloc<uint8_t>((size_t)L.payload_bytes); // this call's: freed with the session
  if (!d_raw) return dev_fail("hipMalloc", hipErrorOutOfMemory);
  if (int rc = reset_tally(h.get())) return rc;

  double upload_ms = 0;
  if (int rc = pv::timed_upload(dev, h->d_rowptr, rowptr.data(), rowptr.size() * 4, &upload_ms)) return rc;
  // row ρ is complete once byte 36·rowptr[ρ + 1] + 4·(ρ + 1) has landed: its kernel runs while the next slice is on its way
  auto row_end = [&](uint32_t row) { return pv::R1CS_TERM_BYTES * (uint64_t)rowptr[(size_t)row + 1] + 4 * ((uint64_t)row + 1); };
  uint32_t row_lo = 0;
  for (uint64_t off = 0; off < L.payload_bytes; off += SLICE_BYTES) {
    const size_t n = (size_t)std::min<uint64_t>(SLICE_BYTES, L.payload_bytes - off);
    if (int rc = pv::timed_upload(dev, d_raw + off, L.payload + off, n, &upload_ms)) return rc;
    uint32_t lo = row_lo, hi = rows; // the first row in [lo, hi] that is not complete
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (row_end(mid) <= off + n) lo = mid + 1;
      else hi = mid;
    }
    if (lo > row_lo) {
      DEV_LAUNCH("fill kernel launch", r1cs_fill_kernel, dim3((lo - row_lo + 255) / 256), dim3(256), h->st, (const uint32_t*)d_raw, h->d_rowptr, row_lo, lo, L.n_wires, h->d_cols,
                 h->d_vals, h->d_tally);
      row_lo = lo;
    }
  }
  Tally t;
  if (int rc = read_tally(h.get(), &t, "fill kernel")) return rc;
  if (t.bad_record != NONE) {
    const uint64_t row = t.bad_record >> 1;
    return pv::fail(pv::ERR_FORMAT, "r1cs: constraint %llu, matrix %c: %s", (unsigned long long)(row / 3), "ABC"[row % 3],
                    (t.bad_record & 1) ? "a coefficient is not below r" : "a wire id is not below nWires");
  }
  h->info.n_wires = L.n_wires;
  h->info.n_public = L.n_public();
  h->info.n_constraints = L.n_constraints;
  h->info.n_terms = n_terms;
  h->info.device_bytes = bytes;
  h->info.walk_ms = walk_ms;
  h->info.upload_ms = upload_ms;
  h->info.device_ms = pv::ms_since(t_dev);
  *out = h.release();
  return 0;
}

int check_resident_values(Groth16R1cs* h, Groth16WitnessReport* rep, std::chrono::steady_clock::time_point t_dev);

int witness_check_impl(Groth16R1cs* h, const uint8_t* wtns, size_t wtns_len, Groth16WitnessReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  if (!wtns) return pv::fail(pv::ERR_ARG, "null wtns");
  pv::Wtns w;
  if (int rc = pv::parse_wtns(wtns, wtns_len, w)) return rc;
  if (w.n_witness != h->n_wires) return pv::fail(pv::ERR_ARG, "the witness has %u values, the circuit %u wires", w.n_witness, h->n_wires);
  std::lock_guard<std::mutex> lk(h->mu);
  const auto t_dev = std::chrono::steady_clock::now();
  isnark::vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, h->dev, 0)) return rc;
  if (int rc = reset_tally(h)) return rc;
  if (int rc = pv::timed_upload(h->dev, h->d_w, w.values, (size_t)h->n_wires * 32, &rep->upload_ms)) return rc;
  return check_resident_values(h, rep, t_dev);
}

// the witness check over the n_wires values at h->d_w; the caller holds h->mu and the session, and has reset the tally
int check_resident_values(Groth16R1cs* h, Groth16WitnessReport* rep, std::chrono::steady_clock::time_point t_dev)
{
  DEV_LAUNCH("range kernel launch", witness_range_kernel, dim3((h->n_wires + 255) / 256), dim3(256), h->st, h->d_w, h->n_wires, h->d_tally);
  Tally t;
  if (int rc = read_tally(h, &t, "range kernel")) return rc;
  // the constraints only over canonical values: Fr::mul's bounds assume them
  if (t.noncanonical == 0 && h->m) {
    DEV_LAUNCH("constraint kernel launch", r1cs_constraint_kernel<0>, dim3((h->m + 255) / 256), dim3(256), h->st, h->d_rowptr, h->d_cols, h->d_vals, h->d_w, h->m, h->d_tally, (fe*)nullptr);
    if (int rc = read_tally(h, &t, "constraint kernel")) return rc;
  }
  rep->device_ms = pv::ms_since(t_dev);
  rep->noncanonical = t.noncanonical;
  rep->failed = t.failed;
  if (t.noncanonical) rep->kind = GROTH16_WTNS_NONCANONICAL, rep->index = t.first_noncanonical;
  else if (t.not_one) rep->kind = GROTH16_WTNS_ONE, rep->index = 0;
  else if (t.failed) rep->kind = GROTH16_WTNS_CONSTRAINT, rep->index = t.first_failed;
  return rep->kind ? 0 : 1;
}

// the same from a PACKED witness (wtns_pack.hip): sections 2 … 4 up, the decode into h->d_w, then the check as it is
int witness_check_packed_impl(Groth16R1cs* h, const uint8_t* wtnz, size_t len, Groth16WitnessReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  if (!wtnz) return pv::fail(pv::ERR_ARG, "null wtnz");
  pv::WtnzLayout L;
  if (int rc = pv::wtnz_layout(wtnz, len, &L)) return rc;
  if (int rc = pv::wtnz_is_bn254(L)) return rc;
  if (L.n_witness != h->n_wires) return pv::fail(pv::ERR_ARG, "the witness has %u values, the circuit %u wires", L.n_witness, h->n_wires);
  std::lock_guard<std::mutex> lk(h->mu);
  const auto t_dev = std::chrono::steady_clock::now();
  isnark::vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, h->dev, 0)) return rc;
  if (int rc = reset_tally(h)) return rc;
  uint8_t* d_buf = ds.buf.alloc<uint8_t>(pv::wtnz_device_bytes(L)); // this call's: freed with the session
  if (!d_buf) return dev_fail("hipMalloc", hipErrorOutOfMemory);
  pv::WtnzFault f;
  if (int rc = pv::wtnz_decode_on_device(h->dev, h->st, L, d_buf, h->d_w, &f, &rep->upload_ms, nullptr)) return rc;
  if (f.kind) return pv::wtnz_fail(f);
  return check_resident_values(h, rep, t_dev);
}

int match_zkey_impl(Groth16R1cs* h, const uint8_t* zkey, size_t len, const uint8_t* seed32, Groth16R1csMatchReport* rep)
{
  if (!rep) return pv::fail(pv::ERR_ARG, "null report");
  memset(rep, 0, sizeof *rep);
  if (!h) return pv::fail(pv::ERR_ARG, "null r1cs handle");
  std::vector<pv::Section> secs;
  pv::ZkeyLayout L;
  if (int rc = pv::zkey_layout(zkey, len, secs, &L, /*need_ic=*/false)) return rc;
  // sizes
  uint32_t k;
  const uint64_t domain = pv::circuit_domain(h->m, h->n_public, &k);
  const bool size_ok[3] = {L.n_vars == h->n_wires, L.n_public == h->n_public, L.domain == domain};
  for (int k = 0; k < 3; k++)
    if (!size_ok[k]) {
      rep->kind = GROTH16_MATCH_SIZES;
      rep->index = (uint64_t)k;
      return 0;
    }
  uint8_t seed[32];
  if (int rc = pv::seed_or_random(seed32, seed)) return rc;
  std::vector<fe> z(h->n_wires);
  pv::fill_coefficients(seed, 0, z.size(), z.data());

  std::lock_guard<std::mutex> lk(h->mu);
  const auto t_dev = std::chrono::steady_clock::now();
  isnark::vb::DeviceSession ds;
  if (int rc = pv::open_session(ds, h->dev, 0)) return rc;
  const uint32_t n = L.domain, m = h->m;
  uint32_t* d_rec = ds.buf.alloc<uint32_t>((size_t)L.n_coef * 11);
  uint32_t* k_rowptr = ds.buf.alloc<uint32_t>(2 * (size_t)n + 1);
  uint32_t* k_cols = ds.buf.alloc<uint32_t>(L.n_coef);
  fe* k_vals = ds.buf.alloc<fe>(L.n_coef);
  fe* d_vec = ds.buf.alloc<fe>(3 * (size_t)n);
  fe* d_ab = ds.buf.alloc<fe>(2 * (size_t)m);
  if (!d_rec || !k_rowptr || !k_cols || !k_vals || !d_vec || !d_ab) return dev_fail("hipMalloc", hipErrorOutOfMemory);
  if (int rc = reset_tally(h)) return rc;
  const isnark::CopyJob jobs[2] = {{h->d_w, z.data(), z.size() * sizeof z[0]}, {d_rec, L.records(), (size_t)L.n_coef * pv::COEF_RECORD_BYTES}};
  DEV_TRY("host to device upload", isnark::staged_copy(h->dev, jobs, 2, true));
  if (m) DEV_LAUNCH("emit kernel launch", r1cs_constraint_kernel<1>, dim3((m + 255) / 256), dim3(256), h->st, h->d_rowptr, h->d_cols, h->d_vals, h->d_w, m, h->d_tally, d_ab);
  // the key's side by the prover's own front end: the same CSR build (with its range rule) and the same spmv
  uint32_t first_bad = 0;
  DEV_TRY("coefficient CSR", isnark::qap_build_csr(d_rec, L.n_coef, n, L.n_vars, k_rowptr, k_cols, k_vals, &first_bad, h->st));
  if (first_bad != 0xffffffffu) return pv::fail(pv::ERR_FORMAT, "zkey: coefficient %u out of range", first_bad);
  DEV_TRY("spmv launch", isnark::qap_spmv(h->d_w, k_rowptr, k_cols, k_vals, n, d_vec, h->st));
  DEV_LAUNCH("compare kernel launch", r1cs_compare_kernel, dim3((n + 255) / 256), dim3(256), h->st, d_vec, d_ab, h->d_w, n, m, h->n_public, h->d_tally);
  Tally t;
  if (int rc = read_tally(h, &t, "match kernels")) return rc;
  rep->device_ms = pv::ms_since(t_dev);
  rep->rows_a = t.rows_a;
  rep->rows_b = t.rows_b;
  if (t.rows_a) rep->kind = GROTH16_MATCH_ROW_A, rep->index = t.first_a;
  else if (t.rows_b) rep->kind = GROTH16_MATCH_ROW_B, rep->index = t.first_b;
  return rep->kind ? 0 : 1;
}

} // namespace

// what groth16_zkey_verify_ptau (zkey_verify.hip) needs of a handle: its shape, its lock, and the rows at a vector of its own
namespace isnark {
namespace prover {
R1csShape r1cs_shape(const Groth16R1cs* h) { return {h->dev, h->n_wires, h->n_public, h->m}; }
std::mutex& r1cs_mutex(Groth16R1cs* h) { return h->mu; }
R1csDeviceRows r1cs_device_rows(const Groth16R1cs* h) { return {h->d_rowptr, h->d_cols, h->d_vals, h->n_terms}; }
int r1cs_emit_abc(Groth16R1cs* h, const fe* d_v, fe* d_abc, hipStream_t stream)
{
  if (!h->m) return 0;
  DEV_LAUNCH("emit kernel launch", r1cs_constraint_kernel<2>, dim3((h->m + 255) / 256), dim3(256), stream, h->d_rowptr, h->d_cols, h->d_vals, d_v, h->m, h->d_tally, d_abc);
  return 0;
}
} // namespace prover
} // namespace isnark

ISNARK_API int groth16_r1cs_match_zkey(Groth16R1cs* h, const void* zkey, size_t len, const uint8_t* seed32, Groth16R1csMatchReport* report)
{
  return match_zkey_impl(h, (const uint8_t*)zkey, len, seed32, report);
}

ISNARK_API int groth16_r1cs_load(const void* r1cs, size_t len, const char* device, Groth16R1cs** out)
{
  return r1cs_load_impl((const uint8_t*)r1cs, len, device, out);
}

ISNARK_API int groth16_r1cs_load_file(const char* path, const char* device, Groth16R1cs** out)
{
  if (out) *out = nullptr;
  if (!path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile mf;
  if (int rc = mf.open_ro(path)) return rc;
  const pv::FileHint hint(mf.data, mf.len, mf.fd); // (the staging workers pread() the file instead of copying out of the mapping)
  return r1cs_load_impl(mf.data, mf.len, device, out);
}

ISNARK_API int groth16_r1cs_get_info(const Groth16R1cs* h, Groth16R1csInfo* info)
{
  if (!h || !info) return pv::fail(pv::ERR_ARG, "null argument");
  *info = h->info;
  return 0;
}

ISNARK_API void groth16_r1cs_free(Groth16R1cs* h)
{
  if (!h) return;
  isnark::vb::DeviceSession ds;
  (void)ds.open(h->dev, 0);
  delete h;
}

ISNARK_API int groth16_witness_check(Groth16R1cs* h, const void* wtns, size_t wtns_len, Groth16WitnessReport* report)
{
  return witness_check_impl(h, (const uint8_t*)wtns, wtns_len, report);
}

ISNARK_API int groth16_witness_check_file(Groth16R1cs* h, const char* wtns_path, Groth16WitnessReport* report)
{
  if (!wtns_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile mf;
  if (int rc = mf.open_ro(wtns_path)) return rc;
  const pv::FileHint hint(mf.data, mf.len, mf.fd);
  return witness_check_impl(h, mf.data, mf.len, report);
}

ISNARK_API int groth16_witness_check_packed(Groth16R1cs* h, const void* wtnz, size_t len, Groth16WitnessReport* report)
{
  return witness_check_packed_impl(h, (const uint8_t*)wtnz, len, report);
}

ISNARK_API int groth16_witness_check_packed_file(Groth16R1cs* h, const char* wtnz_path, Groth16WitnessReport* report)
{
  if (!wtnz_path) return pv::fail(pv::ERR_ARG, "null path");
  pv::MappedFile mf;
  if (int rc = mf.open_ro(wtnz_path)) return rc;
  const pv::FileHint hint(mf.data, mf.len, mf.fd);
  return witness_check_packed_impl(h, mf.data, mf.len, report);
}
