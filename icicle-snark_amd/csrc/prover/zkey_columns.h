// zkey_columns.h — what groth16_zkey_new (zkey_new.hip) and groth16_setup (zkey_setup.hip) share: the handle's rows transposed into
// column lists, section 4's records, the heavy-column plan's types, and the layout of the key file both write.  Internal; the two
// translation units include it and each gets its own copy of the kernels (an unnamed namespace, as msm_impl.h's).
//
//   transpose   the handle's rows become column lists, one per (matrix, wire): zn_count_kernel (one lane per row: an atomic per
//               term on its column's counter; the public-binding rows nc … nc + npub count as terms of A), msm_sort.hip's scan, and
//               zn_scatter_kernel with an atomic cursor per column.  The order inside a column is whatever the atomics gave: the
//               sums do not depend on it.  The same pass counts A's and B's terms per constraint; their scan places section 4's
//               records, which zn_records_kernel writes.  transpose_rows enqueues all of it on one stream.
//   the file    FileLayout: sections 1 … 10 in this order; write_key_frame: the container's head, the section heads, sections 1 and
//               2, section 4's count and section 10's zero — everything of the file that is not a downloaded array.
#pragma once
#include <algorithm>
#include <type_traits>

#include "../workers.h"
#include "device_call.h"
#include "prover_internal.h"
#include "verify_batch.h"
#include "zkey_new29.h"

namespace {

namespace zcols_pv = isnark::prover;
using bn254::fe;
using bn254::Fq;
using bn254::Fr;
using bn254::zn29::ZnEntry;

constexpr uint32_t DEFAULT_HEAVY_COLUMN_TERMS = 64; // the large-bucket rule's floor (msm_sort.hip); swept for groth16_setup, not for zkey-new (§7e)
constexpr uint32_t MIN_HEAVY_COLUMN_TERMS = 8;
constexpr int ITEM_WG = 64;                          // lanes of an item's / a heavy column's workgroup: one wave

// an option's heavy_column_terms (0 = the default) as the kernels take it
inline uint32_t heavy_threshold(uint32_t asked) { return std::max(asked ? asked : DEFAULT_HEAVY_COLUMN_TERMS, MIN_HEAVY_COLUMN_TERMS); }

// what the kernels know of the transposed circuit: column (mat, s) is entries[colptr[mat·m + s] … colptr[mat·m + s + 1])
struct Columns {
  const uint32_t* colptr; // 3m + 1
  const ZnEntry* entries;
  const fe* vals;
  uint32_t m, thr;
};
struct Counters {
  uint32_t heavy[2], items[2]; // zkey-new: [0] G1, [1] G2; setup: [0] alone
  uint32_t longest;
};
struct Heavy {
  uint32_t job, first, n_items;
};
struct Item {
  uint32_t job, lo, hi;
};

// one lane per row ρ < 3·nc of the handle (ρ = 3j + matrix), then one per public-binding row
__global__ __launch_bounds__(256) void zn_count_kernel(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ cols, uint32_t nc, uint32_t m, uint32_t npub,
                                                        uint32_t* __restrict__ counts, uint32_t* __restrict__ ab_terms)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t rows = 3 * (uint64_t)nc;
  if (i < rows) {
    const uint32_t mat = (uint32_t)(i % 3);
    for (uint32_t t = rowptr[i]; t < rowptr[i + 1]; t++) atomicAdd(&counts[(size_t)mat * m + cols[t]], 1u);
    if (mat == 0) ab_terms[i / 3] = rowptr[i + 2] - rowptr[i];
  } else if (i - rows <= npub) {
    atomicAdd(&counts[i - rows], 1u);
  }
}
__global__ __launch_bounds__(256) void zn_scatter_kernel(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ cols, uint32_t nc, uint32_t m, uint32_t npub,
                                                          const uint32_t* __restrict__ colptr, uint32_t* __restrict__ cursor, ZnEntry* __restrict__ entries)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t rows = 3 * (uint64_t)nc;
  if (i < rows) {
    const uint32_t mat = (uint32_t)(i % 3), j = (uint32_t)(i / 3);
    for (uint32_t t = rowptr[i]; t < rowptr[i + 1]; t++) {
      const size_t col = (size_t)mat * m + cols[t];
      entries[colptr[col] + atomicAdd(&cursor[col], 1u)] = {j, t};
    }
  } else if (i - rows <= npub) {
    const uint32_t s = (uint32_t)(i - rows);
    entries[colptr[s] + atomicAdd(&cursor[s], 1u)] = {nc + s, bn254::zn29::ZN_BINDING};
  }
}
// section 4: record {matrix, row, wire, value·R² mod r} of A's and B's terms, constraint by constraint in the file's order
// (rec_off[j] = the records before constraint j, rec_off[nc] = all of them), then the binding records (0, nc + s, s, 1)
__global__ __launch_bounds__(256) void zn_records_kernel(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ cols, const fe* __restrict__ vals, uint32_t nc, uint32_t npub,
                                                          const uint32_t* __restrict__ rec_off, uint32_t* __restrict__ rec)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t rows = 3 * (uint64_t)nc;
  if (i < rows) {
    const uint32_t mat = (uint32_t)(i % 3), j = (uint32_t)(i / 3);
    if (mat == 2) return;
    const uint32_t t0 = rowptr[i];
    const size_t base = (size_t)rec_off[j] + (mat ? t0 - rowptr[i - 1] : 0u);
    for (uint32_t t = t0; t < rowptr[i + 1]; t++) {
      uint32_t* e = rec + (base + (t - t0)) * 11;
      const fe v = Fr::to_mont(ld(vals + t)); // value·R in the handle, value·R² in the file
      e[0] = mat, e[1] = j, e[2] = cols[t];
#pragma unroll
      for (int k = 0; k < 8; k++) e[3 + k] = v.l[k];
    }
  } else if (i - rows <= npub) {
    const uint32_t s = (uint32_t)(i - rows);
    uint32_t* e = rec + ((size_t)rec_off[nc] + s) * 11;
    const fe v = Fr::r2();
    e[0] = 0, e[1] = nc + s, e[2] = s;
#pragma unroll
    for (int k = 0; k < 8; k++) e[3 + k] = v.l[k];
  }
}

// the transposed circuit on the device, owned by the session it was made in
struct Transposed {
  uint32_t n_cols = 0;      // 3m + 1
  uint64_t n_entries = 0;   // the handle's terms and the npub + 1 binding rows
  uint32_t *d_colptr = nullptr, *d_recoff = nullptr, *d_rec = nullptr; // d_recoff[nc]: A's and B's terms; d_rec: section 4's records
  ZnEntry* d_entries = nullptr;
  Columns columns(const fe* d_vals, uint32_t m, uint32_t thr) const { return {d_colptr, d_entries, d_vals, m, thr}; }
};
// allocate in the session and enqueue on `st`: count, the two scans, scatter, records.  The caller has checked that 3m + 1 and the
// entries fit 32-bit offsets.
inline int transpose_rows(isnark::vb::DeviceSession& ds, hipStream_t st, const zcols_pv::R1csDeviceRows& rows, uint32_t nc, uint32_t m, uint32_t npub, Transposed* t)
{
  t->n_cols = 3 * m + 1;
  t->n_entries = rows.n_terms + npub + 1;
  uint32_t *d_counts, *d_ab, *d_scan;
  bool oom = false;
  auto alloc = [&](auto** p, size_t count) {
    typedef typename std::remove_pointer<typename std::remove_pointer<decltype(p)>::type>::type T;
    *p = ds.buf.alloc<T>(std::max<size_t>(count, 1));
    if (!*p) oom = true;
  };
  alloc(&d_counts, t->n_cols);
  alloc(&t->d_colptr, t->n_cols);
  alloc(&d_ab, (size_t)nc + 1);
  alloc(&t->d_recoff, (size_t)nc + 1);
  alloc(&d_scan, std::max(isnark::exclusive_scan_u32_scratch_words(t->n_cols), isnark::exclusive_scan_u32_scratch_words(nc + 1)));
  alloc(&t->d_rec, (size_t)t->n_entries * 11);
  alloc(&t->d_entries, (size_t)t->n_entries);
  if (oom) return zcols_pv::dev_fail("hipMalloc", hipErrorOutOfMemory);
  DEV_TRY("hipMemset", hipMemsetAsync(d_counts, 0, (size_t)t->n_cols * 4, st));
  DEV_TRY("hipMemset", hipMemsetAsync(d_ab, 0, ((size_t)nc + 1) * 4, st));
  const uint64_t row_lanes = 3 * (uint64_t)nc + npub + 1;
  const dim3 row_grid((uint32_t)((row_lanes + 255) / 256));
  DEV_LAUNCH("count kernel launch", zn_count_kernel, row_grid, dim3(256), st, rows.d_rowptr, rows.d_cols, nc, m, npub, d_counts, d_ab);
  DEV_TRY("column scan", isnark::exclusive_scan_u32(d_counts, t->n_cols, t->d_colptr, d_scan, st));
  DEV_TRY("record scan", isnark::exclusive_scan_u32(d_ab, nc + 1, t->d_recoff, d_scan, st));
  DEV_TRY("hipMemset", hipMemsetAsync(d_counts, 0, (size_t)t->n_cols * 4, st)); // now the cursors
  DEV_LAUNCH("scatter kernel launch", zn_scatter_kernel, row_grid, dim3(256), st, rows.d_rowptr, rows.d_cols, nc, m, npub, t->d_colptr, d_counts, t->d_entries);
  DEV_LAUNCH("records kernel launch", zn_records_kernel, row_grid, dim3(256), st, rows.d_rowptr, rows.d_cols, rows.d_vals, nc, npub, t->d_recoff, t->d_rec);
  return 0;
}

// byte offsets of the payloads in the file: sections 1 … 10 in this order, each behind its 12-byte {id, length}
struct FileLayout {
  uint64_t off[11], len[11], total;
  FileLayout(uint64_t m, uint64_t npub, uint64_t n, uint64_t n_coeffs)
  {
    const uint64_t l[11] = {0, 4, 4 + 32 + 4 + 32 + 12 + 3 * 64 + 3 * 128, 64 * (npub + 1), 4 + zcols_pv::COEF_RECORD_BYTES * n_coeffs, 64 * m, 64 * m, 128 * m, 64 * (m - npub - 1), 64 * n, 4};
    uint64_t pos = 12;
    for (int s = 1; s <= 10; s++) {
      len[s] = l[s];
      off[s] = pos + 12;
      pos += 12 + l[s];
    }
    total = pos;
  }
};

// the header's six points in the file's form, in the header's order
struct KeyHeaderPoints {
  const void *alpha1, *beta1, *beta2, *gamma2, *delta1, *delta2; // 64, 64, 128, 128, 64, 128 bytes
};
// everything of the file that is not a downloaded array
inline void write_key_frame(uint8_t* out, const FileLayout& F, uint32_t m, uint32_t npub, uint32_t n, uint64_t n_coeffs, const KeyHeaderPoints& hp)
{
  memcpy(out, "zkey", 4);
  const uint32_t version = 1, n_sections = 10, protocol = 1, n8 = 32, zero = 0, n_coeffs32 = (uint32_t)n_coeffs;
  memcpy(out + 4, &version, 4);
  memcpy(out + 8, &n_sections, 4);
  for (uint32_t s = 1; s <= 10; s++) {
    memcpy(out + F.off[s] - 12, &s, 4);
    memcpy(out + F.off[s] - 8, &F.len[s], 8);
  }
  memcpy(out + F.off[1], &protocol, 4);
  uint8_t* hd = out + F.off[2];
  const fe q = Fq::modulus(), r = Fr::modulus();
  memcpy(hd, &n8, 4);
  memcpy(hd + 4, q.l, 32);
  memcpy(hd + 36, &n8, 4);
  memcpy(hd + 40, r.l, 32);
  memcpy(hd + 72, &m, 4);
  memcpy(hd + 76, &npub, 4);
  memcpy(hd + 80, &n, 4);
  memcpy(hd + 84, hp.alpha1, 64);
  memcpy(hd + 148, hp.beta1, 64);
  memcpy(hd + 212, hp.beta2, 128);
  memcpy(hd + 340, hp.gamma2, 128);
  memcpy(hd + 468, hp.delta1, 64);
  memcpy(hd + 532, hp.delta2, 128);
  memcpy(out + F.off[4], &n_coeffs32, 4);
  memcpy(out + F.off[10], &zero, 4);
}

} // namespace
