// containers.cpp — snarkjs binary containers (.zkey / .wtns / .r1cs / .ptau) and the prover host's error text.
//   FileWrapper::read_bin_file ← src/file_wrapper.rs:45-103;  read_wtns_header ← :169-177, src/proof_helper.rs:247-268
#include <algorithm>
#include <fcntl.h>
#include <errno.h>
#include <sys/mman.h>
#include <sys/random.h>
#include <sys/stat.h>
#include <unistd.h>

#include "prover_internal.h"
#include "wtns_pack.h"

using namespace bn254;
using namespace isnark;
using namespace isnark::prover;

namespace isnark {
namespace prover {

static thread_local char g_perr[512] = "";
int fail(int code, const char* fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_perr, sizeof g_perr, fmt, ap);
  va_end(ap);
  return code;
}
const char* last_error_text() { return g_perr; }
void set_error_text(const char* text) { snprintf(g_perr, sizeof g_perr, "%s", text ? text : ""); }

// FileWrapper::read_bin_file — src/file_wrapper.rs:45-103
int read_sections(const uint8_t* data, size_t len, const char* type, uint32_t max_version, std::vector<Section>& out)
{
  if (len < 12 || memcmp(data, type, 4) != 0) return fail(ERR_FORMAT, "Invalid File format (expected '%s')", type);
  uint32_t version, nsec;
  memcpy(&version, data + 4, 4);
  memcpy(&nsec, data + 8, 4);
  if (version > max_version) return fail(ERR_FORMAT, "Version not supported");
  // (ids up to the section count, but no more slots than the file has room for section headers: a hostile count sizes nothing)
  const uint64_t slots = std::min<uint64_t>(nsec, (len - 12) / 12) + 1;
  out.assign(slots > 16 ? (size_t)slots : 16, Section());
  size_t pos = 12;
  for (uint32_t i = 0; i < nsec; i++) {
    if (len - pos < 12) return fail(ERR_FORMAT, "truncated section table");
    uint32_t ht;
    uint64_t hl;
    memcpy(&ht, data + pos, 4);
    memcpy(&hl, data + pos + 4, 8);
    pos += 12;
    if (hl > len - pos) return fail(ERR_FORMAT, "section %u exceeds the file", ht); // pos <= len here; `pos + hl` could wrap for a hostile 64-bit length
    if (ht < out.size()) {
      out[ht].p = data + pos;
      out[ht].size = hl;
      out[ht].count++;
    }
    pos += hl;
  }
  return 0;
}
int unique_section(const std::vector<Section>& s, size_t id, const Section** sec)
{
  if (id >= s.size() || s[id].count == 0) return fail(ERR_FORMAT, "Missing section %zu", id);
  if (s[id].count > 1) return fail(ERR_FORMAT, "Section Duplicated %zu", id);
  *sec = &s[id];
  return 0;
}

// sections and header of a zkey (prover_internal.h: ZkeyLayout) — the only code that knows the container's and the header's rules
// the sections of a container that read_sections has passed, in the file's order
std::vector<SectionEntry> sections_in_order(const uint8_t* data)
{
  uint32_t nsec;
  memcpy(&nsec, data + 8, 4);
  std::vector<SectionEntry> out;
  size_t pos = 12;
  for (uint32_t i = 0; i < nsec; i++) {
    SectionEntry e;
    memcpy(&e.id, data + pos, 4);
    memcpy(&e.size, data + pos + 4, 8);
    e.p = data + pos + 12;
    out.push_back(e);
    pos += 12 + (size_t)e.size;
  }
  return out;
}
// where the last of them ends (bytes behind it are no part of the container)
static uint64_t container_end(const uint8_t* data)
{
  uint64_t pos = 12;
  for (const SectionEntry& e : sections_in_order(data)) pos += 12 + e.size;
  return pos;
}

// the container, section 1 and the header (section 2) of a key under `magic`: what a .zkey and a packed key share
static int zkey_header(const uint8_t* data, size_t len, const char* magic, uint32_t max_version, std::vector<Section>& secs, ZkeyLayout* L, bool need_ic)
{
  if (int rc = read_sections(data, len, magic, max_version, secs)) return rc;
  const Section* s1;
  if (int rc = unique_section(secs, 1, &s1)) return rc;
  uint32_t protocol = 0;
  if (s1->size >= 4) memcpy(&protocol, s1->p, 4);
  if (protocol != 1) return fail(ERR_FORMAT, "Protocol not supported"); // GROTH16_PROTOCOL_ID, file_wrapper.rs:12,196-207
  for (int id : {2, 3, 4, 5, 6, 7, 8, 9}) {
    if (id == 3 && !need_ic) {
      L->sec[3] = secs[3].count == 1 ? &secs[3] : nullptr; // (read_sections makes room for the ids below 16)
      continue;
    }
    if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  }
  // read_header_groth16 — src/zkey.rs:47-85
  const Section* s2 = L->sec[2];
  const uint8_t* h = s2->p;
  if (s2->size < 4 + 32 + 4 + 32 + 12 + 3 * 64 + 3 * 128) return fail(ERR_FORMAT, "zkey header too short");
  memcpy(&L->n8q, h, 4);
  if (L->n8q != 32) return fail(ERR_FORMAT, "zkey: unsupported base field size");
  memcpy(L->q.l, h + 4, 32);
  memcpy(&L->n8r, h + 36, 4);
  if (L->n8r != 32) return fail(ERR_FORMAT, "zkey: unsupported scalar field size");
  memcpy(L->r.l, h + 40, 32);
  memcpy(&L->n_vars, h + 72, 4);
  memcpy(&L->n_public, h + 76, 4);
  memcpy(&L->domain, h + 80, 4);
  if (!Fq::eq(L->q, Fq::modulus()) || !Fr::eq(L->r, Fr::modulus())) return fail(ERR_FORMAT, "zkey: not a BN254 key");
  const uint32_t n = L->domain;
  if (n == 0 || (n & (n - 1))) return fail(ERR_FORMAT, "zkey: domain size %u is not a power of two", n);
  if (L->n_public + 1 > L->n_vars) return fail(ERR_FORMAT, "zkey: n_public exceeds n_vars");
  L->header_points = h + 84;
  return 0;
}

int zkey_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, ZkeyLayout* L, bool need_ic)
{
  if (!data) return fail(ERR_ARG, "null zkey");
  if (int rc = zkey_header(data, len, "zkey", 2, secs, L, need_ic)) return rc;
  const uint32_t n = L->domain;
  // coefficients (section 4): a declared count, then the records — src/cache.rs:126-166
  const Section* s4 = L->sec[4];
  if (s4->size < 4 || (s4->size - 4) % COEF_RECORD_BYTES) return fail(ERR_FORMAT, "zkey: coefficient section size");
  if ((s4->size - 4) / COEF_RECORD_BYTES > 0xffffffffull) return fail(ERR_FORMAT, "zkey: too many coefficients");
  L->n_coef = (uint32_t)((s4->size - 4) / COEF_RECORD_BYTES);
  const uint64_t nv = L->n_vars, np1 = (uint64_t)L->n_public + 1;
  if ((need_ic && L->sec[3]->size != np1 * 64) || L->sec[5]->size != nv * 64 || L->sec[6]->size != nv * 64 || L->sec[7]->size != nv * 128 || L->sec[8]->size != (nv - np1) * 64 ||
      L->sec[9]->size != (uint64_t)n * 64)
    return fail(ERR_FORMAT, "zkey: point section size mismatch");
  return 0;
}

// section 4 of a packed key, or a raw packed body (prover_internal.h: ZkezCoefs): the size against the sum of its parts, the directory
int zkez_coefs_layout(const uint8_t* body, uint64_t size, ZkezCoefs* C)
{
  if (size < ZKEZ_COEFS_HEAD) return fail(ERR_FORMAT, "zkez: section 4 holds %llu bytes, its three counts alone have %llu", (unsigned long long)size, (unsigned long long)ZKEZ_COEFS_HEAD);
  memcpy(&C->declared, body, 4);
  memcpy(&C->n_coef, body + 4, 4);
  memcpy(&C->payload_bytes, body + 8, 8);
  C->n_blocks = ((uint64_t)C->n_coef + wz::WZ_BLOCK - 1) / wz::WZ_BLOCK;
  // (the payload's size is compared first: a hostile one cannot wrap the sum)
  if (C->payload_bytes > size || zkez_coefs_bytes(C->n_coef, C->payload_bytes) != size)
    return fail(ERR_FORMAT, "zkez: section 4 holds %llu bytes, %u coefficients with a payload of %llu bytes have %llu", (unsigned long long)size, C->n_coef,
                (unsigned long long)C->payload_bytes, (unsigned long long)(C->payload_bytes > size ? 0 : zkez_coefs_bytes(C->n_coef, C->payload_bytes)));
  C->triples = body + ZKEZ_COEFS_HEAD;
  C->codes = C->triples + 12 * (uint64_t)C->n_coef;
  C->dir = C->codes + C->n_coef;
  C->payload = C->dir + 8 * (C->n_blocks + 1);
  uint64_t at = 0;
  switch (wz::wz_check_directory(C->dir, C->n_blocks, C->payload_bytes, &at)) {
  case 0: break;
  case 1: return fail(ERR_FORMAT, "zkez: directory entry 0 is %llu, not 0", (unsigned long long)wz::wz_dir_entry(C->dir, 0));
  case 2: return fail(ERR_FORMAT, "zkez: directory entry %llu is below entry %llu", (unsigned long long)at, (unsigned long long)(at - 1));
  case 3:
    return fail(ERR_FORMAT, "zkez: block %llu spans %llu bytes, %u is the most", (unsigned long long)at, (unsigned long long)(wz::wz_dir_entry(C->dir, at + 1) - wz::wz_dir_entry(C->dir, at)),
                wz::WZ_MAX_SPAN);
  default:
    return fail(ERR_FORMAT, "zkez: the directory ends at %llu, the payload holds %llu bytes", (unsigned long long)wz::wz_dir_entry(C->dir, C->n_blocks), (unsigned long long)C->payload_bytes);
  }
  return 0;
}

// sections, header and section 4 of a PACKED proving key (prover_internal.h: PackedZkey): everything an unpack kernel relies on
// is bounded here, before a byte goes up
int zkez_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, ZkeyLayout* L, PackedZkey* P)
{
  if (!data) return fail(ERR_ARG, "null zkez");
  if (int rc = zkey_header(data, len, "zkez", 1, secs, L, /*need_ic=*/true)) return rc;
  const uint64_t nv = L->n_vars, np1 = (uint64_t)L->n_public + 1;
  const uint64_t want[10] = {0, 0, 0, np1 * 32, 0, nv * 32, nv * 32, nv * 64, (nv - np1) * 32, (uint64_t)L->domain * 32};
  uint64_t points = 0;
  for (int id : {3, 5, 6, 7, 8, 9}) {
    if (L->sec[id]->size != want[id])
      return fail(ERR_FORMAT, "zkez: section %d holds %llu bytes, a packed key of %u wires, %u public signals and domain %u has %llu", id, (unsigned long long)L->sec[id]->size, L->n_vars,
                  L->n_public, L->domain, (unsigned long long)want[id]);
    points += want[id];
  }
  if (int rc = zkez_coefs_layout(L->sec[4]->p, L->sec[4]->size, &P->coefs)) return rc;
  L->n_coef = P->coefs.n_coef;
  P->unpacked_bytes = container_end(data) + points - L->sec[4]->size + 4 + (uint64_t)L->n_coef * COEF_RECORD_BYTES;
  L->packed = P;
  return 0;
}

// sections and header of an .r1cs (prover_internal.h: R1csLayout) — iden3's binary format: sections by id in any order, unknown
// ids (the wire → label map 3, the custom-gate sections 4 and 5) ignored
int r1cs_layout(const uint8_t* data, size_t len, R1csLayout* L)
{
  if (!data) return fail(ERR_ARG, "null r1cs");
  std::vector<Section> secs;
  if (int rc = read_sections(data, len, "r1cs", 1, secs)) return rc;
  const Section *h, *c;
  if (int rc = unique_section(secs, 1, &h)) return rc;
  if (int rc = unique_section(secs, 2, &c)) return rc;
  uint32_t n8 = 0;
  if (h->size >= 4) memcpy(&n8, h->p, 4);
  if (n8 != 32) return fail(ERR_FORMAT, "r1cs: unsupported field size %u", n8);
  if (h->size != 4 + 32 + 16 + 8 + 4) return fail(ERR_FORMAT, "r1cs: header size mismatch");
  fe prime;
  memcpy(prime.l, h->p + 4, 32);
  if (!Fr::eq(prime, Fr::modulus())) return fail(ERR_FORMAT, "r1cs: the prime is not the BN254 scalar field's");
  memcpy(&L->n_wires, h->p + 36, 4);
  memcpy(&L->n_pub_out, h->p + 40, 4);
  memcpy(&L->n_pub_in, h->p + 44, 4);
  memcpy(&L->n_prv_in, h->p + 48, 4);
  memcpy(&L->n_labels, h->p + 52, 8);
  memcpy(&L->n_constraints, h->p + 60, 4);
  if ((uint64_t)L->n_pub_out + L->n_pub_in + 1 > L->n_wires) return fail(ERR_FORMAT, "r1cs: the public signals exceed nWires");
  // (a constraint is at least its three count words: a hostile mConstraints must not size the row table)
  if (L->n_constraints > 0xfffffffeu / 3) return fail(ERR_FORMAT, "r1cs: too many constraints"); // row ids 3j + k are 32 bits
  if ((uint64_t)L->n_constraints * 12 > c->size) return fail(ERR_FORMAT, "r1cs: %u constraints do not fit section 2", L->n_constraints);
  L->payload = c->p;
  L->payload_bytes = c->size;
  return 0;
}

// One sequential pass over section 2 that reads the count words alone: rowptr[3m + 1] in terms, row 3j + k = linear combination
// k (A, B, C) of constraint j.  Every record the kernels will read lies inside the payload once this has passed.
int r1cs_walk(const R1csLayout& L, std::vector<uint32_t>& rowptr, uint64_t* n_terms)
{
  const uint64_t rows = 3 * (uint64_t)L.n_constraints, size = L.payload_bytes;
  rowptr.assign((size_t)rows + 1, 0);
  uint64_t pos = 0, terms = 0;
  for (uint64_t row = 0; row < rows; row++) {
    const unsigned j = (unsigned)(row / 3);
    const char mat = "ABC"[row % 3];
    if (size - pos < 4) return fail(ERR_FORMAT, "r1cs: constraint %u, matrix %c: section 2 ends before its count", j, mat);
    uint32_t cnt;
    memcpy(&cnt, L.payload + pos, 4);
    pos += 4;
    if ((size - pos) / R1CS_TERM_BYTES < cnt) return fail(ERR_FORMAT, "r1cs: constraint %u, matrix %c: a count of %u overruns section 2", j, mat, cnt);
    pos += (uint64_t)cnt * R1CS_TERM_BYTES;
    terms += cnt;
    if (terms > 0xffffffffull) return fail(ERR_FORMAT, "r1cs: more than 2^32 - 1 terms");
    rowptr[(size_t)row + 1] = (uint32_t)terms;
  }
  if (pos != size) return fail(ERR_FORMAT, "r1cs: section 2 has %llu bytes left behind its %u constraints", (unsigned long long)(size - pos), L.n_constraints);
  *n_terms = terms;
  return 0;
}

// container and section 1 of a .ptau, prepared or not: magic, version, n8, q, power
static int ptau_header(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L, bool bound_power = true, const char* magic = "ptau")
{
  if (!data) return fail(ERR_ARG, "null ptau");
  if (int rc = read_sections(data, len, magic, 1, secs)) return rc;
  const Section* h;
  if (int rc = unique_section(secs, 1, &h)) return rc;
  uint32_t n8 = 0;
  if (h->size >= 4) memcpy(&n8, h->p, 4);
  if (n8 != 32) return fail(ERR_FORMAT, "ptau: unsupported base field size %u", n8);
  if (h->size != 4 + 32 + 8) return fail(ERR_FORMAT, "ptau: header size mismatch");
  fe q;
  memcpy(q.l, h->p + 4, 32);
  if (!Fq::eq(q, Fq::modulus())) return fail(ERR_FORMAT, "ptau: the prime is not the BN254 base field's");
  memcpy(&L->power, h->p + 36, 4);
  memcpy(&L->ceremony_power, h->p + 40, 4);
  if (bound_power && L->power > 28) return fail(ERR_FORMAT, "ptau: power %u is above the field's two-adicity", L->power);
  L->sec[1] = h;
  return 0;
}

// sections and header of a prepared .ptau (prover_internal.h: PtauLayout)
int ptau_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L)
{
  if (int rc = ptau_header(data, len, secs, L)) return rc;
  for (int id : {4, 5, 6})
    if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  if (L->sec[4]->size < 64 || L->sec[5]->size < 64 || L->sec[6]->size < 128) return fail(ERR_FORMAT, "ptau: section 4, 5 or 6 is shorter than one point");
  bool prepared = false;
  for (int id = 12; id < 16; id++) prepared = prepared || secs[(size_t)id].count != 0; // (read_sections makes room for the ids below 16)
  if (!prepared) return fail(ERR_FORMAT, "ptau: sections 12 to 15 are missing: the file has not been prepared for phase 2 (snarkjs powersoftau prepare phase2)");
  for (int id = 12; id < 16; id++)
    if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  return 0;
}

// sections and header of an UNPREPARED .ptau, what a ceremony ends with: sections 2 … 7 once each with exactly the element counts
// of the layout, none of 12 … 15
int ptau_unprepared_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L)
{
  if (int rc = ptau_header(data, len, secs, L)) return rc;
  for (int id = 12; id < 16; id++) // (read_sections makes room for the ids below 16)
    if (secs[(size_t)id].count) return fail(ERR_FORMAT, "ptau: section %d is present: the file is already prepared for phase 2", id);
  for (int id : {2, 3, 4, 5, 6, 7})
    if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  const uint64_t N = (uint64_t)1 << L->power;
  const uint64_t want[7] = {0, 0, (2 * N - 1) * 64, N * 128, N * 64, N * 64, 128};
  for (int id = 2; id <= 6; id++)
    if (L->sec[id]->size != want[id])
      return fail(ERR_FORMAT, "ptau: section %d holds %llu bytes, an unprepared file of power %u has %llu", id, (unsigned long long)L->sec[id]->size, L->power,
                  (unsigned long long)want[id]);
  return 0;
}

uint64_t ptau_prepared_section_bytes(uint32_t power, int sid)
{
  const uint64_t N = (uint64_t)1 << power;
  return sid == 12 ? (4 * N - 1) * 64 : (2 * N - 1) * (sid == 13 ? 128 : 64);
}

// sections and header of a .ptau in EITHER form, what groth16_ptau_verify takes: sections 2 … 7 once each with the unprepared
// layout's exact element counts, and of 12 … 15 none, or all four once each with exactly what prepare writes
int ptau_either_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L, bool* prepared)
{
  if (int rc = ptau_header(data, len, secs, L, /*bound_power=*/false)) return rc;
  if (L->power > 27) return fail(ERR_ARG, "ptau: power %u is above 27, the highest a file with section 12's block for power + 1 can have", L->power);
  int have = 0;
  for (int id = 12; id < 16; id++) have += secs[(size_t)id].count != 0; // (read_sections makes room for the ids below 16)
  if (have != 0 && have != 4) return fail(ERR_FORMAT, "ptau: %d of the sections 12 to 15 are present: a file has none of them or all four", have);
  *prepared = have == 4;
  for (int id = 2; id < 16; id++)
    if (id <= 7 || (id >= 12 && *prepared))
      if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  const uint64_t N = (uint64_t)1 << L->power;
  const uint64_t want[7] = {0, 0, (2 * N - 1) * 64, N * 128, N * 64, N * 64, 128};
  for (int id = 2; id < 16; id++) {
    if (id == 7 || (id > 7 && !(id >= 12 && *prepared))) continue;
    const uint64_t w = id <= 6 ? want[id] : ptau_prepared_section_bytes(L->power, id);
    if (L->sec[id]->size != w)
      return fail(ERR_FORMAT, "ptau: section %d holds %llu bytes, a file of power %u has %llu", id, (unsigned long long)L->sec[id]->size, L->power, (unsigned long long)w);
  }
  return 0;
}

uint64_t ptau_packed_section_bytes(uint32_t power, int sid)
{
  const uint64_t N = (uint64_t)1 << power;
  const uint64_t low[7] = {0, 0, (2 * N - 1) * 32, N * 64, N * 32, N * 32, 64};
  return sid <= 6 ? low[sid] : ptau_prepared_section_bytes(power, sid) / 2;
}

// sections and header of a PACKED powers-of-tau file (ptau_pack.hip): a .ptau's section table and section 1 under magic "ptaz",
// version 1; sections 2 … 7 once each, and of 12 … 15 none or all four, the point sections with exactly the packed element counts
int ptau_packed_layout(const uint8_t* data, size_t len, std::vector<Section>& secs, PtauLayout* L, bool* prepared)
{
  if (int rc = ptau_header(data, len, secs, L, /*bound_power=*/false, "ptaz")) return rc;
  if (L->power > 27) return fail(ERR_ARG, "ptau: power %u is above 27, the highest a packed file can have", L->power);
  int have = 0;
  for (int id = 12; id < 16; id++) have += secs[(size_t)id].count != 0; // (read_sections makes room for the ids below 16)
  if (have != 0 && have != 4) return fail(ERR_FORMAT, "ptau: %d of the sections 12 to 15 are present: a file has none of them or all four", have);
  *prepared = have == 4;
  for (int id = 2; id < 16; id++)
    if (id <= 7 || (id >= 12 && *prepared))
      if (int rc = unique_section(secs, (size_t)id, &L->sec[id])) return rc;
  for (int id = 2; id < 16; id++) {
    if (id == 7 || (id > 7 && !(id >= 12 && *prepared))) continue;
    const uint64_t w = ptau_packed_section_bytes(L->power, id);
    if (L->sec[id]->size != w)
      return fail(ERR_FORMAT, "ptau: section %d holds %llu bytes, a packed file of power %u has %llu", id, (unsigned long long)L->sec[id]->size, L->power, (unsigned long long)w);
  }
  return 0;
}

int ptau_block(const PtauLayout& L, int sid, uint32_t p, size_t elem_bytes, const uint8_t** out)
{
  const uint64_t first = ((uint64_t)1 << p) - 1, end = (first + ((uint64_t)1 << p)) * elem_bytes; // p <= 29: no overflow
  if (end > L.sec[sid]->size)
    return fail(ERR_FORMAT, "ptau: section %d holds %llu bytes, its block for power %u ends at byte %llu", sid, (unsigned long long)L.sec[sid]->size, p, (unsigned long long)end);
  *out = L.sec[sid]->p + first * elem_bytes;
  return 0;
}

int ptau_blocks_for_domain(const PtauLayout& L, uint32_t k)
{
  if (L.power < k) return fail(ERR_ARG, "ptau: power %u is below the key's domain 2^%u", L.power, k);
  const uint8_t* p;
  for (int id : {12, 13, 14, 15})
    if (int rc = ptau_block(L, id, k, id == 13 ? 128 : 64, &p)) return rc;
  return ptau_block(L, 12, k + 1, 64, &p);
}

MappedFile::~MappedFile()
{
  if (data) munmap((void*)data, len);
  if (fd >= 0) close(fd);
}
int MappedFile::open_ro(const char* path, bool read_ahead)
  {
    fd = ::open(path, O_RDONLY); // the reference opens read-write although it only reads (file_wrapper.rs:50-54)
    if (fd < 0) return fail(ERR_IO, "cannot open %s", path);
    struct stat st;
    if (fstat(fd, &st) != 0) return fail(ERR_IO, "cannot stat %s", path);
    len = (size_t)st.st_size;
    void* p = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) return fail(ERR_IO, "cannot mmap %s", path);
    data = (const uint8_t*)p;
    if (read_ahead) (void)madvise(p, len, MADV_WILLNEED); // start the read-ahead; the upload workers touch the pages in parallel
    return 0;
  }

// read_wtns_header + section 2 — src/file_wrapper.rs:169-177, src/proof_helper.rs:247-268
int parse_wtns(const uint8_t* data, size_t len, Wtns& w)
{
  std::vector<Section> s;
  if (int rc = read_sections(data, len, "wtns", 2, s)) return rc;
  const Section *h, *v;
  if (int rc = unique_section(s, 1, &h)) return rc;
  if (int rc = unique_section(s, 2, &v)) return rc;
  if (h->size < 8) return fail(ERR_FORMAT, "wtns header too short");
  memcpy(&w.n8, h->p, 4);
  if (w.n8 != 32 || h->size != 4 + 32 + 4) return fail(ERR_FORMAT, "wtns: unsupported field size %u", w.n8);
  memcpy(w.q.l, h->p + 4, 32);
  memcpy(&w.n_witness, h->p + 36, 4);
  if (v->size != (uint64_t)w.n_witness * 32) return fail(ERR_FORMAT, "wtns: section 2 size mismatch");
  w.values = v->p;
  return 0;
}

// sections, header and directory of a PACKED witness (prover_internal.h: WtnzLayout; wtns_pack.h): everything a decoder — the host's
// or the kernel — relies on is bounded here, before a byte goes up
int wtnz_layout(const uint8_t* data, size_t len, WtnzLayout* L)
{
  if (!data) return fail(ERR_ARG, "null wtnz");
  std::vector<Section> s;
  if (int rc = read_sections(data, len, "wtnz", 1, s)) return rc;
  const Section* sec[5];
  for (size_t id = 1; id <= 4; id++)
    if (int rc = unique_section(s, id, &sec[id])) return rc;
  if (sec[1]->size >= 4) memcpy(&L->n8, sec[1]->p, 4);
  if (L->n8 != 32 || sec[1]->size != 4 + 32 + 4) return fail(ERR_FORMAT, "wtnz: unsupported field size %u", L->n8);
  L->header = sec[1]->p;
  memcpy(L->q.l, sec[1]->p + 4, 32);
  memcpy(&L->n_witness, sec[1]->p + 36, 4);
  L->n_blocks = ((uint64_t)L->n_witness + wz::WZ_BLOCK - 1) / wz::WZ_BLOCK;
  if (sec[2]->size != L->n_witness)
    return fail(ERR_FORMAT, "wtnz: section 2 holds %llu bytes, %u values have %u codes", (unsigned long long)sec[2]->size, L->n_witness, L->n_witness);
  if (sec[3]->size != (L->n_blocks + 1) * 8)
    return fail(ERR_FORMAT, "wtnz: section 3 holds %llu bytes, the directory of %u values has %llu", (unsigned long long)sec[3]->size, L->n_witness, (unsigned long long)((L->n_blocks + 1) * 8));
  L->codes = sec[2]->p;
  L->dir = sec[3]->p;
  L->payload = sec[4]->p;
  L->payload_bytes = sec[4]->size;
  uint64_t at = 0;
  switch (wz::wz_check_directory(L->dir, L->n_blocks, L->payload_bytes, &at)) {
  case 0: break;
  case 1: return fail(ERR_FORMAT, "wtnz: directory entry 0 is %llu, not 0", (unsigned long long)wz::wz_dir_entry(L->dir, 0));
  case 2: return fail(ERR_FORMAT, "wtnz: directory entry %llu is below entry %llu", (unsigned long long)at, (unsigned long long)(at - 1));
  case 3:
    return fail(ERR_FORMAT, "wtnz: block %llu spans %llu bytes, %u is the most", (unsigned long long)at, (unsigned long long)(wz::wz_dir_entry(L->dir, at + 1) - wz::wz_dir_entry(L->dir, at)),
                wz::WZ_MAX_SPAN);
  default:
    return fail(ERR_FORMAT, "wtnz: the directory ends at %llu, section 4 holds %llu bytes", (unsigned long long)wz::wz_dir_entry(L->dir, L->n_blocks), (unsigned long long)L->payload_bytes);
  }
  return 0;
}
int wtnz_is_bn254(const WtnzLayout& L)
{
  return Fr::eq(L.q, Fr::modulus()) ? 0 : fail(ERR_FORMAT, "wtnz: the prime is not the BN254 scalar field's");
}

} // namespace prover
} // namespace isnark

// host only: never initialises a GPU
__attribute__((visibility("default"))) int groth16_r1cs_info(const void* r1cs, size_t len, Groth16R1csInfo* info)
{
  if (!info) return fail(ERR_ARG, "null info");
  memset(info, 0, sizeof *info);
  R1csLayout L;
  if (int rc = r1cs_layout((const uint8_t*)r1cs, len, &L)) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> rowptr;
  if (int rc = r1cs_walk(L, rowptr, &info->n_terms)) return rc;
  info->walk_ms = ms_since(t0);
  info->n_wires = L.n_wires;
  info->n_public = L.n_public();
  info->n_constraints = L.n_constraints;
  return 0;
}

// host only: never initialises a GPU
__attribute__((visibility("default"))) int groth16_ptau_info(const void* ptau, size_t len, int32_t domain_power, Groth16PtauInfo* info)
{
  if (!info) return fail(ERR_ARG, "null info");
  memset(info, 0, sizeof *info);
  std::vector<Section> secs;
  PtauLayout L;
  if (int rc = ptau_layout((const uint8_t*)ptau, len, secs, &L)) return rc;
  if (domain_power > 28) return fail(ERR_ARG, "domain power %d is above the field's two-adicity", domain_power);
  if (domain_power >= 0)
    if (int rc = ptau_blocks_for_domain(L, (uint32_t)domain_power)) return rc;
  info->power = L.power;
  info->ceremony_power = L.ceremony_power;
  for (size_t id = 0; id < 16; id++) info->section_bytes[id] = secs[id].count == 1 ? secs[id].size : 0;
  return 0;
}

// host only: never initialises a GPU.  The sizes of groth16_zkey_new's file (zkey_new.hip has its layout).
__attribute__((visibility("default"))) int groth16_zkey_new_size(const void* r1cs, size_t len, uint64_t* zkey_bytes, uint64_t* n_coeffs)
{
  if (!zkey_bytes || !n_coeffs) return fail(ERR_ARG, "null output");
  *zkey_bytes = *n_coeffs = 0;
  R1csLayout L;
  if (int rc = r1cs_layout((const uint8_t*)r1cs, len, &L)) return rc;
  std::vector<uint32_t> rowptr;
  uint64_t n_terms = 0;
  if (int rc = r1cs_walk(L, rowptr, &n_terms)) return rc;
  const uint64_t m = L.n_wires, npub = L.n_public(), nc = L.n_constraints;
  if (m < npub + 1) return fail(ERR_FORMAT, "r1cs: %u wires cannot hold the constant and %u public signals", L.n_wires, L.n_public());
  uint64_t ab = 0;
  for (uint64_t j = 0; j < nc; j++) ab += rowptr[3 * j + 2] - rowptr[3 * j]; // A's and B's terms; C has no records
  uint32_t k;
  const uint64_t n = circuit_domain(nc, npub, &k);
  *n_coeffs = ab + npub + 1;
  const uint64_t payload = 4 + (4 + 32 + 4 + 32 + 12 + 3 * 64 + 3 * 128) + 64 * (npub + 1) + (4 + COEF_RECORD_BYTES * *n_coeffs) + 64 * m + 64 * m + 128 * m +
                           64 * (m - npub - 1) + 64 * n + 4;
  *zkey_bytes = 12 + 10 * 12 + payload;
  return 0;
}

// host only: never initialise a GPU.  The size of groth16_zkey_unpack's file, exact, and an upper bound of groth16_zkey_pack's — every
// coefficient at 32 payload bytes — both from the container alone (zkey_pack.hip).
__attribute__((visibility("default"))) int groth16_zkey_unpacked_size(const void* zkez, size_t len, uint64_t* zkey_bytes)
{
  if (!zkey_bytes) return fail(ERR_ARG, "null output");
  *zkey_bytes = 0;
  std::vector<Section> secs;
  ZkeyLayout L;
  PackedZkey P;
  if (int rc = zkez_layout((const uint8_t*)zkez, len, secs, &L, &P)) return rc;
  *zkey_bytes = P.unpacked_bytes;
  return 0;
}
__attribute__((visibility("default"))) int groth16_zkey_packed_bound(const void* zkey, size_t len, uint64_t* packed_bytes)
{
  if (!packed_bytes) return fail(ERR_ARG, "null output");
  *packed_bytes = 0;
  std::vector<Section> secs;
  ZkeyLayout L;
  if (int rc = zkey_layout((const uint8_t*)zkey, len, secs, &L, /*need_ic=*/true)) return rc;
  uint64_t points = 0;
  for (int id : {3, 5, 6, 7, 8, 9}) points += L.sec[id]->size;
  *packed_bytes = container_end((const uint8_t*)zkey) - points / 2 - L.sec[4]->size + zkez_coefs_bytes(L.n_coef, 32 * (uint64_t)L.n_coef);
  return 0;
}

// host only: never initialises a GPU.  The size of groth16_ptau_prepare's file (ptau_prepare.hip).
__attribute__((visibility("default"))) int groth16_ptau_prepared_size(const void* ptau, size_t len, uint64_t* ptau_bytes)
{
  if (!ptau_bytes) return fail(ERR_ARG, "null output");
  *ptau_bytes = 0;
  std::vector<Section> secs;
  PtauLayout L;
  if (int rc = ptau_unprepared_layout((const uint8_t*)ptau, len, secs, &L)) return rc;
  uint64_t total = len;
  for (int sid = 12; sid < 16; sid++) total += 12 + ptau_prepared_section_bytes(L.power, sid);
  *ptau_bytes = total;
  return 0;
}

// host only: never initialise a GPU.  The sizes of groth16_ptau_pack's and groth16_ptau_unpack's files (ptau_pack.hip): whatever is
// no point section is carried over as it is, so the other form's size follows from (power, prepared, this form's size).
static int ptau_pack_sizes(uint32_t power, int prepared, uint64_t in_bytes, bool unpack, uint64_t* out_bytes)
{
  if (!out_bytes) return fail(ERR_ARG, "null output");
  *out_bytes = 0;
  if (power > 27) return fail(ERR_ARG, "ptau: power %u is above 27", power);
  uint64_t packed = 0;
  for (int sid = 2; sid < 16; sid++)
    if (sid <= 6 || (sid >= 12 && prepared)) packed += ptau_packed_section_bytes(power, sid);
  const uint64_t points_in = unpack ? packed : 2 * packed, least = 12 + 12 * (prepared ? 11 : 7) + 44 + points_in; // sections 1 to 7 (and 12 to 15)
  if (in_bytes < least) return fail(ERR_ARG, "ptau: a %s file of power %u has at least %llu bytes, not %llu", unpack ? "packed" : prepared ? "prepared" : "unprepared", power, (unsigned long long)least, (unsigned long long)in_bytes);
  *out_bytes = unpack ? in_bytes + packed : in_bytes - packed;
  return 0;
}
__attribute__((visibility("default"))) int groth16_ptau_packed_size(uint32_t power, int prepared, uint64_t ptau_bytes, uint64_t* packed_bytes)
{
  return ptau_pack_sizes(power, prepared, ptau_bytes, false, packed_bytes);
}
__attribute__((visibility("default"))) int groth16_ptau_unpacked_size(uint32_t power, int prepared, uint64_t packed_bytes, uint64_t* ptau_bytes)
{
  return ptau_pack_sizes(power, prepared, packed_bytes, true, ptau_bytes);
}
