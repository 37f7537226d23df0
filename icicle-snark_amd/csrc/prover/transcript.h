// transcript.h — the Fiat–Shamir transcript of a ceremony contribution, host only: what groth16_ptau_contribute / _contributions
// (ptau_contribute.hip) and groth16_zkey_contribute / _contributions (zkey_contribute.hip; §7f) say the same way, in ONE
// text — the scalars a secret is hashed to, the challenge of a digest, the walk over a section of records, the Schnorr response and the
// proof-of-knowledge test of the audit, and a file's point as the host pairing takes it (ptau_verify.hip still has a copy of that
// one, std_g1 / std_g2: DESIGN.md §7i says why).  What differs between the two ceremonies stays in the tools: the tags, the record
// layouts, chain_start, what a chain_step feeds the hash, the header rule and the secrets.  A random beacon is the
// same in both: the digest its public value is stretched to, and the flag and the trailer that mark its record.
// No HIP types, no worker pool: the .hip files and the F29_CHECK host build (tests/transcript_check.cpp) compile the same code.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../../include/icicle_snark_hip.h"
#include "sha256.h"
#include "zkey_check29.h"
#include "zkey_contribute29.h"

namespace isnark {
namespace transcript {

using namespace bn254;
using bn254::zc29::ZcDigits;

constexpr uint32_t NAME_BYTES_MAX = 255;
// A beacon record sets bit 31 of its stored name_len word, and beacon_hash (32 B) ‖ iter_exp (u32 LE) follow its name.
constexpr uint32_t BEACON_FLAG = (uint32_t)1 << 31;
constexpr size_t BEACON_TRAILER = 36;
// A condition, not a measurement: what a hostile record can make the audit hash, 2^24 per record and 2^25 per file.
constexpr uint32_t BEACON_ITER_EXP_MAX = 24;
constexpr uint64_t BEACON_WORK_MAX = (uint64_t)1 << 25;

// ---- scalars: standard form, below r
inline fe fr_mul(const fe& a, const fe& b) { return Fr::mul(Fr::to_mont(a), b); }
inline fe fr_inv(const fe& a) { return Fr::from_mont(Fr::inv(Fr::to_mont(a))); }
// a big-endian integer of `len` bytes mod r, by Horner's rule in additions
inline fe fr_from_be(const uint8_t* b, size_t len)
{
  fe acc = Fr::zero();
  for (size_t i = 0; i < len; i++) {
    for (int k = 0; k < 8; k++) acc = Fr::dbl(acc);
    fe d = Fr::zero();
    d.l[0] = b[i];
    acc = Fr::add(acc, d);
  }
  return acc;
}
// W(x) = SHA-256(x ‖ 0x00) ‖ SHA-256(x ‖ 0x01) as a 512-bit big-endian integer, mod r.  x is wiped: it holds the secret.
inline fe wide_hash(std::vector<uint8_t>& x)
{
  uint8_t d[64];
  x.push_back(0);
  sha256(x.data(), x.size(), d);
  x.back() = 1;
  sha256(x.data(), x.size(), d + 32);
  const fe v = fr_from_be(d, 64);
  explicit_bzero(d, sizeof d);
  explicit_bzero(x.data(), x.size());
  return v;
}
inline void append(std::vector<uint8_t>& v, const void* p, size_t n) { v.insert(v.end(), (const uint8_t*)p, (const uint8_t*)p + n); }
// The beacon's digest: d₀ = hash, d_{j+1} = SHA-256(d_j), out = d at j = 2^iter_exp (iter_exp = 0: one hash).  Sequential by design;
// the caller bounds iter_exp (BEACON_ITER_EXP_MAX).  The digest is public: a beacon's secrets are a contribution's with secret := digest.
inline void beacon_digest(const uint8_t hash[32], uint32_t iter_exp, uint8_t out[32])
{
  uint8_t d[32];
  memcpy(d, hash, 32);
  for (uint64_t j = 0, n = (uint64_t)1 << iter_exp; j < n; j++) sha256(d, 32, d);
  memcpy(out, d, 32);
}

// ---- the chain
// the challenge of a digest: its first 16 bytes, little-endian, 0 → 1
inline fe challenge_from_digest(const uint8_t digest[32])
{
  uint8_t c16[16];
  combined_coefficient_from_digest(digest, c16);
  fe c = Fr::zero();
  memcpy(c.l, c16, 16);
  return c;
}
// the end of a chain_step: SHA-256(m) → h (m may have begun with h), its challenge → *c
inline void hash_step(const std::vector<uint8_t>& m, uint8_t h[32], fe* c)
{
  sha256(m.data(), m.size(), h);
  *c = challenge_from_digest(h);
}

// A record of a contributions section: `fixed` bytes, the u32 name_len word at byte name_len_off of them (the last four), then the
// name; a beacon record (bit 31 of the word) has its trailer behind the name.
struct Record {
  const uint8_t* p;
  uint32_t name_len;                // the name's bytes: the word's low bits
  bool beacon = false;
  const uint8_t* trailer = nullptr; // beacon_hash ‖ iter_exp, when beacon
};
// what a chain_step hashes from the name_len word on: the word AS STORED, the name, a beacon's trailer
inline size_t hashed_tail(const Record& r) { return 4 + r.name_len + (r.beacon ? BEACON_TRAILER : 0); }
inline uint32_t beacon_iter_exp(const Record& r)
{
  uint32_t e;
  memcpy(&e, r.trailer + 32, 4);
  return e;
}
// The records of a section {u32 count, records} (sec->p, sec->size; sec null: no section, no records).  0, or 1 with *bad = the
// record that does not fit (0: the count); recs holds the records before it.  A word with any bit above bit 8 other than bit 31
// does not fit, nor does a trailer that is cut short.
template <class S>
int walk_records(const S* sec, size_t fixed, size_t name_len_off, std::vector<Record>& recs, uint32_t* count, uint32_t* bad)
{
  recs.clear();
  *count = 0, *bad = 0;
  if (!sec) return 0;
  if (sec->size < 4) return 1;
  uint32_t n;
  memcpy(&n, sec->p, 4);
  if ((uint64_t)n * fixed > sec->size - 4) return 1; // (a hostile count sizes nothing)
  *count = n;
  uint64_t pos = 4;
  for (uint32_t i = 0; i < n; i++) {
    *bad = i + 1;
    if (sec->size - pos < fixed) return 1;
    Record r;
    r.p = sec->p + pos;
    uint32_t word;
    memcpy(&word, r.p + name_len_off, 4);
    r.beacon = (word & BEACON_FLAG) != 0;
    r.name_len = word & ~BEACON_FLAG;
    const uint64_t behind = (uint64_t)r.name_len + (r.beacon ? BEACON_TRAILER : 0);
    if (r.name_len > NAME_BYTES_MAX || sec->size - pos - fixed < behind) return 1;
    if (r.beacon) r.trailer = r.p + fixed + r.name_len;
    recs.push_back(r);
    pos += fixed + behind;
  }
  *bad = n;
  return pos == sec->size ? 0 : 1; // bytes behind the last record
}
// The records an audit lists behind a walk: all of them, or after a SECTION fault those BEFORE the record at fault (bad − 1 of them;
// none for the count) — also where the fault is bytes behind the last record, whose own bounds hold.
inline std::vector<Record>& held_records(std::vector<Record>& recs, int malformed, uint32_t bad)
{
  if (malformed) recs.resize(bad ? bad - 1 : 0);
  return recs;
}
// The flagged records among recs as Groth16BeaconInfo {index from 1, hash, iter_exp}: the first min(their number, cap) to infos (may
// be null) → their number.  Bounds only: nothing is verified.
template <class Info>
int list_beacons(const std::vector<Record>& recs, Info* infos, size_t cap)
{
  size_t n = 0;
  for (size_t i = 0; i < recs.size(); i++) {
    if (!recs[i].beacon) continue;
    if (infos && n < cap) {
      infos[n].index = (uint32_t)(i + 1);
      memcpy(infos[n].hash, recs[i].trailer, 32);
      infos[n].iter_exp = beacon_iter_exp(recs[i]);
    }
    n++;
  }
  return (int)n;
}
// What a beacon call was given; null where a participant contributes.
struct Beacon {
  const uint8_t* hash; // 32 bytes
  uint32_t iter_exp;
};
// the bytes of a new record behind its fixed part
inline size_t tail_bytes(size_t name_len, const Beacon* b) { return name_len + (b ? BEACON_TRAILER : 0); }
// The end of a record being written at rec: the name_len word (the last four of the fixed bytes), the name, a beacon's trailer.
// → the record as walk_records would hand it to a chain_step.
inline Record put_tail(uint8_t* rec, size_t name_len_off, const char* name, size_t name_len, const Beacon* b)
{
  const uint32_t word = (uint32_t)name_len | (b ? BEACON_FLAG : 0);
  uint8_t* const w = rec + name_len_off;
  memcpy(w, &word, 4);
  memcpy(w + 4, name, name_len);
  Record r = {rec, (uint32_t)name_len};
  if (b) {
    uint8_t* const t = w + 4 + name_len;
    memcpy(t, b->hash, 32);
    memcpy(t + 32, &b->iter_exp, 4);
    r.beacon = true, r.trailer = t;
  }
  return r;
}
// The audit's work bound for a beacon record, ahead of any hashing: iter_exp ≤ BEACON_ITER_EXP_MAX, and the file's running total
// Σ 2^iter_exp (*work, kept by the caller across the records) at most BEACON_WORK_MAX.
inline bool beacon_work_allowed(uint32_t iter_exp, uint64_t* work)
{
  if (iter_exp > BEACON_ITER_EXP_MAX) return false;
  *work += (uint64_t)1 << iter_exp;
  return *work <= BEACON_WORK_MAX;
}

// ---- the proof of knowledge of x with after = x·cur: commitment R = k·before, challenge c, response z
inline fe schnorr_response(const fe& k, const fe& c, const fe& x) { return Fr::add(k, fr_mul(c, x)); }
// z canonical and z·before = R + c·after, compared in the file's canonical affine form (R the identity: nothing is added)
inline bool pok_holds(const G1::A& before, const G1::A& after, const G1::A& commitment, const fe& z, const ZcDigits& c)
{
  if (!Fr::is_canonical(z)) return false;
  const G1::A lhs = zc29::zc_mul_affine<G1, G1L>(before, z);
  G1L::X acc = zc29::zc_scale<G1L>(after, c);
  if (!G1::aff_is_zero(commitment)) G1L::x_madd(acc, G1L::load_affine(commitment, G1L::MONT256, false));
  const G1::A rhs = G1::p_to_affine(G1::x_to_projective(G1L::x_store(acc)));
  return memcmp(&lhs, &rhs, sizeof lhs) == 0;
}

// ---- a file's points (affine, Montgomery form, the identity all zero)
template <class A>
A point_at(const uint8_t* p)
{
  A a;
  memcpy(&a, p, sizeof a);
  return a;
}
// the lane test (zkey_check29.h) of one point
inline int classify(const G1::A& a)
{
  const fe w[2] = {a.x, a.y};
  return p29::classify_g1(w);
}
inline int classify(const G2::A& a)
{
  const fe2 w[2] = {a.x, a.y};
  return p29::classify_g2(w);
}
// as the host pairing takes it: standard form
inline bn254_affine_t std_affine(const G1::A& a)
{
  const G1::A s = {Fq::from_mont(a.x), Fq::from_mont(a.y)};
  bn254_affine_t p;
  memcpy(&p, &s, sizeof p);
  return p;
}
inline bn254_g2_affine_t std_affine(const G2::A& a)
{
  const G2::A s = {Fq2Ops::from_mont(a.x), Fq2Ops::from_mont(a.y)};
  bn254_g2_affine_t p;
  memcpy(&p, &s, sizeof p);
  return p;
}

} // namespace transcript
} // namespace isnark
