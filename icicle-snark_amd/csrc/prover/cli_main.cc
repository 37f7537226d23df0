// prove — stdin REPL worker with the protocol of the reference CLI (src/main.rs:121-186):
//   > prove --witness W --zkey Z --proof P --public Q --device HIP
// prints COMMAND_COMPLETED after every command, COMMAND_EMPTY for blank lines, COMMAND_EXIT on "exit".  An unknown command, and a
// `prove` or `verify` with an unknown --system, print the help and no completion line.
// The commands are the entries of `commands` below: name, usage line (the help is assembled from them) and function.  A new command
// is one entry and one function; its options go through parse(), its failure line through report_failure().
#include <algorithm>
#include <fstream>
#include <initializer_list>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "groth16_prover.h"

struct Command;
struct Call {             // one command line, as the command's function sees it
  std::istringstream& in; // the tokens after the command's name
  const Command& cmd;     // the entry that was looked up
  Groth16CacheManager* cm;
  bool completed = true;  // cleared by an unknown --system alone: no completion line then
};
struct Command {
  const char* name;
  const char* usage;  // what follows the name in the help
  void (*run)(Call&); // null: a usage line only
  bool second;        // of a pair that shares a function: the unpack of pack / unpack, the r1cs-match of wtns-check / r1cs-match
};

static void print_help();

// --- shared pieces ---------------------------------------------------------------------------------------------------------------

// One option of a command: the flag and where its value goes.  A std::string or a long takes the next token, a bool is set by the
// flag alone, and no destination is --system, which takes a value and accepts only groth16.
struct Opt {
  const char* flag;
  std::string* text = nullptr;
  long* number = nullptr;
  bool* set = nullptr;
  Opt(const char* f, std::string* d) : flag(f), text(d) {}
  Opt(const char* f, long* d) : flag(f), number(d) {}
  Opt(const char* f, bool* d) : flag(f), set(d) {}
  Opt(const char* f) : flag(f) {}
};

// An unknown token prints the help and parsing goes on; a flag whose value is missing leaves the default; nothing is an error but
// an unknown proof system, which is false: the command does not run.
static bool parse(Call& c, std::initializer_list<Opt> opts)
{
  std::istringstream& in = c.in;
  std::string a, v;
  bool ok = true;
  while (in >> a) {
    const Opt* o = nullptr;
    for (const Opt& x : opts)
      if (a == x.flag) {
        o = &x;
        break;
      }
    if (!o) print_help();
    else if (o->text) in >> *o->text;
    else if (o->number) in >> *o->number;
    else if (o->set) *o->set = true;
    else if (in >> v && v != "groth16" && v != "Groth16" && v != "GROTH16") {
      std::cerr << "Unknown proof system: " << v << std::endl;
      ok = false;
    }
  }
  if (!ok) {
    print_help();
    c.completed = false;
  }
  return ok;
}

static bool read_file(const std::string& path, std::string* image)
{
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::ostringstream ss;
  ss << f.rdbuf();
  *image = ss.str();
  return true;
}

// the reference unwraps (aborts) where a call fails; report and keep the worker alive instead
static void report_failure(const std::string& name, long long rc, const char* text)
{
  std::cerr << name << " failed (" << rc << "): " << text << std::endl;
}

// The key's verification_key.json to vk_path (groth16_zkey_export_vk).  0 written; 1 the file cannot be written; below 0 the
// export's own code, its text in groth16_last_error().
static int64_t write_vk(const std::string& image, const std::string& vk_path)
{
  const int64_t need = groth16_zkey_export_vk(image.data(), image.size(), nullptr, 0);
  if (need < 0) return need;
  std::string text((size_t)need, '\0');
  (void)groth16_zkey_export_vk(image.data(), image.size(), &text[0], text.size());
  text.resize((size_t)need - 1);
  std::ofstream o(vk_path, std::ios::binary);
  o << text;
  return o ? 0 : 1;
}

// One line per record that is listed, then CHAIN_OK or CHAIN_BAD <kind> <index>: for section 10 of a key and section 7 of a
// powers-of-tau file, which differ in the point that is shown.  The verdict is over all records, listed or not.  A beacon record's
// line ends in " beacon <the 64 hex digits of its hash> <iter_exp>" (beacons: groth16_*_beacons' list).
template <class Report, class Info>
static void print_chain(int rc, const Report& rep, const std::vector<Info>& infos, uint8_t (Info::*shown)[64], const char* label, const std::vector<Groth16BeaconInfo>& beacons)
{
  static const char* const kinds[7] = {"", "SECTION", "POINT", "POK", "HEADER", "PAIR", "BEACON"};
  static const char hex[] = "0123456789abcdef";
  auto hex_of = [](const uint8_t* p, int n) {
    std::string d;
    for (int k = 0; k < n; k++) d += {hex[p[k] >> 4], hex[p[k] & 15]};
    return d;
  };
  const uint32_t held = rep.kind == GROTH16_CONTRIB_SECTION ? (rep.index ? rep.index - 1 : 0) : rep.count;
  size_t b = 0;
  for (uint32_t i = 0; i < held && i < infos.size(); i++) {
    std::cout << "contribution " << i + 1 << " name \"" << infos[i].name << "\" " << label << " " << hex_of(infos[i].*shown, 8) << "...";
    if (b < beacons.size() && beacons[b].index == i + 1) {
      std::cout << " beacon " << hex_of(beacons[b].hash, 32) << " " << beacons[b].iter_exp;
      b++;
    }
    std::cout << std::endl;
  }
  if (rc == 1) std::cout << "CHAIN_OK" << std::endl;
  else std::cout << "CHAIN_BAD " << kinds[rep.kind >= 1 && rep.kind <= 6 ? rep.kind : 0] << " " << rep.index << std::endl;
}

// the end of the summary line of a tool that writes a file; device_detail, when given, stands between the device and download times
template <class Report>
static void print_times(const Report& rep, const std::string& device_detail = std::string())
{
  std::cout << "; upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms " << device_detail << "download " << rep.download_ms << " ms write " << rep.write_ms << " ms"
            << std::endl;
}

struct R1cs { // a circuit on the device for the length of one command
  Groth16R1cs* h = nullptr;
  int load(const std::string& path, const std::string& device) { return groth16_r1cs_load_file(path.c_str(), device.c_str(), &h); }
  ~R1cs() { groth16_r1cs_free(h); }
};

// --- the commands ----------------------------------------------------------------------------------------------------------------

static void cmd_prove(Call& c)
{
  // defaults of src/main.rs:46-50, except the device: this build registers "HIP" ("CUDA" is an alias)
  std::string witness = "witness.wtns", zkey = "circuit_final.zkey", proof = "proof.json", pub = "public.json", device = "CUDA";
  if (!parse(c, {{"--system"}, {"--witness", &witness}, {"--zkey", &zkey}, {"--proof", &proof}, {"--public", &pub}, {"--device", &device}})) return;
  const int rc = groth16_prove(witness.c_str(), zkey.c_str(), proof.c_str(), pub.c_str(), device.c_str(), c.cm);
  if (rc != 0) report_failure(c.cmd.name, rc, groth16_last_error());
}

static void cmd_verify(Call& c)
{
  // defaults of src/main.rs:84-86
  std::string proof = "proof.json", pub = "public.json", vk = "verification_key.json";
  if (!parse(c, {{"--system"}, {"--proof", &proof}, {"--public", &pub}, {"--vk", &vk}})) return;
  const int rc = groth16_verify(proof.c_str(), pub.c_str(), vk.c_str());
  // the reference panics on a rejected proof (assert, src/lib.rs:79)
  if (rc == 0) std::cout << "VERIFY_OK" << std::endl;
  else {
    report_failure(c.cmd.name, rc, groth16_verify_last_error());
    std::cout << "VERIFY_FAILED" << std::endl;
  }
}

// every "<proof.json> <public.json>" line of the list against one key, on one GPU: one line per item, then the counts.
// --combined: one randomised pairing equation over the batch, the per-item stage only when it fails
static void cmd_verify_batch(Call& c)
{
  std::string list, vk = "verification_key.json", device = "HIP";
  bool combined = false;
  parse(c, {{"--list", &list}, {"--vk", &vk}, {"--device", &device}, {"--combined", &combined}});
  std::string vk_text, list_text;
  if (list.empty() || !read_file(list, &list_text) || !read_file(vk, &vk_text)) {
    std::cerr << "verify-batch: cannot read " << (list.empty() ? std::string("--list (missing)") : list) << " or " << vk << std::endl;
    return;
  }
  std::vector<std::string> proofs, publics;
  std::vector<int> readable; // 1: both files read; 0: reported as an error without being judged
  std::istringstream ls(list_text);
  std::string ln;
  while (std::getline(ls, ln)) {
    std::istringstream lf(ln);
    std::string pp, qp, pt, qt;
    if (!(lf >> pp)) continue; // blank line
    const bool ok = (lf >> qp) && read_file(pp, &pt) && read_file(qp, &qt);
    proofs.push_back(ok ? pt : std::string());
    publics.push_back(ok ? qt : std::string());
    readable.push_back(ok ? 1 : 0);
  }
  const int n = (int)proofs.size();
  std::vector<const char*> pj(n), qj(n);
  for (int i = 0; i < n; i++) {
    pj[i] = proofs[i].c_str();
    qj[i] = publics[i].c_str();
  }
  std::vector<int32_t> verdicts(n);
  int32_t path = 0;
  const int rc = combined ? groth16_verify_batch_combined(pj.data(), qj.data(), n, vk_text.c_str(), device.c_str(), nullptr, verdicts.data(), &path)
                          : groth16_verify_batch(pj.data(), qj.data(), n, vk_text.c_str(), device.c_str(), verdicts.data());
  if (rc != 0) return report_failure(c.cmd.name, rc, groth16_verify_last_error());
  int acc = 0, rej = 0, err = 0;
  for (int i = 0; i < n; i++) {
    if (!readable[i]) {
      std::cout << i << " error: cannot read input file" << std::endl;
      err++;
    } else if (verdicts[i] == 1) {
      std::cout << i << " accepted" << std::endl;
      acc++;
    } else if (verdicts[i] == 0) {
      std::cout << i << " rejected" << std::endl;
      rej++;
    } else {
      std::cout << i << " error: malformed proof or public signals (code " << verdicts[i] << ")" << std::endl;
      err++;
    }
  }
  std::cout << "accepted " << acc << " rejected " << rej << " errors " << err << std::endl;
  if (combined) std::cout << "decided by: " << (path ? "combined equation" : "per-item fallback") << std::endl;
}

// every point and record of the key tested on the GPU (groth16_zkey_check): one line per faulty section, then "sound" or "unsound"
static void cmd_zkey_check(Call& c)
{
  std::string zkey = "circuit_final.zkey", device = "HIP";
  parse(c, {{"--zkey", &zkey}, {"--device", &device}});
  Groth16ZkeyReport rep;
  const int rc = groth16_zkey_check_file(zkey.c_str(), device.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  static const char* const kinds[7] = {"", "non-canonical coordinate", "point off the curve", "point outside the subgroup", "identity", "pair mismatch", "coefficient out of range"};
  for (int s = 2; s < 10; s++) {
    if (!rep.faults[s]) continue;
    std::cout << "section " << s << ": " << rep.faults[s] << " at fault";
    if (s == rep.section) { // the report names kind and index of the first fault of the key
      std::cout << ", first: " << kinds[rep.kind >= 1 && rep.kind <= 6 ? rep.kind : 0];
      if (rep.index != UINT64_MAX) std::cout << " at index " << rep.index;
    }
    std::cout << std::endl;
  }
  std::cout << (rc == 1 ? "sound" : "unsound") << std::endl;
}

static void cmd_zkey_export_vk(Call& c)
{
  std::string zkey = "circuit_final.zkey", vk = "verification_key.json", image;
  parse(c, {{"--zkey", &zkey}, {"--vk", &vk}});
  const bool read = read_file(zkey, &image);
  const int64_t rc = read ? write_vk(image, vk) : -1;
  if (rc < 0) report_failure(c.cmd.name, rc, read ? groth16_last_error() : "cannot read the zkey");
  else if (rc > 0) std::cerr << "zkey-export-vk: cannot write " << vk << std::endl;
  else std::cout << "VK_WRITTEN" << std::endl;
}

// wtns-check: does the witness (--wtns, or packed: --wtnz) satisfy the circuit: "satisfied", or the first fault with the counts and
// "not satisfied".  r1cs-match (second): does the key carry the circuit's A and B
static void cmd_r1cs_against(Call& c)
{
  std::string r1cs = "circuit.r1cs", wtns = "witness.wtns", wtnz, zkey = "circuit_final.zkey", device = "HIP";
  parse(c, {{"--r1cs", &r1cs}, {"--wtns", &wtns}, {"--wtnz", &wtnz}, {"--zkey", &zkey}, {"--device", &device}});
  R1cs circuit;
  int rc = circuit.load(r1cs, device);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  if (!c.cmd.second) {
    Groth16WitnessReport rep;
    rc = wtnz.empty() ? groth16_witness_check_file(circuit.h, wtns.c_str(), &rep) : groth16_witness_check_packed_file(circuit.h, wtnz.c_str(), &rep);
    if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
    if (rep.kind == GROTH16_WTNS_NONCANONICAL) std::cout << rep.noncanonical << " values not below r, first: wire " << rep.index << std::endl;
    else if (rep.kind == GROTH16_WTNS_ONE) std::cout << "wire 0 is not 1" << std::endl;
    if (rep.failed) std::cout << rep.failed << " constraints violated" << (rep.kind == GROTH16_WTNS_CONSTRAINT ? ", first: constraint " + std::to_string(rep.index) : std::string()) << std::endl;
    std::cout << (rc == 1 ? "satisfied" : "not satisfied") << std::endl;
  } else {
    std::string image;
    const bool read = read_file(zkey, &image);
    Groth16R1csMatchReport rep;
    rc = read ? groth16_r1cs_match_zkey(circuit.h, image.data(), image.size(), nullptr, &rep) : -1;
    if (rc < 0) return report_failure(c.cmd.name, rc, read ? groth16_last_error() : "cannot read the zkey");
    static const char* const sizes[3] = {"n_vars against nWires", "n_public", "domain_size"};
    if (rep.kind == GROTH16_MATCH_SIZES) std::cout << "sizes differ: " << sizes[rep.index < 3 ? rep.index : 0] << std::endl;
    if (rep.rows_a) std::cout << rep.rows_a << " rows of A differ" << (rep.kind == GROTH16_MATCH_ROW_A ? ", first: row " + std::to_string(rep.index) : std::string()) << std::endl;
    if (rep.rows_b) std::cout << rep.rows_b << " rows of B differ" << (rep.kind == GROTH16_MATCH_ROW_B ? ", first: row " + std::to_string(rep.index) : std::string()) << std::endl;
    std::cout << (rc == 1 ? "match" : "no match") << std::endl;
  }
}

// the two questions `snarkjs zkey verify` asks of a key, one line each: section 4 against the circuit (r1cs-match), then the
// point sections against the circuit and the ceremony (groth16_zkey_verify_ptau); the first line stands even when the second fails
static void cmd_zkey_verify(Call& c)
{
  std::string r1cs = "circuit.r1cs", zkey = "circuit_final.zkey", ptau = "pot_final.ptau", device = "HIP", image;
  parse(c, {{"--r1cs", &r1cs}, {"--zkey", &zkey}, {"--ptau", &ptau}, {"--device", &device}});
  R1cs circuit;
  int rc = circuit.load(r1cs, device);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  const bool read = read_file(zkey, &image);
  Groth16R1csMatchReport mrep;
  const int mrc = read ? groth16_r1cs_match_zkey(circuit.h, image.data(), image.size(), nullptr, &mrep) : -1;
  if (mrc < 0) {
    report_failure("zkey-verify: r1cs-match", mrc, read ? groth16_last_error() : "cannot read the zkey");
  } else {
    static const char* const mkinds[4] = {"match", "no match: SIZES", "no match: ROW_A", "no match: ROW_B"};
    std::cout << "section 4 against the circuit: " << mkinds[mrep.kind >= 0 && mrep.kind <= 3 ? mrep.kind : 0] << std::endl;
  }
  Groth16ZkeyVerifyReport rep;
  rc = groth16_zkey_verify_ptau_file(circuit.h, zkey.c_str(), ptau.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  static const char* const kinds[10] = {"", "SIZES", "KEY", "HEADER", "A", "B1", "B2", "IC", "C", "H"};
  std::cout << "point sections against the circuit and the ptau: ";
  if (rc == 1) std::cout << "verified";
  else {
    std::cout << "not verified: " << kinds[rep.kind >= 1 && rep.kind <= 9 ? rep.kind : 0];
    if (rep.kind == GROTH16_VERIFY_SIZES || rep.kind == GROTH16_VERIFY_HEADER) std::cout << " " << rep.index;
    if (rep.kind == GROTH16_VERIFY_KEY) std::cout << " (zkey-check: kind " << rep.key.kind << ", section " << rep.key.section << ")";
    if (rep.failed_mask) {
      std::cout << ", failing:";
      for (int k = GROTH16_VERIFY_HEADER; k <= GROTH16_VERIFY_H; k++)
        if (rep.failed_mask >> (k - GROTH16_VERIFY_HEADER) & 1) std::cout << " " << kinds[k];
    }
  }
  std::cout << std::endl;
  std::cout << (rc == 1 && mrc == 1 ? "ZKEY_OK" : "ZKEY_NOT_OK") << std::endl;
}

// the sizes that zkey-new and zkey-setup report alike, up to the times
template <class Report>
static void print_key_sizes(const Report& rep)
{
  std::cout << "wires " << rep.n_vars << " public " << rep.n_public << " domain " << rep.domain << " coefficients " << rep.n_coeffs << " bytes " << rep.zkey_bytes
            << " longest column " << rep.longest_column << " heavy columns " << rep.heavy_columns << " in " << rep.heavy_items << " items";
}

// the circuit's key over the ceremony before any contribution, gamma = delta = 1 (groth16_zkey_new_file)
static void cmd_zkey_new(Call& c)
{
  std::string r1cs = "circuit.r1cs", zkey = "circuit_0000.zkey", ptau = "pot_final.ptau", device = "HIP";
  parse(c, {{"--r1cs", &r1cs}, {"--zkey", &zkey}, {"--ptau", &ptau}, {"--device", &device}});
  R1cs circuit;
  int rc = circuit.load(r1cs, device);
  Groth16ZkeyNewReport rep;
  if (rc == 0) rc = groth16_zkey_new_file(circuit.h, ptau.c_str(), zkey.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  print_key_sizes(rep);
  print_times(rep);
  std::cout << "ZKEY_WRITTEN" << std::endl;
}

// the circuit's key directly from fresh toxic waste (groth16_setup_file); the waste is the operating system's: none is taken from
// a command line.  --vk also writes the key's verification_key.json
static void cmd_zkey_setup(Call& c)
{
  std::string r1cs = "circuit.r1cs", zkey = "circuit_final.zkey", vk, device = "HIP";
  parse(c, {{"--r1cs", &r1cs}, {"--zkey", &zkey}, {"--vk", &vk}, {"--device", &device}});
  R1cs circuit;
  int rc = circuit.load(r1cs, device);
  Groth16SetupReport rep;
  if (rc == 0) rc = groth16_setup_file(circuit.h, nullptr, zkey.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  std::ostringstream stages;
  stages << "(lagrange " << rep.lagrange_ms << " columns " << rep.columns_ms << " G1 " << rep.g1_ms << " G2 " << rep.g2_ms << ") ";
  print_key_sizes(rep);
  print_times(rep, stages.str());
  std::cout << "single-party key: whoever ran this command can forge proofs for it; a key for third parties comes from the ceremony chain" << std::endl;
  int64_t vk_rc = 0;
  if (!vk.empty()) {
    std::string image;
    vk_rc = read_file(zkey, &image) ? write_vk(image, vk) : -1;
    if (vk_rc) std::cerr << "zkey-setup: cannot write " << vk << ": " << (vk_rc < 0 ? groth16_last_error() : "I/O") << std::endl;
  }
  std::cout << "ZKEY_WRITTEN" << std::endl;
  if (!vk.empty() && !vk_rc) std::cout << "VK_WRITTEN" << std::endl;
}

// one phase-2 contribution (groth16_zkey_contribute_file); the secret is the operating system's: none is taken from a command line
static void cmd_zkey_contribute(Call& c)
{
  std::string zkey = "circuit_0000.zkey", out = "circuit_0001.zkey", name, device = "HIP";
  parse(c, {{"--zkey", &zkey}, {"--out", &out}, {"--name", &name}, {"--device", &device}});
  Groth16ZkeyContributeReport rep;
  const int rc = groth16_zkey_contribute_file(zkey.c_str(), out.c_str(), nullptr, name.c_str(), device.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  std::cout << "contribution " << rep.contribution << " points C " << rep.points_c << " H " << rep.points_h << " bytes " << rep.zkey_bytes;
  print_times(rep);
  std::cout << "ZKEY_WRITTEN" << std::endl;
}

// the chain of section 10 and the header's delta pair, on the host; that C and H follow delta2 is zkey-verify's question
static void cmd_zkey_contributions(Call& c)
{
  std::string zkey = "circuit_final.zkey", image;
  parse(c, {{"--zkey", &zkey}});
  const bool read = read_file(zkey, &image);
  Groth16ContributionsReport rep;
  std::vector<Groth16ContributionInfo> infos(4096); // the records that are listed
  const int rc = read ? groth16_zkey_contributions(image.data(), image.size(), &rep, infos.data(), infos.size()) : -1;
  if (rc < 0) return report_failure(c.cmd.name, rc, read ? groth16_last_error() : "cannot read the zkey");
  std::vector<Groth16BeaconInfo> beacons(infos.size());
  const int n_beacons = groth16_zkey_beacons(image.data(), image.size(), beacons.data(), beacons.size());
  beacons.resize(std::min<size_t>(beacons.size(), (size_t)std::max(n_beacons, 0)));
  print_chain(rc, rep, infos, &Groth16ContributionInfo::after1, "delta1", beacons);
}

// sections 12 to 15 of a powers-of-tau file made from its sections 2 to 5 (groth16_ptau_prepare_file)
static void cmd_ptau_prepare(Call& c)
{
  std::string ptau = "pot.ptau", out = "pot_final.ptau", device = "HIP";
  parse(c, {{"--ptau", &ptau}, {"--out", &out}, {"--device", &device}});
  Groth16PtauPrepareReport rep;
  const int rc = groth16_ptau_prepare_file(ptau.c_str(), out.c_str(), device.c_str(), &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  std::cout << "power " << rep.power << " points " << rep.points[0] << " " << rep.points[1] << " " << rep.points[2] << " " << rep.points[3] << " bytes " << rep.ptau_bytes;
  print_times(rep);
  std::cout << "PTAU_WRITTEN" << std::endl;
}

static void cmd_ptau_new(Call& c)
{
  std::string out = "pot_0000.ptau";
  long power = -1;
  parse(c, {{"--power", &power}, {"--out", &out}});
  const bool bad_power = power < 0 || power > 64;
  const int rc = bad_power ? -3 : groth16_ptau_new_file((uint32_t)power, out.c_str());
  if (rc < 0) return report_failure(c.cmd.name, rc, bad_power ? "--power <P> is required, 0 to 27" : groth16_last_error());
  std::cout << "PTAU_WRITTEN" << std::endl;
}

// one phase-1 contribution (groth16_ptau_contribute_file); the secrets are the operating system's: none is taken from a command line
static void cmd_ptau_contribute(Call& c)
{
  std::string ptau = "pot_0000.ptau", out = "pot_0001.ptau", name, device = "HIP";
  parse(c, {{"--ptau", &ptau}, {"--out", &out}, {"--name", &name}, {"--device", &device}});
  Groth16PtauContributeReport rep;
  const int rc = groth16_ptau_contribute_file(ptau.c_str(), out.c_str(), nullptr, name.c_str(), device.c_str(), nullptr, &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  std::cout << "contribution " << rep.contribution << " power " << rep.power << " points " << rep.points[0] << " " << rep.points[1] << " " << rep.points[2] << " " << rep.points[3]
            << " bytes " << rep.ptau_bytes;
  print_times(rep);
  std::cout << "PTAU_WRITTEN" << std::endl;
}

// the chain of section 7 against the file's first elements, on the host; that the other powers follow is ptau-verify's question
static void cmd_ptau_contributions(Call& c)
{
  std::string ptau = "pot_final.ptau", image;
  parse(c, {{"--ptau", &ptau}});
  const bool read = read_file(ptau, &image);
  Groth16PtauContributionsReport rep;
  std::vector<Groth16PtauContributionInfo> infos(1024); // the records that are listed
  const int rc = read ? groth16_ptau_contributions(image.data(), image.size(), &rep, infos.data(), infos.size()) : -1;
  if (rc < 0) return report_failure(c.cmd.name, rc, read ? groth16_last_error() : "cannot read the ptau");
  std::vector<Groth16BeaconInfo> beacons(infos.size());
  const int n_beacons = groth16_ptau_beacons(image.data(), image.size(), beacons.data(), beacons.size());
  beacons.resize(std::min<size_t>(beacons.size(), (size_t)std::max(n_beacons, 0)));
  print_chain(rc, rep, infos, &Groth16PtauContributionInfo::tau1, "tau1", beacons);
}

// the audit first, as zkey-verify runs r1cs-match: who contributed, then whether the points are what they should be
// (groth16_ptau_verify_file): one line per question, then PTAU_OK or PTAU_BAD <kind> [<section> <element>]
static void cmd_ptau_verify(Call& c)
{
  std::string ptau = "pot_final.ptau", device = "HIP";
  parse(c, {{"--ptau", &ptau}, {"--device", &device}});
  static const char* const kinds[14] = {"", "GENERATORS", "TAU_PAIR", "BETA_PAIR", "TAU_G1", "TAU_G2", "ALPHA_TAU", "BETA_TAU", "LAGRANGE_12", "LAGRANGE_13", "LAGRANGE_14",
                                        "LAGRANGE_15", "POINT", "IDENTITY"};
  Groth16PtauVerifyReport rep;
  const int rc = groth16_ptau_verify_file(ptau.c_str(), nullptr, device.c_str(), &rep);
  if (rc < 0) return report_failure(c.cmd.name, rc, groth16_last_error());
  // the chain of section 7: the audit reads an unprepared file; for a prepared one it is said, not skipped silently
  int chain = -1;
  if (!rep.prepared) {
    std::string image;
    Groth16PtauContributionsReport crep = {};
    chain = read_file(ptau, &image) ? groth16_ptau_contributions(image.data(), image.size(), &crep, nullptr, 0) : -1;
    std::cout << "contributions: " << (chain == 1 ? "the chain holds" : chain == 0 ? "the chain does NOT hold" : "not read") << ", " << crep.count << " records" << std::endl;
  } else {
    std::cout << "contributions: not audited (groth16_ptau_contributions reads the unprepared file)" << std::endl;
  }
  const uint32_t powers_mask = rep.failed_mask & 0x7f, lagrange_mask = rep.failed_mask >> 7;
  const bool point = rep.kind == GROTH16_PTAU_VERIFY_POINT || rep.kind == GROTH16_PTAU_VERIFY_IDENTITY;
  auto names = [&](uint32_t mask, int first) {
    std::string out;
    for (int b = 0; b < 11; b++)
      if (mask >> b & 1) out += std::string(" ") + kinds[first + b];
    return out;
  };
  std::cout << "power " << rep.power << ", sections 2 to 6 are the powers of one (tau, alpha, beta): "
            << (point ? "not decided" : powers_mask ? "NO:" + names(powers_mask, 1) : std::string("yes")) << std::endl;
  if (rep.prepared)
    std::cout << "sections 12 to 15 are the transforms of 2 to 5: " << (point ? "not decided" : lagrange_mask ? "NO:" + names(lagrange_mask, 8) : std::string("yes")) << std::endl;
  std::cout << "upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms pairing " << rep.pairing_ms << " ms" << std::endl;
  if (rc == 1 && chain != 0) std::cout << "PTAU_OK" << std::endl;
  else if (rc == 1) std::cout << "PTAU_BAD CHAIN" << std::endl;
  else if (point) std::cout << "PTAU_BAD " << kinds[rep.kind] << " " << rep.fault_section << " " << rep.fault_index << std::endl;
  else std::cout << "PTAU_BAD " << kinds[rep.kind >= 1 && rep.kind <= 13 ? rep.kind : 0] << std::endl;
}

// the file with every point as x and one bit of y (groth16_ptau_pack_file), and back, byte for byte (second: groth16_ptau_unpack_file)
static void cmd_ptau_pack(Call& c)
{
  const bool unpack = c.cmd.second;
  std::string inp = unpack ? "pot_final.ptaz" : "pot_final.ptau", out = unpack ? "pot_final.ptau" : "pot_final.ptaz", device = "HIP";
  parse(c, {{unpack ? "--packed" : "--ptau", &inp}, {"--out", &out}, {"--device", &device}});
  Groth16PtauPackReport rep = {};
  const int rc = (unpack ? groth16_ptau_unpack_file : groth16_ptau_pack_file)(inp.c_str(), out.c_str(), device.c_str(), &rep);
  if (rc < 0) {
    report_failure(c.cmd.name, rc, groth16_last_error());
    if (rep.fault_kind) std::cout << "PTAU_BAD POINT " << rep.fault_section << " " << rep.fault_index << std::endl;
    return;
  }
  std::cout << "power " << rep.power << (rep.prepared ? " prepared" : " unprepared") << " points " << rep.points[0] << " " << rep.points[1] << " bytes " << rep.in_bytes << " to "
            << rep.out_bytes;
  print_times(rep);
  std::cout << "PTAU_WRITTEN" << std::endl;
}

// the file of power p <= the input's: prefixes of the sections, and section 12's block p + 1 fixed up on the GPU
// (groth16_ptau_truncate_file; an unprepared input opens no GPU)
static void cmd_ptau_truncate(Call& c)
{
  std::string inp = "pot_final.ptau", out = "pot_cut.ptau", device = "HIP";
  long power = -1;
  parse(c, {{"--ptau", &inp}, {"--power", &power}, {"--out", &out}, {"--device", &device}});
  Groth16PtauTruncateReport rep = {};
  const bool bad_power = power < 0 || power > 64;
  const int rc = bad_power ? -3 : groth16_ptau_truncate_file(inp.c_str(), out.c_str(), (uint32_t)power, device.c_str(), &rep);
  if (rc < 0) {
    report_failure(c.cmd.name, rc, bad_power ? "--power <p> is required, 0 to the file's power" : groth16_last_error());
    if (rep.fault_kind) std::cout << "PTAU_BAD POINT " << rep.fault_section << " " << rep.fault_index << " " << rep.fault_count << std::endl;
    return;
  }
  std::cout << "power " << rep.power_in << " to " << rep.power_out << (rep.prepared ? " prepared" : " unprepared") << " fixed " << rep.points_fixed << " bytes " << rep.in_bytes << " to "
            << rep.out_bytes;
  print_times(rep);
  std::cout << "PTAU_WRITTEN" << std::endl;
}

// the witness with a code byte per value and only its significant bytes, on the host (groth16_wtns_pack_file), and back (second):
// on the host too (groth16_wtns_unpack_host_file) unless --device names a GPU (groth16_wtns_unpack_file)
static void cmd_wtns_pack(Call& c)
{
  const bool unpack = c.cmd.second;
  std::string inp = unpack ? "witness.wtnz" : "witness.wtns", out = unpack ? "witness.wtns" : "witness.wtnz", device;
  // "" matches no token: --device is unknown to wtns-pack
  parse(c, {{unpack ? "--packed" : "--wtns", &inp}, {"--out", &out}, {unpack ? "--device" : "", &device}});
  Groth16WtnsPackReport rep = {};
  const int rc = !unpack          ? groth16_wtns_pack_file(inp.c_str(), out.c_str(), &rep)
                 : device.empty() ? groth16_wtns_unpack_host_file(inp.c_str(), out.c_str(), &rep)
                                  : groth16_wtns_unpack_file(inp.c_str(), out.c_str(), device.c_str(), &rep);
  if (rc < 0) {
    report_failure(c.cmd.name, rc, groth16_last_error());
    if (rep.fault_kind) std::cout << "WTNS_BAD VALUE " << rep.fault_index << " " << rep.fault_count << std::endl;
    return;
  }
  std::cout << "values " << rep.n_witness << " bytes " << rep.in_bytes << " to " << rep.out_bytes;
  if (!device.empty()) std::cout << "; upload " << rep.upload_ms << " ms kernel " << rep.kernel_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms";
  std::cout << " write " << rep.write_ms << " ms" << std::endl;
  std::cout << "WTNS_WRITTEN" << std::endl;
}

// prove from a packed witness (groth16_prove_packed_files)
static void cmd_prove_packed(Call& c)
{
  std::string witness = "witness.wtnz", zkey = "circuit_final.zkey", proof = "proof.json", pub = "public.json", device = "HIP";
  parse(c, {{"--witness", &witness}, {"--zkey", &zkey}, {"--proof", &proof}, {"--public", &pub}, {"--device", &device}});
  const int rc = groth16_prove_packed_files(witness.c_str(), zkey.c_str(), proof.c_str(), pub.c_str(), device.c_str(), c.cm);
  if (rc != 0) report_failure(c.cmd.name, rc, groth16_last_error());
}

// the key with every point as x and one bit of y and every coefficient as a code byte and its significant bytes
// (groth16_zkey_pack_file), and back, byte for byte (second: groth16_zkey_unpack_file)
static void cmd_zkey_pack(Call& c)
{
  const bool unpack = c.cmd.second;
  std::string inp = unpack ? "circuit_final.zkez" : "circuit_final.zkey", out = unpack ? "circuit_final.zkey" : "circuit_final.zkez", device = "HIP";
  parse(c, {{unpack ? "--packed" : "--zkey", &inp}, {"--out", &out}, {"--device", &device}});
  Groth16ZkeyPackReport rep = {};
  const int rc = (unpack ? groth16_zkey_unpack_file : groth16_zkey_pack_file)(inp.c_str(), out.c_str(), device.c_str(), &rep);
  if (rc < 0) {
    report_failure(c.cmd.name, rc, groth16_last_error());
    if (rep.fault_kind && rep.fault_section == 4) std::cout << "ZKEY_BAD COEFFICIENT " << rep.fault_index << " " << rep.fault_count << std::endl;
    else if (rep.fault_kind) std::cout << "ZKEY_BAD POINT " << rep.fault_section << " " << rep.fault_index << " " << rep.fault_count << std::endl;
    return;
  }
  std::cout << "wires " << rep.n_vars << " domain " << rep.domain << " coefficients " << rep.n_coef << " points " << rep.points[0] << " " << rep.points[1] << " bytes " << rep.in_bytes
            << " to " << rep.out_bytes << " (packed points " << rep.point_bytes << " section 4 " << rep.coef_bytes << ")";
  print_times(rep);
  std::cout << "ZKEY_WRITTEN" << std::endl;
}

// prove from a packed key (groth16_prove_zkez_files)
static void cmd_prove_zkez(Call& c)
{
  std::string witness = "witness.wtns", zkez = "circuit_final.zkez", proof = "proof.json", pub = "public.json", device = "HIP";
  parse(c, {{"--witness", &witness}, {"--zkez", &zkez}, {"--proof", &proof}, {"--public", &pub}, {"--device", &device}});
  const int rc = groth16_prove_zkez_files(witness.c_str(), zkez.c_str(), proof.c_str(), pub.c_str(), device.c_str(), c.cm);
  if (rc != 0) report_failure(c.cmd.name, rc, groth16_last_error());
}

// --- the table: the help lists it in this order; the first entry of a name that has a function runs -------------------------------

static const Command commands[] = {
  {"prove", "[--system groth16] --witness <file> --zkey <file> --proof <file> --public <file> --device <HIP>", cmd_prove, false},
  {"verify", "[--system groth16] --proof <file> --public <file> --vk <file>", cmd_verify, false},
  {"verify-batch", "--list <file> --vk <file> [--device HIP] [--combined]", cmd_verify_batch, false},
  {"zkey-check", "--zkey <file> [--device HIP]", cmd_zkey_check, false},
  {"zkey-export-vk", "--zkey <file> --vk <file>", cmd_zkey_export_vk, false},
  {"wtns-check", "--r1cs <file> --wtns <file> [--device HIP]", cmd_r1cs_against, false},
  {"r1cs-match", "--r1cs <file> --zkey <file> [--device HIP]", cmd_r1cs_against, true},
  {"zkey-verify", "--r1cs <file> --zkey <file> --ptau <file> [--device HIP]", cmd_zkey_verify, false},
  {"zkey-new", "--r1cs <file> --ptau <file> --zkey <file> [--device HIP]", cmd_zkey_new, false},
  {"zkey-setup", "--r1cs <file> --zkey <file> [--vk <file>] [--device HIP]   (a single-party key from the operating system's randomness: whoever runs it can forge proofs)",
   cmd_zkey_setup, false},
  {"zkey-contribute", "--zkey <file> --out <file> [--name <text>] [--device HIP]   (the secret is the operating system's)", cmd_zkey_contribute, false},
  {"zkey-contributions", "--zkey <file>   (section 10's chain and the header's delta; that C and H follow delta2 is zkey-verify's)", cmd_zkey_contributions, false},
  {"ptau-prepare", "--ptau <file> --out <file> [--device HIP]   (sections 12 to 15 from 2 to 5: powersoftau prepare phase2)", cmd_ptau_prepare, false},
  {"ptau-new", "--power <P> --out <file>   (the starting file of a ceremony: tau = alpha = beta = 1)", cmd_ptau_new, false},
  {"ptau-contribute", "--ptau <file> --out <file> [--name <text>] [--device HIP]   (the secrets are the operating system's)", cmd_ptau_contribute, false},
  {"ptau-contributions", "--ptau <file>   (section 7's chain and the file's first elements; that the other powers follow is ptau-verify's)", cmd_ptau_contributions, false},
  {"ptau-verify", "--ptau <file> [--device HIP]   (the contributions, then every power against the others and sections 12 to 15 against 2 to 5)", cmd_ptau_verify, false},
  {"ptau-pack", "--ptau <file> --out <file> [--device HIP]   (every point as x and one bit of y: half the bytes)", cmd_ptau_pack, false},
  {"ptau-unpack", "--packed <file> --out <file> [--device HIP]   (the .ptau back, byte for byte; a root per point)", cmd_ptau_pack, true},
  {"ptau-truncate", "--ptau <file> --power <p> --out <file> [--device HIP]   (the file of a lower power; section 12's last block fixed up)", cmd_ptau_truncate, false},
  {"wtns-pack", "--wtns <file> --out <file>   (a code byte per value and only its significant bytes; on the host)", cmd_wtns_pack, false},
  {"wtns-unpack", "--packed <file> --out <file> [--device HIP]   (the .wtns back; without --device on the host)", cmd_wtns_pack, true},
  {"prove-packed", "--witness <packed file> --zkey <file> --proof <file> --public <file> [--device HIP]", cmd_prove_packed, false},
  {"wtns-check", "--r1cs <file> --wtnz <packed file> [--device HIP]", nullptr, false},
  {"zkey-pack", "--zkey <file> --out <file> [--device HIP]   (points as x and one bit of y, coefficients as a code byte and their significant bytes)", cmd_zkey_pack, false},
  {"zkey-unpack", "--packed <file> --out <file> [--device HIP]   (the .zkey back, byte for byte)", cmd_zkey_pack, true},
  {"prove-zkez", "--witness <file> --zkez <packed key> --proof <file> --public <file> [--device HIP]", cmd_prove_zkez, false},
  {"exit", "", nullptr, false}, // the loop's own
};

static void print_help()
{
  std::cout << "Usage:\n";
  for (const Command& c : commands) std::cout << "  " << c.name << (*c.usage ? " " : "") << c.usage << "\n";
}

int main()
{
  Groth16CacheManager* cm = groth16_cache_manager_new();
  {
    // the device the first `prove` will most likely name ("HIP" → device 0, or the first of ICICLE_SNARK_DEVICES): its streams
    // and staging buffers are created while the worker waits for its first command
    int ids[1] = {0};
    if (groth16_parse_device("HIP", ids, 1) >= 1) groth16_cache_manager_prewarm(cm, ids[0]);
  }
  std::string line;
  for (;;) {
    std::cout << "> " << std::flush;
    if (!std::getline(std::cin, line)) break;
    std::istringstream in(line);
    std::string cmd;
    const bool blank = !(in >> cmd), leave = cmd == "exit" || cmd == "EXIT" || cmd == "Exit";
    const Command* found = nullptr;
    for (const Command& c : commands)
      if (!found && c.run && cmd == c.name) found = &c;
    bool completed = true;
    if (blank) std::cout << "COMMAND_EMPTY\n";
    else if (leave) std::cout << "COMMAND_EXIT\n";
    else if (found) {
      Call call{in, *found, cm};
      found->run(call);
      completed = call.completed;
    } else {
      print_help();
      completed = false;
    }
    if (completed) std::cout << "COMMAND_COMPLETED" << std::endl;
    if (leave) break;
  }
  std::cout << "Exiting CLI worker..." << std::endl;
  groth16_cache_manager_free(cm);
  return 0;
}
