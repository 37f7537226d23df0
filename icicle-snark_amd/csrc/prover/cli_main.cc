// prove — stdin REPL worker with the protocol of the reference CLI (src/main.rs:121-186):
//   > prove --witness W --zkey Z --proof P --public Q --device HIP
// prints COMMAND_COMPLETED after every command, COMMAND_EMPTY for blank lines, COMMAND_EXIT on "exit".
//   > verify --proof P --public Q --vk verification_key.json
//   > verify-batch --list L --vk verification_key.json [--device HIP] [--combined]   (L: one "<proof.json> <public.json>" per line;
//     --combined: one randomised pairing equation over the batch, the per-item stage only when it fails)
//   > zkey-check --zkey Z [--device HIP]       every point and record of the key tested on the GPU (groth16_zkey_check): one line per
//     faulty section, then "sound" or "unsound"
//   > zkey-export-vk --zkey Z --vk OUT         the key's verification_key.json (groth16_zkey_export_vk)
//   > wtns-check --r1cs R --wtns W [--device HIP]    does the witness satisfy the circuit (groth16_witness_check): "satisfied", or
//     the first fault with the counts and "not satisfied"
//   > r1cs-match --r1cs R --zkey Z [--device HIP]    does the key carry the circuit's A and B (groth16_r1cs_match_zkey)
//   > zkey-verify --r1cs R --zkey Z --ptau P [--device HIP]   r1cs-match, then the point sections against circuit and ceremony (groth16_zkey_verify_ptau)
//   > zkey-new --r1cs R --ptau P --zkey OUT [--device HIP]    the circuit's key over the ceremony before any contribution, gamma = delta = 1
//     (groth16_zkey_new_file): one line with sizes and times, then ZKEY_WRITTEN
//   > zkey-setup --r1cs R --zkey OUT [--vk VK] [--device HIP]    the circuit's key directly from fresh toxic waste of the operating
//     system's (groth16_setup_file): one summary line, a line saying that this is a single-party key, then ZKEY_WRITTEN; --vk also
//     writes the key's verification_key.json
//   > zkey-contribute --zkey Z --out OUT [--name N] [--device HIP]    one phase-2 contribution with a secret from the operating system
//     (groth16_zkey_contribute_file): one summary line, then ZKEY_WRITTEN
//   > zkey-contributions --zkey Z             section 10's chain and the header's delta pair, on the host (groth16_zkey_contributions):
//     one line per record, then CHAIN_OK or CHAIN_BAD <kind> <index>.  It does not show that C and H follow delta2: zkey-verify does
//   > ptau-prepare --ptau IN --out OUT [--device HIP]    sections 12 to 15 of a powers-of-tau file made from its sections 2 to 5
//     (groth16_ptau_prepare_file, snarkjs' `powersoftau prepare phase2`): one summary line, then PTAU_WRITTEN
//   > ptau-new --power P --out OUT            the starting file of a ceremony, tau = alpha = beta = 1 (groth16_ptau_new_file): PTAU_WRITTEN
//   > ptau-contribute --ptau IN --out OUT [--name N] [--device HIP]    one phase-1 contribution with secrets from the operating system
//     (groth16_ptau_contribute_file): one summary line, then PTAU_WRITTEN
//   > ptau-contributions --ptau P             section 7's chain against the file's first elements, on the host (groth16_ptau_contributions):
//     one line per record, then CHAIN_OK or CHAIN_BAD <kind> <index>.  It does not show that the other powers follow: ptau-verify does
//   > ptau-verify --ptau P [--device HIP]     ptau-contributions (an unprepared file), then the powers of sections 2 to 6 against one
//     another and sections 12 to 15 against them (groth16_ptau_verify_file): one line per question, then PTAU_OK or
//     PTAU_BAD <kind> [<section> <element>]
//   > ptau-pack --ptau IN --out OUT [--device HIP]       the file with every point as x and one bit of y, half the bytes
//     (groth16_ptau_pack_file): one summary line, then PTAU_WRITTEN; a faulty point: PTAU_BAD POINT <section> <element>
//   > ptau-unpack --packed IN --out OUT [--device HIP]   the .ptau back, byte for byte (groth16_ptau_unpack_file): the same lines
//   > ptau-truncate --ptau IN --power p --out OUT [--device HIP]   the file of power p <= the input's: prefixes of the sections, and
//     section 12's block p + 1 fixed up on the GPU (groth16_ptau_truncate_file; an unprepared input opens no GPU): one summary line,
//     then PTAU_WRITTEN; a faulty point: PTAU_BAD POINT <section> <element> <count>
//   > wtns-pack --wtns W --out Z              the witness with a code byte per value and only its significant bytes, on the host
//     (groth16_wtns_pack_file): one summary line, then WTNS_WRITTEN; a value >= r: WTNS_BAD VALUE <element> <count>
//   > wtns-unpack --packed Z --out W [--device HIP]   the .wtns back; on the host, or with --device decoded on the GPU
//     (groth16_wtns_unpack_host_file / groth16_wtns_unpack_file): the same lines
//   > prove-packed --witness Z --zkey K --proof P --public Q [--device HIP]   prove from a packed witness (groth16_prove_packed_files)
//   > wtns-check --r1cs R --wtnz Z [--device HIP]     wtns-check from a packed witness (groth16_witness_check_packed_file)
//   > zkey-pack --zkey IN --out OUT [--device HIP]       the key with every point as x and one bit of y and every coefficient as a code
//     byte and its significant bytes (groth16_zkey_pack_file): one summary line, then ZKEY_WRITTEN; a fault:
//     ZKEY_BAD POINT <section> <element> <count> or ZKEY_BAD COEFFICIENT <element> <count>
//   > zkey-unpack --packed IN --out OUT [--device HIP]   the .zkey back, byte for byte (groth16_zkey_unpack_file): the same lines
//   > prove-zkez --witness W --zkez Z --proof P --public Q [--device HIP]   prove from a packed key (groth16_prove_zkez_files)
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "groth16_prover.h"

static void print_help()
{
  std::cout << "Usage:\n  prove [--system groth16] --witness <file> --zkey <file> --proof <file> --public <file> --device <HIP>\n  verify [--system groth16] --proof <file> --public <file> --vk <file>\n  verify-batch --list <file> --vk <file> [--device HIP] [--combined]\n  zkey-check --zkey <file> [--device HIP]\n  zkey-export-vk --zkey <file> --vk <file>\n  wtns-check --r1cs <file> --wtns <file> [--device HIP]\n  r1cs-match --r1cs <file> --zkey <file> [--device HIP]\n  zkey-verify --r1cs <file> --zkey <file> --ptau <file> [--device HIP]\n  zkey-new --r1cs <file> --ptau <file> --zkey <file> [--device HIP]\n  zkey-setup --r1cs <file> --zkey <file> [--vk <file>] [--device HIP]   (a single-party key from the operating system's randomness: whoever runs it can forge proofs)\n  zkey-contribute --zkey <file> --out <file> [--name <text>] [--device HIP]   (the secret is the operating system's)\n  zkey-contributions --zkey <file>   (section 10's chain and the header's delta; that C and H follow delta2 is zkey-verify's)\n  ptau-prepare --ptau <file> --out <file> [--device HIP]   (sections 12 to 15 from 2 to 5: powersoftau prepare phase2)\n  ptau-new --power <P> --out <file>   (the starting file of a ceremony: tau = alpha = beta = 1)\n  ptau-contribute --ptau <file> --out <file> [--name <text>] [--device HIP]   (the secrets are the operating system's)\n  ptau-contributions --ptau <file>   (section 7's chain and the file's first elements; that the other powers follow is ptau-verify's)\n  ptau-verify --ptau <file> [--device HIP]   (the contributions, then every power against the others and sections 12 to 15 against 2 to 5)\n  ptau-pack --ptau <file> --out <file> [--device HIP]   (every point as x and one bit of y: half the bytes)\n  ptau-unpack --packed <file> --out <file> [--device HIP]   (the .ptau back, byte for byte; a root per point)\n  ptau-truncate --ptau <file> --power <p> --out <file> [--device HIP]   (the file of a lower power; section 12's last block fixed up)\n  wtns-pack --wtns <file> --out <file>   (a code byte per value and only its significant bytes; on the host)\n  wtns-unpack --packed <file> --out <file> [--device HIP]   (the .wtns back; without --device on the host)\n  prove-packed --witness <packed file> --zkey <file> --proof <file> --public <file> [--device HIP]\n  wtns-check --r1cs <file> --wtnz <packed file> [--device HIP]\n  zkey-pack --zkey <file> --out <file> [--device HIP]   (points as x and one bit of y, coefficients as a code byte and their significant bytes)\n  zkey-unpack --packed <file> --out <file> [--device HIP]   (the .zkey back, byte for byte)\n  prove-zkez --witness <file> --zkez <packed key> --proof <file> --public <file> [--device HIP]\n  exit\n";
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
    if (!(in >> cmd)) {
      std::cout << "COMMAND_EMPTY\nCOMMAND_COMPLETED" << std::endl;
      continue;
    }
    if (cmd == "exit" || cmd == "EXIT" || cmd == "Exit") {
      std::cout << "COMMAND_EXIT\nCOMMAND_COMPLETED" << std::endl;
      break;
    }
    if (cmd == "prove") {
      // defaults of src/main.rs:46-50, except the device: this build registers "HIP" ("CUDA" is an alias)
      std::string witness = "witness.wtns", zkey = "circuit_final.zkey", proof = "proof.json", pub = "public.json", device = "CUDA", a, v;
      bool ok = true;
      while (in >> a) {
        if (a == "--system") {
          if (in >> v && v != "groth16" && v != "Groth16" && v != "GROTH16") {
            std::cerr << "Unknown proof system: " << v << std::endl;
            ok = false;
          }
        } else if (a == "--witness") in >> witness;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--proof") in >> proof;
        else if (a == "--public") in >> pub;
        else if (a == "--device") in >> device;
        else print_help();
      }
      if (!ok) {
        print_help();
        continue;
      }
      int rc = groth16_prove(witness.c_str(), zkey.c_str(), proof.c_str(), pub.c_str(), device.c_str(), cm);
      if (rc != 0) {
        // the reference unwraps (aborts) here; report and keep the worker alive instead
        std::cerr << "prove failed (" << rc << "): " << groth16_last_error() << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "verify") {
      // defaults of src/main.rs:84-86
      std::string proof = "proof.json", pub = "public.json", vk = "verification_key.json", a, v;
      bool ok = true;
      while (in >> a) {
        if (a == "--system") {
          if (in >> v && v != "groth16" && v != "Groth16" && v != "GROTH16") {
            std::cerr << "Unknown proof system: " << v << std::endl;
            ok = false;
          }
        } else if (a == "--proof") in >> proof;
        else if (a == "--public") in >> pub;
        else if (a == "--vk") in >> vk;
        else print_help();
      }
      if (!ok) {
        print_help();
        continue;
      }
      int rc = groth16_verify(proof.c_str(), pub.c_str(), vk.c_str());
      // the reference panics on a rejected proof (assert, src/lib.rs:79); report and keep the worker alive instead
      if (rc == 0) std::cout << "VERIFY_OK" << std::endl;
      else {
        std::cerr << "verify failed (" << rc << "): " << groth16_verify_last_error() << std::endl;
        std::cout << "VERIFY_FAILED" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "verify-batch") {
      // every "<proof.json> <public.json>" line of the list against one key, on one GPU: one line per item, then the counts
      std::string list, vk = "verification_key.json", device = "HIP", a;
      bool combined = false;
      while (in >> a) {
        if (a == "--list") in >> list;
        else if (a == "--vk") in >> vk;
        else if (a == "--device") in >> device;
        else if (a == "--combined") combined = true;
        else print_help();
      }
      auto slurp = [](const std::string& path, std::string* out) {
        std::ifstream f(path, std::ios::binary);
        if (!f) return false;
        std::ostringstream ss;
        ss << f.rdbuf();
        *out = ss.str();
        return true;
      };
      std::string vk_text, list_text;
      if (list.empty() || !slurp(list, &list_text) || !slurp(vk, &vk_text)) {
        std::cerr << "verify-batch: cannot read " << (list.empty() ? std::string("--list (missing)") : list) << " or " << vk << std::endl;
        std::cout << "COMMAND_COMPLETED" << std::endl;
        continue;
      }
      std::vector<std::string> proofs, publics;
      std::vector<int> readable; // 1: both files read; 0: reported as an error without being judged
      std::istringstream ls(list_text);
      std::string ln;
      while (std::getline(ls, ln)) {
        std::istringstream lf(ln);
        std::string pp, qp, pt, qt;
        if (!(lf >> pp)) continue; // blank line
        const bool ok = (lf >> qp) && slurp(pp, &pt) && slurp(qp, &qt);
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
      if (rc != 0) {
        std::cerr << "verify-batch failed (" << rc << "): " << groth16_verify_last_error() << std::endl;
      } else {
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
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-check") {
      std::string zkey = "circuit_final.zkey", device = "HIP", a;
      while (in >> a) {
        if (a == "--zkey") in >> zkey;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16ZkeyReport rep;
      const int rc = groth16_zkey_check_file(zkey.c_str(), device.c_str(), nullptr, &rep);
      if (rc < 0) {
        std::cerr << "zkey-check failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
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
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-export-vk") {
      std::string zkey = "circuit_final.zkey", vk = "verification_key.json", a;
      while (in >> a) {
        if (a == "--zkey") in >> zkey;
        else if (a == "--vk") in >> vk;
        else print_help();
      }
      std::ifstream f(zkey, std::ios::binary);
      std::ostringstream ss;
      if (f) ss << f.rdbuf();
      const std::string image = ss.str();
      const int64_t need = f ? groth16_zkey_export_vk(image.data(), image.size(), nullptr, 0) : -1;
      if (need < 0) {
        std::cerr << "zkey-export-vk failed (" << need << "): " << (f ? groth16_last_error() : "cannot read the zkey") << std::endl;
      } else {
        std::string text((size_t)need, '\0');
        (void)groth16_zkey_export_vk(image.data(), image.size(), &text[0], text.size());
        text.resize((size_t)need - 1);
        std::ofstream o(vk, std::ios::binary);
        o << text;
        if (!o) std::cerr << "zkey-export-vk: cannot write " << vk << std::endl;
        else std::cout << "VK_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "wtns-check" || cmd == "r1cs-match") {
      std::string r1cs = "circuit.r1cs", wtns = "witness.wtns", wtnz, zkey = "circuit_final.zkey", device = "HIP", a;
      while (in >> a) {
        if (a == "--r1cs") in >> r1cs;
        else if (a == "--wtns") in >> wtns;
        else if (a == "--wtnz") in >> wtnz;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16R1cs* h = nullptr;
      int rc = groth16_r1cs_load_file(r1cs.c_str(), device.c_str(), &h);
      if (rc < 0) {
        std::cerr << cmd << " failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else if (cmd == "wtns-check") {
        Groth16WitnessReport rep;
        rc = wtnz.empty() ? groth16_witness_check_file(h, wtns.c_str(), &rep) : groth16_witness_check_packed_file(h, wtnz.c_str(), &rep);
        if (rc < 0) {
          std::cerr << "wtns-check failed (" << rc << "): " << groth16_last_error() << std::endl;
        } else {
          if (rep.kind == GROTH16_WTNS_NONCANONICAL) std::cout << rep.noncanonical << " values not below r, first: wire " << rep.index << std::endl;
          else if (rep.kind == GROTH16_WTNS_ONE) std::cout << "wire 0 is not 1" << std::endl;
          if (rep.failed) std::cout << rep.failed << " constraints violated" << (rep.kind == GROTH16_WTNS_CONSTRAINT ? ", first: constraint " + std::to_string(rep.index) : std::string()) << std::endl;
          std::cout << (rc == 1 ? "satisfied" : "not satisfied") << std::endl;
        }
      } else {
        std::ifstream f(zkey, std::ios::binary);
        std::ostringstream ss;
        if (f) ss << f.rdbuf();
        const std::string image = ss.str();
        Groth16R1csMatchReport rep;
        rc = f ? groth16_r1cs_match_zkey(h, image.data(), image.size(), nullptr, &rep) : -1;
        if (rc < 0) {
          std::cerr << "r1cs-match failed (" << rc << "): " << (f ? groth16_last_error() : "cannot read the zkey") << std::endl;
        } else {
          static const char* const sizes[3] = {"n_vars against nWires", "n_public", "domain_size"};
          if (rep.kind == GROTH16_MATCH_SIZES) std::cout << "sizes differ: " << sizes[rep.index < 3 ? rep.index : 0] << std::endl;
          if (rep.rows_a) std::cout << rep.rows_a << " rows of A differ" << (rep.kind == GROTH16_MATCH_ROW_A ? ", first: row " + std::to_string(rep.index) : std::string()) << std::endl;
          if (rep.rows_b) std::cout << rep.rows_b << " rows of B differ" << (rep.kind == GROTH16_MATCH_ROW_B ? ", first: row " + std::to_string(rep.index) : std::string()) << std::endl;
          std::cout << (rc == 1 ? "match" : "no match") << std::endl;
        }
      }
      groth16_r1cs_free(h);
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-verify") {
      // the two questions `snarkjs zkey verify` asks of a key, one line each: section 4 against the circuit (r1cs-match), then the
      // point sections against the circuit and the ceremony
      std::string r1cs = "circuit.r1cs", zkey = "circuit_final.zkey", ptau = "pot_final.ptau", device = "HIP", a;
      while (in >> a) {
        if (a == "--r1cs") in >> r1cs;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--ptau") in >> ptau;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16R1cs* h = nullptr;
      int rc = groth16_r1cs_load_file(r1cs.c_str(), device.c_str(), &h);
      if (rc < 0) {
        std::cerr << "zkey-verify failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::ifstream f(zkey, std::ios::binary);
        std::ostringstream ss;
        if (f) ss << f.rdbuf();
        const std::string image = ss.str();
        Groth16R1csMatchReport mrep;
        const int mrc = f ? groth16_r1cs_match_zkey(h, image.data(), image.size(), nullptr, &mrep) : -1;
        if (mrc < 0) {
          std::cerr << "zkey-verify: r1cs-match failed (" << mrc << "): " << (f ? groth16_last_error() : "cannot read the zkey") << std::endl;
        } else {
          static const char* const mkinds[4] = {"match", "no match: SIZES", "no match: ROW_A", "no match: ROW_B"};
          std::cout << "section 4 against the circuit: " << mkinds[mrep.kind >= 0 && mrep.kind <= 3 ? mrep.kind : 0] << std::endl;
        }
        Groth16ZkeyVerifyReport rep;
        rc = groth16_zkey_verify_ptau_file(h, zkey.c_str(), ptau.c_str(), nullptr, &rep);
        if (rc < 0) {
          std::cerr << "zkey-verify failed (" << rc << "): " << groth16_last_error() << std::endl;
        } else {
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
      }
      groth16_r1cs_free(h);
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-new") {
      std::string r1cs = "circuit.r1cs", zkey = "circuit_0000.zkey", ptau = "pot_final.ptau", device = "HIP", a;
      while (in >> a) {
        if (a == "--r1cs") in >> r1cs;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--ptau") in >> ptau;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16R1cs* h = nullptr;
      int rc = groth16_r1cs_load_file(r1cs.c_str(), device.c_str(), &h);
      Groth16ZkeyNewReport rep;
      if (rc == 0) rc = groth16_zkey_new_file(h, ptau.c_str(), zkey.c_str(), nullptr, &rep);
      if (rc < 0) {
        std::cerr << "zkey-new failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::cout << "wires " << rep.n_vars << " public " << rep.n_public << " domain " << rep.domain << " coefficients " << rep.n_coeffs << " bytes " << rep.zkey_bytes
                  << " longest column " << rep.longest_column << " heavy columns " << rep.heavy_columns << " in " << rep.heavy_items << " items; upload " << rep.upload_ms
                  << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms" << std::endl;
        std::cout << "ZKEY_WRITTEN" << std::endl;
      }
      groth16_r1cs_free(h);
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-setup") {
      // the toxic waste is the operating system's: none is taken from a command line
      std::string r1cs = "circuit.r1cs", zkey = "circuit_final.zkey", vk, device = "HIP", a;
      while (in >> a) {
        if (a == "--r1cs") in >> r1cs;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--vk") in >> vk;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16R1cs* h = nullptr;
      int rc = groth16_r1cs_load_file(r1cs.c_str(), device.c_str(), &h);
      Groth16SetupReport rep;
      if (rc == 0) rc = groth16_setup_file(h, nullptr, zkey.c_str(), nullptr, &rep);
      if (rc < 0) {
        std::cerr << "zkey-setup failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::cout << "wires " << rep.n_vars << " public " << rep.n_public << " domain " << rep.domain << " coefficients " << rep.n_coeffs << " bytes " << rep.zkey_bytes
                  << " longest column " << rep.longest_column << " heavy columns " << rep.heavy_columns << " in " << rep.heavy_items << " items; upload " << rep.upload_ms
                  << " ms device " << rep.device_ms << " ms (lagrange " << rep.lagrange_ms << " columns " << rep.columns_ms << " G1 " << rep.g1_ms << " G2 " << rep.g2_ms
                  << ") download " << rep.download_ms << " ms write " << rep.write_ms << " ms" << std::endl;
        std::cout << "single-party key: whoever ran this command can forge proofs for it; a key for third parties comes from the ceremony chain" << std::endl;
        bool vk_ok = true;
        if (!vk.empty()) {
          std::ifstream f(zkey, std::ios::binary);
          std::ostringstream ss;
          if (f) ss << f.rdbuf();
          const std::string image = ss.str();
          const int64_t need = f ? groth16_zkey_export_vk(image.data(), image.size(), nullptr, 0) : -1;
          vk_ok = need >= 0;
          if (vk_ok) {
            std::string text((size_t)need, '\0');
            (void)groth16_zkey_export_vk(image.data(), image.size(), &text[0], text.size());
            text.resize((size_t)need - 1);
            std::ofstream o(vk, std::ios::binary);
            o << text;
            vk_ok = (bool)o;
          }
          if (!vk_ok) std::cerr << "zkey-setup: cannot write " << vk << ": " << (need < 0 ? groth16_last_error() : "I/O") << std::endl;
        }
        std::cout << "ZKEY_WRITTEN" << std::endl;
        if (!vk.empty() && vk_ok) std::cout << "VK_WRITTEN" << std::endl;
      }
      groth16_r1cs_free(h);
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-contribute") {
      // the secret is the operating system's: none is taken from a command line
      std::string zkey = "circuit_0000.zkey", out = "circuit_0001.zkey", name, device = "HIP", a;
      while (in >> a) {
        if (a == "--zkey") in >> zkey;
        else if (a == "--out") in >> out;
        else if (a == "--name") in >> name;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16ZkeyContributeReport rep;
      const int rc = groth16_zkey_contribute_file(zkey.c_str(), out.c_str(), nullptr, name.c_str(), device.c_str(), nullptr, &rep);
      if (rc < 0) {
        std::cerr << "zkey-contribute failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::cout << "contribution " << rep.contribution << " points C " << rep.points_c << " H " << rep.points_h << " bytes " << rep.zkey_bytes << "; upload " << rep.upload_ms
                  << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms" << std::endl;
        std::cout << "ZKEY_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-contributions") {
      // the chain of section 10 and the header's delta pair, on the host; that C and H follow delta2 is zkey-verify's question
      std::string zkey = "circuit_final.zkey", a;
      while (in >> a) {
        if (a == "--zkey") in >> zkey;
        else print_help();
      }
      std::ifstream f(zkey, std::ios::binary);
      std::ostringstream ss;
      if (f) ss << f.rdbuf();
      const std::string image = ss.str();
      Groth16ContributionsReport rep;
      std::vector<Groth16ContributionInfo> infos(4096); // the records that are listed; the verdict is over all of them
      const int rc = f ? groth16_zkey_contributions(image.data(), image.size(), &rep, infos.data(), infos.size()) : -1;
      if (rc < 0) {
        std::cerr << "zkey-contributions failed (" << rc << "): " << (f ? groth16_last_error() : "cannot read the zkey") << std::endl;
      } else {
        static const char* const kinds[6] = {"", "SECTION", "POINT", "POK", "HEADER", "PAIR"};
        const uint32_t held = rep.kind == GROTH16_CONTRIB_SECTION ? (rep.index ? rep.index - 1 : 0) : rep.count;
        for (uint32_t i = 0; i < held && i < infos.size(); i++) {
          static const char hex[] = "0123456789abcdef";
          std::string d;
          for (int k = 0; k < 8; k++) d += {hex[infos[i].after1[k] >> 4], hex[infos[i].after1[k] & 15]};
          std::cout << "contribution " << i + 1 << " name \"" << infos[i].name << "\" delta1 " << d << "..." << std::endl;
        }
        if (rc == 1) std::cout << "CHAIN_OK" << std::endl;
        else std::cout << "CHAIN_BAD " << kinds[rep.kind >= 1 && rep.kind <= 5 ? rep.kind : 0] << " " << rep.index << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-prepare") {
      std::string ptau = "pot.ptau", out = "pot_final.ptau", device = "HIP", a;
      while (in >> a) {
        if (a == "--ptau") in >> ptau;
        else if (a == "--out") in >> out;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16PtauPrepareReport rep;
      const int rc = groth16_ptau_prepare_file(ptau.c_str(), out.c_str(), device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << "ptau-prepare failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::cout << "power " << rep.power << " points " << rep.points[0] << " " << rep.points[1] << " " << rep.points[2] << " " << rep.points[3] << " bytes " << rep.ptau_bytes
                  << "; upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms" << std::endl;
        std::cout << "PTAU_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-new") {
      std::string out = "pot_0000.ptau", a;
      long power = -1;
      while (in >> a) {
        if (a == "--power") in >> power;
        else if (a == "--out") in >> out;
        else print_help();
      }
      const int rc = power < 0 || power > 64 ? -3 : groth16_ptau_new_file((uint32_t)power, out.c_str());
      if (rc < 0) std::cerr << "ptau-new failed (" << rc << "): " << (power < 0 || power > 64 ? "--power <P> is required, 0 to 27" : groth16_last_error()) << std::endl;
      else std::cout << "PTAU_WRITTEN" << std::endl;
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-contribute") {
      // the secrets are the operating system's: none is taken from a command line
      std::string ptau = "pot_0000.ptau", out = "pot_0001.ptau", name, device = "HIP", a;
      while (in >> a) {
        if (a == "--ptau") in >> ptau;
        else if (a == "--out") in >> out;
        else if (a == "--name") in >> name;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16PtauContributeReport rep;
      const int rc = groth16_ptau_contribute_file(ptau.c_str(), out.c_str(), nullptr, name.c_str(), device.c_str(), nullptr, &rep);
      if (rc < 0) {
        std::cerr << "ptau-contribute failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        std::cout << "contribution " << rep.contribution << " power " << rep.power << " points " << rep.points[0] << " " << rep.points[1] << " " << rep.points[2] << " " << rep.points[3]
                  << " bytes " << rep.ptau_bytes << "; upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms
                  << " ms" << std::endl;
        std::cout << "PTAU_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-contributions") {
      // the chain of section 7 against the file's first elements, on the host; that the other powers follow is another question
      std::string ptau = "pot_final.ptau", a;
      while (in >> a) {
        if (a == "--ptau") in >> ptau;
        else print_help();
      }
      std::ifstream f(ptau, std::ios::binary);
      std::ostringstream ss;
      if (f) ss << f.rdbuf();
      const std::string image = ss.str();
      Groth16PtauContributionsReport rep;
      std::vector<Groth16PtauContributionInfo> infos(1024); // the records that are listed; the verdict is over all of them
      const int rc = f ? groth16_ptau_contributions(image.data(), image.size(), &rep, infos.data(), infos.size()) : -1;
      if (rc < 0) {
        std::cerr << "ptau-contributions failed (" << rc << "): " << (f ? groth16_last_error() : "cannot read the ptau") << std::endl;
      } else {
        static const char* const kinds[6] = {"", "SECTION", "POINT", "POK", "HEADER", "PAIR"};
        const uint32_t held = rep.kind == GROTH16_CONTRIB_SECTION ? (rep.index ? rep.index - 1 : 0) : rep.count;
        for (uint32_t i = 0; i < held && i < infos.size(); i++) {
          static const char hex[] = "0123456789abcdef";
          std::string d;
          for (int k = 0; k < 8; k++) d += {hex[infos[i].tau1[k] >> 4], hex[infos[i].tau1[k] & 15]};
          std::cout << "contribution " << i + 1 << " name \"" << infos[i].name << "\" tau1 " << d << "..." << std::endl;
        }
        if (rc == 1) std::cout << "CHAIN_OK" << std::endl;
        else std::cout << "CHAIN_BAD " << kinds[rep.kind >= 1 && rep.kind <= 5 ? rep.kind : 0] << " " << rep.index << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-verify") {
      // the audit first, as zkey-verify runs r1cs-match: who contributed, then whether the points are what they should be
      std::string ptau = "pot_final.ptau", device = "HIP", a;
      while (in >> a) {
        if (a == "--ptau") in >> ptau;
        else if (a == "--device") in >> device;
        else print_help();
      }
      static const char* const kinds[14] = {"", "GENERATORS", "TAU_PAIR", "BETA_PAIR", "TAU_G1", "TAU_G2", "ALPHA_TAU", "BETA_TAU", "LAGRANGE_12", "LAGRANGE_13", "LAGRANGE_14",
                                            "LAGRANGE_15", "POINT", "IDENTITY"};
      Groth16PtauVerifyReport rep;
      const int rc = groth16_ptau_verify_file(ptau.c_str(), nullptr, device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << "ptau-verify failed (" << rc << "): " << groth16_last_error() << std::endl;
      } else {
        // the chain of section 7: the audit reads an unprepared file; for a prepared one it is said, not skipped silently
        int chain = -1;
        if (!rep.prepared) {
          std::ifstream f(ptau, std::ios::binary);
          std::ostringstream ss;
          if (f) ss << f.rdbuf();
          const std::string image = ss.str();
          Groth16PtauContributionsReport crep = {};
          chain = f ? groth16_ptau_contributions(image.data(), image.size(), &crep, nullptr, 0) : -1;
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
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-pack" || cmd == "ptau-unpack") {
      const bool unpack = cmd == "ptau-unpack";
      std::string inp = unpack ? "pot_final.ptaz" : "pot_final.ptau", out = unpack ? "pot_final.ptau" : "pot_final.ptaz", device = "HIP", a;
      while (in >> a) {
        if (a == (unpack ? "--packed" : "--ptau")) in >> inp;
        else if (a == "--out") in >> out;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16PtauPackReport rep = {};
      const int rc = unpack ? groth16_ptau_unpack_file(inp.c_str(), out.c_str(), device.c_str(), &rep) : groth16_ptau_pack_file(inp.c_str(), out.c_str(), device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << cmd << " failed (" << rc << "): " << groth16_last_error() << std::endl;
        if (rep.fault_kind) std::cout << "PTAU_BAD POINT " << rep.fault_section << " " << rep.fault_index << std::endl;
      } else {
        std::cout << "power " << rep.power << (rep.prepared ? " prepared" : " unprepared") << " points " << rep.points[0] << " " << rep.points[1] << " bytes " << rep.in_bytes << " to "
                  << rep.out_bytes << "; upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms"
                  << std::endl;
        std::cout << "PTAU_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "ptau-truncate") {
      std::string inp = "pot_final.ptau", out = "pot_cut.ptau", device = "HIP", a;
      long power = -1;
      while (in >> a) {
        if (a == "--ptau") in >> inp;
        else if (a == "--power") in >> power;
        else if (a == "--out") in >> out;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16PtauTruncateReport rep = {};
      const bool bad_power = power < 0 || power > 64;
      const int rc = bad_power ? -3 : groth16_ptau_truncate_file(inp.c_str(), out.c_str(), (uint32_t)power, device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << "ptau-truncate failed (" << rc << "): " << (bad_power ? "--power <p> is required, 0 to the file's power" : groth16_last_error()) << std::endl;
        if (rep.fault_kind) std::cout << "PTAU_BAD POINT " << rep.fault_section << " " << rep.fault_index << " " << rep.fault_count << std::endl;
      } else {
        std::cout << "power " << rep.power_in << " to " << rep.power_out << (rep.prepared ? " prepared" : " unprepared") << " fixed " << rep.points_fixed << " bytes " << rep.in_bytes << " to "
                  << rep.out_bytes << "; upload " << rep.upload_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms"
                  << std::endl;
        std::cout << "PTAU_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "wtns-pack" || cmd == "wtns-unpack") {
      // pack is the host's; unpack is the host's too unless --device names a GPU
      const bool unpack = cmd == "wtns-unpack";
      std::string inp = unpack ? "witness.wtnz" : "witness.wtns", out = unpack ? "witness.wtns" : "witness.wtnz", device, a;
      while (in >> a) {
        if (a == (unpack ? "--packed" : "--wtns")) in >> inp;
        else if (a == "--out") in >> out;
        else if (a == "--device" && unpack) in >> device;
        else print_help();
      }
      Groth16WtnsPackReport rep = {};
      const int rc = !unpack          ? groth16_wtns_pack_file(inp.c_str(), out.c_str(), &rep)
                     : device.empty() ? groth16_wtns_unpack_host_file(inp.c_str(), out.c_str(), &rep)
                                      : groth16_wtns_unpack_file(inp.c_str(), out.c_str(), device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << cmd << " failed (" << rc << "): " << groth16_last_error() << std::endl;
        if (rep.fault_kind) std::cout << "WTNS_BAD VALUE " << rep.fault_index << " " << rep.fault_count << std::endl;
      } else {
        std::cout << "values " << rep.n_witness << " bytes " << rep.in_bytes << " to " << rep.out_bytes;
        if (!device.empty()) std::cout << "; upload " << rep.upload_ms << " ms kernel " << rep.kernel_ms << " ms device " << rep.device_ms << " ms download " << rep.download_ms << " ms";
        std::cout << " write " << rep.write_ms << " ms" << std::endl;
        std::cout << "WTNS_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "prove-packed") {
      std::string witness = "witness.wtnz", zkey = "circuit_final.zkey", proof = "proof.json", pub = "public.json", device = "HIP", a;
      while (in >> a) {
        if (a == "--witness") in >> witness;
        else if (a == "--zkey") in >> zkey;
        else if (a == "--proof") in >> proof;
        else if (a == "--public") in >> pub;
        else if (a == "--device") in >> device;
        else print_help();
      }
      const int rc = groth16_prove_packed_files(witness.c_str(), zkey.c_str(), proof.c_str(), pub.c_str(), device.c_str(), cm);
      if (rc != 0) std::cerr << "prove-packed failed (" << rc << "): " << groth16_last_error() << std::endl;
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "zkey-pack" || cmd == "zkey-unpack") {
      const bool unpack = cmd == "zkey-unpack";
      std::string inp = unpack ? "circuit_final.zkez" : "circuit_final.zkey", out = unpack ? "circuit_final.zkey" : "circuit_final.zkez", device = "HIP", a;
      while (in >> a) {
        if (a == (unpack ? "--packed" : "--zkey")) in >> inp;
        else if (a == "--out") in >> out;
        else if (a == "--device") in >> device;
        else print_help();
      }
      Groth16ZkeyPackReport rep = {};
      const int rc = unpack ? groth16_zkey_unpack_file(inp.c_str(), out.c_str(), device.c_str(), &rep) : groth16_zkey_pack_file(inp.c_str(), out.c_str(), device.c_str(), &rep);
      if (rc < 0) {
        std::cerr << cmd << " failed (" << rc << "): " << groth16_last_error() << std::endl;
        if (rep.fault_kind && rep.fault_section == 4) std::cout << "ZKEY_BAD COEFFICIENT " << rep.fault_index << " " << rep.fault_count << std::endl;
        else if (rep.fault_kind) std::cout << "ZKEY_BAD POINT " << rep.fault_section << " " << rep.fault_index << " " << rep.fault_count << std::endl;
      } else {
        std::cout << "wires " << rep.n_vars << " domain " << rep.domain << " coefficients " << rep.n_coef << " points " << rep.points[0] << " " << rep.points[1] << " bytes " << rep.in_bytes
                  << " to " << rep.out_bytes << " (packed points " << rep.point_bytes << " section 4 " << rep.coef_bytes << "); upload " << rep.upload_ms << " ms device " << rep.device_ms
                  << " ms download " << rep.download_ms << " ms write " << rep.write_ms << " ms" << std::endl;
        std::cout << "ZKEY_WRITTEN" << std::endl;
      }
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else if (cmd == "prove-zkez") {
      std::string witness = "witness.wtns", zkez = "circuit_final.zkez", proof = "proof.json", pub = "public.json", device = "HIP", a;
      while (in >> a) {
        if (a == "--witness") in >> witness;
        else if (a == "--zkez") in >> zkez;
        else if (a == "--proof") in >> proof;
        else if (a == "--public") in >> pub;
        else if (a == "--device") in >> device;
        else print_help();
      }
      const int rc = groth16_prove_zkez_files(witness.c_str(), zkez.c_str(), proof.c_str(), pub.c_str(), device.c_str(), cm);
      if (rc != 0) std::cerr << "prove-zkez failed (" << rc << "): " << groth16_last_error() << std::endl;
      std::cout << "COMMAND_COMPLETED" << std::endl;
    } else {
      print_help();
    }
  }
  std::cout << "Exiting CLI worker..." << std::endl;
  groth16_cache_manager_free(cm);
  return 0;
}
