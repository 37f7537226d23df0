"""The REPL worker's own text, on commands that open no GPU: one session through lib/prove, every stdout line and the stderr lines
compared with what the worker wrote for the same input before its commands became a table (csrc/prover/cli_main.cc).  The expected
lines below were recorded from that earlier binary, not from the table; only the measured times are masked."""
import re

import cli_repl
import wtns_pack_model as M

HELP = """Usage:
  prove [--system groth16] --witness <file> --zkey <file> --proof <file> --public <file> --device <HIP>
  verify [--system groth16] --proof <file> --public <file> --vk <file>
  verify-batch --list <file> --vk <file> [--device HIP] [--combined]
  zkey-check --zkey <file> [--device HIP]
  zkey-export-vk --zkey <file> --vk <file>
  wtns-check --r1cs <file> --wtns <file> [--device HIP]
  r1cs-match --r1cs <file> --zkey <file> [--device HIP]
  zkey-verify --r1cs <file> --zkey <file> --ptau <file> [--device HIP]
  zkey-new --r1cs <file> --ptau <file> --zkey <file> [--device HIP]
  zkey-setup --r1cs <file> --zkey <file> [--vk <file>] [--device HIP]   (a single-party key from the operating system's randomness: whoever runs it can forge proofs)
  zkey-contribute --zkey <file> --out <file> [--name <text>] [--device HIP]   (the secret is the operating system's)
  zkey-contributions --zkey <file>   (section 10's chain and the header's delta; that C and H follow delta2 is zkey-verify's)
  ptau-prepare --ptau <file> --out <file> [--device HIP]   (sections 12 to 15 from 2 to 5: powersoftau prepare phase2)
  ptau-new --power <P> --out <file>   (the starting file of a ceremony: tau = alpha = beta = 1)
  ptau-contribute --ptau <file> --out <file> [--name <text>] [--device HIP]   (the secrets are the operating system's)
  ptau-contributions --ptau <file>   (section 7's chain and the file's first elements; that the other powers follow is ptau-verify's)
  ptau-verify --ptau <file> [--device HIP]   (the contributions, then every power against the others and sections 12 to 15 against 2 to 5)
  ptau-pack --ptau <file> --out <file> [--device HIP]   (every point as x and one bit of y: half the bytes)
  ptau-unpack --packed <file> --out <file> [--device HIP]   (the .ptau back, byte for byte; a root per point)
  ptau-truncate --ptau <file> --power <p> --out <file> [--device HIP]   (the file of a lower power; section 12's last block fixed up)
  wtns-pack --wtns <file> --out <file>   (a code byte per value and only its significant bytes; on the host)
  wtns-unpack --packed <file> --out <file> [--device HIP]   (the .wtns back; without --device on the host)
  prove-packed --witness <packed file> --zkey <file> --proof <file> --public <file> [--device HIP]
  wtns-check --r1cs <file> --wtnz <packed file> [--device HIP]
  zkey-pack --zkey <file> --out <file> [--device HIP]   (points as x and one bit of y, coefficients as a code byte and their significant bytes)
  zkey-unpack --packed <file> --out <file> [--device HIP]   (the .zkey back, byte for byte)
  prove-zkez --witness <file> --zkez <packed key> --proof <file> --public <file> [--device HIP]
  exit""".split("\n")

DONE = "COMMAND_COMPLETED"


def test_host_session_transcript(tmp_path):
    d = str(tmp_path)
    values = [1] + [(i * i * 7919 + 3) % M.R_MOD if i % 5 else M.R_MOD - i for i in range(1, 300)]
    wtns = M.write_wtns(values)
    (tmp_path / "w.wtns").write_bytes(wtns)
    packed = "values 300 bytes 9676 to 1412 write # ms"
    session = [
        ("", ["COMMAND_EMPTY", DONE]),
        ("frobnicate --x 1", HELP),                                             # an unknown command: no completion line
        (f"ptau-new --out {d}/p.ptau", [DONE]),
        (f"ptau-new --power 2 --out {d}/p.ptau", ["PTAU_WRITTEN", DONE]),
        (f"ptau-contributions --ptau {d}/p.ptau", ["CHAIN_OK", DONE]),
        (f"ptau-contributions --ptau {d}/missing.ptau", [DONE]),
        (f"zkey-contributions --zkey {d}/missing.zkey", [DONE]),
        (f"zkey-export-vk --zkey {d}/missing.zkey --vk {d}/vk.json", [DONE]),
        (f"wtns-pack --wtns {d}/w.wtns --out {d}/w.wtnz", [packed, "WTNS_WRITTEN", DONE]),
        (f"wtns-unpack --packed {d}/w.wtnz --out {d}/w2.wtns", ["values 300 bytes 1412 to 9676 write # ms", "WTNS_WRITTEN", DONE]),
        (f"wtns-pack --device HIP --wtns {d}/w.wtns --out {d}/w3.wtnz", HELP + HELP + [packed, "WTNS_WRITTEN", DONE]),   # two unknown tokens
        (f"verify --system plonk --proof {d}/nope.json", HELP),                # the one command that does not run: no completion line
        ("verify --bogus", HELP + ["VERIFY_FAILED", DONE]),                     # the defaults name files the directory does not hold
        ("Exit", ["COMMAND_EXIT", DONE, "Exiting CLI worker..."]),
        ("ptau-new --power 1", []),                                             # after exit: not read
    ]
    lines, err, rc = cli_repl.run("".join(cmd + "\n" for cmd, _ in session), cwd=d)
    assert rc == 0
    lines = [re.sub(r"[0-9.e+-]+ ms", "# ms", ln) for ln in lines]
    assert lines == [ln for _, want in session for ln in want]
    assert err.splitlines() == ["ptau-new failed (-3): --power <P> is required, 0 to 27",
                                "ptau-contributions failed (-1): cannot read the ptau",
                                "zkey-contributions failed (-1): cannot read the zkey",
                                "zkey-export-vk failed (-1): cannot read the zkey",
                                "Unknown proof system: plonk",
                                "verify failed (-1): cannot read input file"]
    assert len(wtns) == 9676 and M.packed_size(values) == 1412
    assert (tmp_path / "w.wtnz").read_bytes() == (tmp_path / "w3.wtnz").read_bytes() == M.pack(values)
    assert (tmp_path / "w2.wtns").read_bytes() == wtns
    assert not (tmp_path / "vk.json").exists() and not (tmp_path / "pot_0000.ptau").exists()
