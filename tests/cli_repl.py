"""Start the REPL worker (lib/prove) on one session text → (stdout lines without the "> " prompts, stderr, return code)."""
import os
import subprocess

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "icicle-snark_amd", "lib", "prove")


def run(session: str, cwd=None, timeout=60):
    out = subprocess.run([EXE], input=session, capture_output=True, text=True, timeout=timeout, cwd=cwd)
    return [ln[2:] if ln.startswith("> ") else ln for ln in out.stdout.splitlines()], out.stderr, out.returncode
