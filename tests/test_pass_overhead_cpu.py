"""pass_actions (monsoon_amd/csrc/pass_glue.h), the helper that hands a pass's legal actions to the candidate lanes of
the hot kernel, on the host: tests/pass_actions_check.cpp is compiled with the address and UB sanitizers into a
stand-alone program and run (never loaded into Python).  It compares the helper with a plain nth-set-bit walk for all
masks of at most three bits in the 156-bit window, 10 000 seeded random masks, {1}, all 156 bits and bit 155 alone, at
every U in {4, 8, 16, 32, 64}.  The DPP reduction of the same header cannot run here: tests/test_pass_overhead_gpu.py."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MASKS = 1 + 156 + 156 * 155 // 2 + 156 * 155 * 154 // 6 + 10000 + 3


def test_pass_actions_equals_plain_nth_set_bit_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "pass_actions_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "pass_actions_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == N_MASKS and int(words[3]) > 5 * 10000, r.stdout
