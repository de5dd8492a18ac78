"""The mask arithmetic of the wave-cooperative legal set (monsoon_amd/csrc/coop_legal.h) and the target predicate factored
out of get_targets (rules.h target_matches / target_bases / get_targets_hit), on the host: tests/coop_legal_check.cpp is
compiled against the host build of the product core with the address and UB sanitizers into a stand-alone program and run
(never loaded into Python).  It writes coop_legal()'s lanes as loops and compares the result with legal_mask() /
get_targets() of the serial text: all 2^20 empty masks x 8 front lines for the PLACE offsets and a board for each of some
33 000 of them x 6 front lines, every single-tile and 4 000 multi-tile target masks x hand slot 0..4 for the USE bits (across
both word boundaries and past action 155), 400 boards x 64 synthetic target descriptors x both points of view, and every
state of 300 random-policy games on decks holding every targeted spell of the card table.  The ballots and lane reads of
the device form cannot run here: tests/test_coop_legal_gpu.py."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mask_arithmetic_and_target_predicate_equal_the_serial_text_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "coop_legal_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi",
                    "-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "coop_legal_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok", r.stdout
    place, use, desc, states, aimed = (int(words[i]) for i in (1, 3, 5, 7, 9))
    assert place >= 8 * (1 << 20) + 6 * 30000 and use == 4022 * 10 and desc == 400 * 64 * 2 * 5
    # some hundred games, and targeted spells in reach of the mover in a good share of their states
    assert states > 10000 and aimed > 2000, r.stdout
