"""The hand, deck and path bookkeeping of a step on whole words (monsoon_amd/csrc/rules.h discard_wide, draw_take_wide, the hand
entry read once per play, set_path_impl; state.h MSB_WIDE_LISTS, MSB_WIDE_PATH), on the host: tests/wide_lists_check.cpp is
compiled twice against the host build of the product core of each of the three record builds with the address and UB
sanitizers -- the text of the loops (both switches 0, the namespace renamed) and the text of the whole words -- and the two
objects are linked into a stand-alone program and run (never loaded into Python).  Every generated record goes through both
texts and must come out byte for byte the same, with the same return value and fault code; the program's header comment says
over which inputs.  What it counts is pinned here: no case went uncompared and every outcome the inputs are built for occurred.
The same forms inside whole games, on the device: tests/test_wide_lists_gpu.py."""
import os
import shutil
import subprocess

import pytest

import kernel_variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_PY_EXCEPTION, FAULT_UNSUPPORTED, FAULT_CAP_DECK, FAULT_CAP_HAND, FAULT_CAP_PATH = 1, 20, 23, 24, 25


@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_whole_word_forms_equal_the_loops_under_sanitizers(tmp_path, ext):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    common = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi"] + \
        kernel_variants.BUILD_FLAGS[ext] + ["-I", os.path.join(REPO, "monsoon_amd", "csrc")]
    src = os.path.join(REPO, "tests", "wide_lists_check.cpp")
    loops, words, exe = str(tmp_path / "loops.o"), str(tmp_path / "words.o"), str(tmp_path / "wide_lists_check")
    subprocess.run(common + ["-DWL_SIDE=0", "-Dmsb=msb_loops", "-DMSB_WIDE_LISTS=0", "-DMSB_WIDE_PATH=0", "-c", src, "-o", loops], check=True)
    subprocess.run(common + ["-DWL_SIDE=1", "-c", src, "-o", words], check=True)
    subprocess.run([cxx, "-fsanitize=address,undefined", loops, words, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words_out = r.stdout.split()
    assert words_out[0] == "ok", r.stdout
    got = {words_out[i]: int(words_out[i + 1]) for i in range(1, len(words_out), 2)}
    print(r.stdout)

    def outcomes(name):   # every compared case has exactly one outcome
        return sum(v for k, v in got.items() if k == name + "_clean" or k.startswith(name + "_fault"))

    # set_path: 6 boards x 20 tiles x 2 owners x 2 sides to play x mov 0..5 x ff x confused 0..2 x on_play, and the two
    # alternating boards
    assert got["set_path"] == 6 * 20 * 2 * 2 * 6 * 2 * 3 * 2 + 2 == outcomes("set_path"), got
    assert got["set_path_fault%d" % FAULT_CAP_PATH] > 0 and got["sidestep_seen"] == 2, got
    # whole games: plays and REPLACEs in numbers
    assert got["step"] == outcomes("step") and got["games"] >= 50 and got["plays"] > 1000 and got["replaces"] > 500, got
    if ext:
        assert got["discard"] == 0 and got["draw"] == 0, got   # parts 1-3 are the standard record's
        return
    # discard: hand sizes 0..5 (size 0 once, index 0) x indices x 13 deck sizes x single use x 2 players; 10 x 9 x 3 earlier
    # equal cards; 12 bytes x 3 ages x 12 deck sizes; 20 000 random records
    assert got["discard"] == (1 + 15) * 13 * 2 * 2 + 10 * 9 * 3 + 12 * 3 * 12 + 20000 == outcomes("discard"), got
    for i in range(5):
        assert got["hand_remove%d" % i] == (5 - i) * 13 * 2 * 2, got
    for n in range(13):
        assert got["push_at%d" % n] > 0, got   # a push at 11 fills the deck, a push at 12 is FAULT_CAP_DECK
    assert got["discard_fault%d" % FAULT_CAP_DECK] > 0 and got["discard_fault%d" % FAULT_PY_EXCEPTION] > 0 and \
        got["discard_fault%d" % FAULT_UNSUPPORTED] > 0, got
    assert got["dup_hand"] == 10 * 2 and got["dup_deck"] == 66 * 2, got
    # draw: sum over deck sizes of (dn + 1) hints x 6 hand sizes x 2 players; 6 000 searches; 66 x 9 x 3 earlier equal cards
    assert got["draw"] == sum(dn + 1 for dn in range(13)) * 6 * 2 + 6000 + 66 * 9 * 3 == outcomes("draw"), got
    for i in range(12):
        assert got["deck_remove%d" % i] >= 10, got   # removal at every index of a full deck (hand sizes 0..4, both players)
    assert got["draw_fault%d" % FAULT_CAP_HAND] > 0 and got["draw_fault%d" % FAULT_PY_EXCEPTION] > 0 and \
        got["draw_fault%d" % FAULT_UNSUPPORTED] > 0, got
