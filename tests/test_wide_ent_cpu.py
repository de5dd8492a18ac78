"""The entity image and the header word of move, damage, destroy and the ability call (monsoon_amd/csrc/rules.h ei_load / ei_*,
hdr_word / hw_*; state.h MSB_WIDE_ENT), on the host: tests/wide_ent_check.cpp is compiled against the host build of the product
core of each of the three record builds with the address and UB sanitizers -- the per-field text (-DMSB_WIDE_ENT=0, the
namespace renamed) and the text at its defaults -- and the two objects are linked into a stand-alone program and run (never
loaded into Python).  On the standard record a second program holds the per-field text against the text with the header word
as well (-DMSB_WIDE_ENT_HDR=1, which the product does not build).  Every generated record goes through both texts and must
come out byte for byte the same, with the same return value and fault code; the program's header comment says over which inputs.
What it counts is pinned here: no case went uncompared and every outcome the inputs are built for occurred.
The same forms inside whole games, on the device: tests/test_wide_ent_gpu.py."""
import os
import shutil
import subprocess

import pytest

import kernel_variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_DEPTH = 18
TR_ON_DEATH, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING, TR_AFTER_SURVIVING, TR_BEFORE_MOVING = 1, 2, 3, 4, 5

CASES = [(False, []), (False, ["-DMSB_WIDE_ENT_HDR=1"]), (True, []), (2, [])]


@pytest.mark.parametrize("ext,words_flags", CASES, ids=["standard", "standard-header-word", "extended", "large"])
def test_whole_word_forms_equal_the_field_reads_under_sanitizers(tmp_path, ext, words_flags):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    common = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi", "-DMSB_COUNT_FRAMES"] + \
        kernel_variants.BUILD_FLAGS[ext] + ["-I", os.path.join(REPO, "monsoon_amd", "csrc")]
    src = os.path.join(REPO, "tests", "wide_ent_check.cpp")
    fields, words, exe = str(tmp_path / "fields.o"), str(tmp_path / "words.o"), str(tmp_path / "wide_ent_check")
    subprocess.run(common + ["-DWE_SIDE=0", "-Dmsb=msb_bytes", "-DMSB_WIDE_ENT=0", "-c", src, "-o", fields], check=True)
    subprocess.run(common + ["-DWE_SIDE=1"] + words_flags + ["-c", src, "-o", words], check=True)
    subprocess.run([cxx, "-fsanitize=address,undefined", fields, words, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words_out = r.stdout.split()
    assert words_out[0] == "ok", r.stdout
    got = {words_out[i]: int(words_out[i + 1]) for i in range(1, len(words_out), 2)}
    print(r.stdout)

    def outcomes(name):   # every compared case has exactly one outcome
        return sum(v for k, v in got.items() if k == name + "_clean" or k.startswith(name + "_fault"))

    # move: 16 tiles x 2 owners x 2 sides to play x movement 0..3 x ff x 10 things ahead; turn: 4 tiles x 2 sides x 3 bases
    assert got["move"] == 16 * 2 * 2 * 4 * 2 * 10 == outcomes("move"), got
    assert got["turn"] == 4 * 2 * 3 == outcomes("turn"), got
    # status: 5 statuses x counts 0..2 x 2 phases x 2 columns x 4 things ahead x 2 movers x 2 sides to play
    assert got["status"] == 5 * 3 * 2 * 2 * 4 * 2 * 2 == outcomes("status"), got
    # trigger: 5 triggers x 4 strengths x 2 sides to play x (on the mover: played, moved, moved and disabled; on the unit ahead:
    # played or moved x disabled or not)
    assert got["trigger"] == 5 * 4 * 2 * (3 + 4) == outcomes("trigger"), got
    # depth: 3 movers x 3 depths x 2 sides x 3 things ahead; records with a fault: 5 codes x 3 actions x 2 sides, none of them clean
    assert got["depth"] == 3 * 3 * 2 * 3 == outcomes("depth") and got["depth_fault%d" % FAULT_DEPTH] == got["depth_guard"] > 0, got
    assert got["depth_quiet"] > 0, got   # quiet moves one below the guard
    assert got["faulted"] == 5 * 3 * 2 == outcomes("faulted") and got["faulted_clean"] == 0, got
    # what the described records are built for
    for name in ("moved0", "moved1", "moved2", "moved3", "blocked", "fight", "target_dead", "mover_dead", "both_dead", "struct_hit", "sidestep",
                 "base_survives", "base_falls", "base_zero", "thaw", "poison_dmg", "vital_gain", "confused_step", "play_phase_move"):
        assert got[name] > 0, (name, got)
    for t in (TR_BEFORE_MOVING, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING, TR_ON_DEATH, TR_AFTER_SURVIVING):
        assert got["mover_ran%d" % t] > 0, (t, got)
    for t in (TR_BEFORE_MOVING, TR_BEFORE_ATTACKING, TR_AFTER_ATTACKING):   # the move asks ST_DISABLED before it calls these
        assert got["mover_ran%d_disabled" % t] == 0, (t, got)
    for t in (TR_ON_DEATH, TR_AFTER_SURVIVING):
        assert got["target_ran%d" % t] > 0, (t, got)
    # whole games: at least 50 games and 5 000 moves, and each thing the handlers do in them
    assert got["step"] == outcomes("step") and got["games"] >= 50 and got["g_moves"] >= 5000, got
    for name in ("g_fights", "g_base_hits", "g_destroy_plain", "g_destroy_on_death", "g_after_surviving"):
        assert got[name] > 0, (name, got)
