"""The short ability effects on whole words (monsoon_amd/csrc/rules.h: the status methods and heal-then-vitalize on the entity
image, gain_speed through set_path_known, random.choice asked of the hit mask; state.h MSB_WIDE_AB_ST / MSB_WIDE_AB_SPEED /
MSB_WIDE_AB_PICK), on the host: tests/wide_ab_check.cpp is compiled against the host build of the product core with the address
and UB sanitizers -- the text with the three switches at 0 (the namespace renamed) and the new text -- and the two objects are
linked into a stand-alone program and run (never loaded into Python).  On the standard record the new text is built twice: with
all three parts (two of them are switches the product does not build, profiles/wide_ab_ab.txt) and at the product's defaults.
On the extended and large records the switches are off on both sides and the program pins that they change nothing.  Every
generated record goes through both texts and must come out byte for byte the same, with the same return value and fault code;
the program's header comment says over which inputs.  What it counts is pinned here: no case went uncompared and every outcome
the inputs are built for occurred.  The same forms inside whole games, on the device: tests/test_wide_ab_gpu.py."""
import os
import shutil
import subprocess

import pytest

import kernel_variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAULT_PY_EXCEPTION, FAULT_STATUS_SAT, FAULT_CAP_PATH = 1, 21, 25
TOUCHED = "u007 u021 u061 u053 u051 u050 ua07 ud01 u055 s007 s012 ue03 ue01".split()

CASES = [(False, ["-DMSB_WIDE_AB_ST=1", "-DMSB_WIDE_AB_SPEED=1"], 7), (False, [], 4), (True, [], 0), (2, [], 0)]


@pytest.mark.parametrize("ext,side1_flags,parts", CASES, ids=["standard-all-parts", "standard-product", "extended", "large"])
def test_whole_word_effects_equal_the_field_text_under_sanitizers(tmp_path, ext, side1_flags, parts):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    common = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi"] + \
        kernel_variants.BUILD_FLAGS[ext] + ["-I", os.path.join(REPO, "monsoon_amd", "csrc")]
    src = os.path.join(REPO, "tests", "wide_ab_check.cpp")
    fields, words, exe = str(tmp_path / "fields.o"), str(tmp_path / "words.o"), str(tmp_path / "wide_ab_check")
    off = ["-DMSB_WIDE_AB_ST=0", "-DMSB_WIDE_AB_SPEED=0", "-DMSB_WIDE_AB_PICK=0"]
    builds = [subprocess.Popen(common + ["-DWA_SIDE=0", "-Dmsb=msb_fields"] + off + ["-c", src, "-o", fields]),
              subprocess.Popen(common + ["-DWA_SIDE=1"] + side1_flags + ["-c", src, "-o", words])]
    assert [b.wait() for b in builds] == [0, 0]
    subprocess.run([cxx, "-fsanitize=address,undefined", fields, words, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.split()
    assert out[0] == "ok", r.stdout
    got = {out[i]: int(out[i + 1]) for i in range(1, len(out), 2)}
    print(r.stdout)

    def outcomes(name):   # every compared case has exactly one outcome
        return sum(v for k, v in got.items() if k == name + "_clean" or k.startswith(name + "_fault"))

    assert got["parts"] == parts, got   # b0 statuses, b1 gain_speed, b2 the pick: which text side 1 is
    # effect: 9 effects x 6 targets x 4 counts x 3 counts of the opposite status x 3 strengths x a fault before the call or not x 2 sides
    assert got["effect"] == 9 * 6 * 4 * 3 * 3 * 2 * 2 == outcomes("effect"), got
    assert got["effect_fault%d" % FAULT_STATUS_SAT] == got["sat"] > 0 and got["effect_fault%d" % FAULT_PY_EXCEPTION] > 0, got
    assert got["fault_kept"] == got["effect"] // 2, got   # a fault set before the call is the fault after it
    for name in ("removed_at_zero", "not_a_unit", "vit_took_poison", "poison_took_vit", "no_ability", "healed_structure", "deconfused"):
        assert got[name] > 0, (name, got)
    # speed: 20 tiles x 2 owners x 2 sides x movement 0..3 x amount 1..3 x confused 0..2 x resolving or not x 3 boards
    assert got["speed"] == 20 * 2 * 2 * 4 * 3 * 3 * 2 * 3 == outcomes("speed"), got
    assert got["speed_fault%d" % FAULT_CAP_PATH] == got["speed_cap"] > 0, got   # movement + amount beyond four steps, resolving
    for name in ("speed_path1", "speed_path2", "speed_path3", "speed_path4", "speed_confused_draw", "speed_resolving_long"):
        assert got[name] > 0, (name, got)
    # choice: only the text with the pick holds both forms
    if parts & 4:
        assert got["choice"] > 20000 and got["choice_base"] > 0 and got["choice_empty"] > 0, got
    else:
        assert got["choice"] == 0, got
    assert got["pick"] > 100000 and got["pick_empty"] > 0 and got["pick_base"] > 0 and got["pick_drawn"] > 0, got
    # whole games on N12M and on the deck of the touched cards: no step faults, every touched ability ran
    assert got["step"] == outcomes("step") == got["step_clean"] and got["games"] >= 80 and got["step"] >= 5000, got
    for card in TOUCHED:
        assert got["ran_" + card] > 0, (card, got)
