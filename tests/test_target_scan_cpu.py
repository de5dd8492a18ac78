"""The target scans of a step that read only the tiles their caller keeps (monsoon_amd/csrc/rules.h shape_mask,
get_targets, shape_targets, shape_any, targets_any, target_has), on the host: tests/target_scan_check.cpp is compiled
against the host build of the product core of each of the three record builds with the address and UB sanitizers into a stand-alone program and run (never loaded
into Python).  On random boards it holds every restricted form against the -DMSB_TARGET_SCAN=0 text compiled into the same
program; its header comment says over which inputs.  What it counts is pinned here: no shape and no form went uncompared.
The same forms inside whole games, on the device: tests/test_target_scan_gpu.py."""
import os
import shutil
import subprocess

import pytest

import kernel_variants

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_restricted_scans_equal_the_full_board_forms_under_sanitizers(tmp_path, ext):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "target_scan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi"] +
                   kernel_variants.BUILD_FLAGS[ext] +
                   ["-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "target_scan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok", r.stdout
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    print(r.stdout)
    boards, desc = got["boards"], got["descriptors"]
    assert boards >= 100 and got["table_descriptors"] > 0 and desc > 1000
    for shape in range(7):
        # 20 centres x 2 points of view x 20 tiles on four boards (two per side to play); the lists over a window of 32
        # descriptors per board x 20 centres x 2 points of view x 3 exclusions
        assert got[f"mask{shape}"] == 4 * 20 * 2 * 20, got
        assert got[f"shape{shape}"] == boards * 32 * 20 * 2 * 3 and got[f"shape_any{shape}"] == boards * 32 * 20 * 2, got
    assert got["targets"] == boards * desc * 2 * 4 and got["any"] == boards * desc * 2, got
    assert got["has"] == boards * desc * 2 * 42 and got["spell"] == boards * desc * 2 * 23, got
    # scans that hit nothing and scans that hit more than one tile both occur
    assert got["scan_none"] > 1000 and got["scan_many"] > 1000, got
