"""The candidate records' LDS map of the wavefront-per-game kernels (monsoon_amd/csrc/lds_layout.h) on the host:
tests/lds_layout_check.cpp is compiled against the map header and the record layout of each of the three builds with the
address and UB sanitizers into a stand-alone program and run (never loaded into Python).  It checks the bounds of the map,
the round trip of a record from the whole-wave granule moves to the per-lane, column-0 and sub-lane accessor forms, and the
LDS banks the accesses fall on; its header comment says how.  What it reports per build is pinned here: which map the build
selects and why, and that the candidate area of the standard record did not grow.  The accessors themselves run on the device
only: tests/test_lds_layout_gpu.py."""
import os
import shutil
import subprocess

import pytest

import kernel_variants
import lds_layout_line as LL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# build -> what the check program must report.  column_lane_degree: the worst number of distinct addresses on one bank when
# lanes 0..7 touch one offset of a column each (1 = none collide), whether or not the build uses columns; move_*_degree: the same
# for the whole-wave moves of a record on the map the build selects.
EXPECT = {
    False: dict(state_bytes=752, columns=1, stride_mod128=112, column_lane_degree=1, move_store_degree=1, move_read_degree=1, area8=6016),
    # 2 400 = 96 (mod 128): columns k and k + 4 would share banks on 4-byte accesses, so the extended record keeps the
    # interleave, whose moves are 8-way on stores and 16-way on reads at the worst U (listed per U in the check program)
    True: dict(state_bytes=2400, columns=0, stride_mod128=96, column_lane_degree=2, move_store_degree=8, move_read_degree=16, area8=19200),
    # 8 336 = +16 (mod 128) would pass the rule; the large record stays on the interleave until an A/B of the workloads that
    # reach it shows no loss (state.h MSB_LDS_COLUMNS_LARGE)
    2: dict(state_bytes=8336, columns=0, stride_mod128=16, column_lane_degree=1, move_store_degree=8, move_read_degree=16, area8=66688),
}


@pytest.mark.parametrize("ext", [False, True, 2], ids=["standard", "extended", "large"])
def test_map_bounds_round_trip_and_banks_under_sanitizers(tmp_path, ext):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "lds_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-psabi"] +
                   kernel_variants.BUILD_FLAGS[ext] +
                   ["-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "lds_layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok", r.stdout
    got = {words[i]: int(words[i + 1]) for i in range(1, len(words), 2)}
    for k, v in EXPECT[ext].items():
        assert got[k] == v, (k, got[k], v)
    # PlayLds<8>::TOTAL = origin + candidate area + 240 B of features + 8 work stacks of 21 words: room for 22 (registers allow 20),
    # 8 and 2 wavefronts per CU's 160 KiB on the standard, extended and large record, as before the columns
    total = got["origin"] + got["area8"] + 240 + 8 * 21 * 4
    assert total == {False: 7216, True: 20400, 2: 67888}[ext] and (160 * 1024) // total == {False: 22, True: 8, 2: 2}[ext], total
    assert got["reads"] > 700000 and got["bank_cases"] > 10000, got   # (every column of 5 lane counts x 2 maps, every offset and width)


def test_the_games_of_the_gpu_test_hold_every_case():
    """The oracle's line of the 64 games: a decision with 1, with U and with more than 2 U legal actions for every U of every
    build's variants, and scenario games that play all 40 decisions."""
    for ext in (False, True, 2):
        LL.check_cases(LL.line(ext), sorted({u for u, _ in kernel_variants.variants(ext)}))
