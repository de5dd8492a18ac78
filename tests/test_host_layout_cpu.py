"""The host side's workspace layouts (monsoon_amd/csrc/host_layout.h) and the owner of the handle's device memory
(host_mem.h), on the host: tests/host_layout_check.cpp is compiled with the address and UB sanitizers into a stand-alone
program and run (never loaded into Python), once with each record build's constants.  Layouts: alignment, disjoint
fields inside the total, and the totals the allocations have always had, at caps 1, 63, 64, 65, 2 048, 65 536 and
1 048 576.  Owner: a counting allocator fails the k-th allocation of a handle-like life, for every k; everything is freed
exactly once, a failed replace leaves null / 0, a failed retire leaves the old block in use, retired blocks live until
destroy.  The sanitizers' leak check and the program's own live set are the judges."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = 7
# per cap: env, opp, five uses of d_bytes, results, 2 x 4 logs; then the GA packing: 3 dims x 5 lambdas x 2 mus
N_LAYOUTS = CAPS * (1 + 1 + 5 + 1 + 8) + 3 * 5 * 2
# allocations of the life the check program plays: 4 fixed + first overflow block + 2 replaces + 2 retires + 3 temporaries + 1 adopted
N_LIVES = 1 + (4 + 1 + 2 + 2 + 3 + 1)


@pytest.mark.parametrize("ext", [0, 1, 2], ids=["std", "ext", "big"])
def test_layouts_and_owner_under_sanitizers(tmp_path, ext):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler builds the oracle too"
    exe = str(tmp_path / "host_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-DMSB_EXT={ext}",
                    "-I", os.path.join(REPO, "monsoon_amd", "csrc"), os.path.join(REPO, "tests", "host_layout_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == N_LAYOUTS and int(words[3]) == N_LIVES, r.stdout
    # the three record builds differ in the record size the state blob carries: this run saw its own
    assert int(words[6]) > 0 and int(words[6]) % 16 == 0, r.stdout
