"""The hot-kernel instantiations (U candidate lanes per game, W waves per SIMD) of every record build, read from
monsoon_amd/csrc/variants.def the way its Makefile reads them, so that a new instantiation is tested without editing a
test."""
import os
import re
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS_DEF = os.path.join(REPO, "monsoon_amd", "csrc", "variants.def")
BUILD_FLAGS = {False: [], True: ["-DMSB_EXT=1"], 2: ["-DMSB_EXT=2"]}
BUILD_NAMES = {False: "standard", True: "extended", 2: "large"}


def variants(ext):
    """[(U, W), ...] of a build; the first one is its default."""
    cc = shutil.which("gcc") or shutil.which("cpp")
    args = [cc, "-E", "-P"] + BUILD_FLAGS[ext] + ["-x", "c", "-DMSB_LIST", VARIANTS_DEF]
    out = subprocess.run(args, capture_output=True, text=True, check=True).stdout
    return [(int(u), int(w)) for u, w in re.findall(r"X\((\d+),\s*(\d+)\)", out)]


def matrix():
    """[(build, U, W)] over the three builds, and pytest ids such as "standard-8x5"."""
    cases = [(ext, u, w) for ext in (False, True, 2) for u, w in variants(ext)]
    return cases, [f"{BUILD_NAMES[e]}-{u}x{w}" for e, u, w in cases]


def select(monkeypatch, u, w):
    """Make the next handle run variant (u, w): the library reads MONSOON_LANES / MONSOON_WPE in monsoon_create."""
    monkeypatch.setenv("MONSOON_LANES", str(u))
    monkeypatch.setenv("MONSOON_WPE", str(w))
