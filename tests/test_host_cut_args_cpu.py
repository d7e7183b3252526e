"""The argument checks of lsf_cut_cells_band (levelsetfortran_amd/csrc/lsf_host_args_cut.hpp) on the CPU: tests/host_args/
cut_cells_args_main.cpp runs a table of argument lists through cut_cells_args_ok and prints one line per case, held line for line
against tests/golden/cut_cells_args_messages.txt.  No GPU and no library: the header is compiled into a stand-alone program."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import GOLDEN as GOLDEN_DIR, ROOT

HEADER = os.path.join(ROOT, "levelsetfortran_amd", "csrc", "lsf_host_args_cut.hpp")
GOLDEN = os.path.join(GOLDEN_DIR, "cut_cells_args_messages.txt")


@pytest.fixture(scope="module")
def lines():
    src = os.path.join(ROOT, "tests", "host_args", "cut_cells_args_main.cpp")
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    assert cxx, "no host C++ compiler (c++, or ROCm's clang++)"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "cut_cells_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-Wno-unused-function", "-o", exe, src], check=True)
        return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_every_case_gives_the_recorded_code_and_message(lines):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for n, (g, w) in enumerate(zip(lines, want), 1):
        assert g == w, f"line {n}"
    assert len(lines) == len(want) >= 50


def test_valid_lists_pass_and_every_other_is_refused_in_the_call_s_name(lines):
    for line in lines:
        name, rc, msg = (p.strip() for p in line.split("|"))
        valid = name.startswith("valid")
        assert int(rc) == (0 if valid else 2), name
        assert (msg == "") == valid, name
        # (the dimensions are refused in the shared words of lsf_reinit_band's check, which carry no call name)
        assert valid or msg.startswith("lsf_cut_cells_band: ") or msg in ("nx, ny, nz must be >= 2", "field too large",
                                                                           "a k-plane of the field exceeds 2 GB"), name


def test_the_table_reaches_every_refusal_of_the_header(lines):
    """every piece of message text in the header -- a string literal of a line with fail( or grid_ok(, or of the line that continues
    one -- is part of some refused case's message; so is every pair overlap_ok can name"""
    with open(HEADER) as f:
        code = [ln for ln in f.read().splitlines() if "fail(" in ln or "grid_ok(" in ln or ln.lstrip().startswith('"')]
    pieces = [s for ln in code for s in re.findall(r'"([^"]+)"', ln)]
    assert len(pieces) >= 9
    messages = [ln.split(" | ", 2)[2] for ln in lines if " | 2 | " in ln]
    unreached = [s for s in pieces if not any(s in m for m in messages)]
    assert not unreached, unreached
    for needle in ("1 of 3 given", "2 of 3 given", "nothing is requested", "vof overlaps phi", "vof overlaps mask", "ax overlaps phi",
                   "ax overlaps vof", "ay overlaps mask", "ay overlaps ax", "az overlaps ay", "az overlaps vof", "bx overlaps az",
                   "bx overlaps phi", "by overlaps bx", "by overlaps mask", "bz overlaps by", "bz overlaps vof", "bz overlaps ax",
                   "nx, ny, nz must be >= 2", "field too large", "a k-plane of the field exceeds 2 GB", "more than 2^31 - 1 points"):
        assert any(needle in m for m in messages), needle


def test_the_header_includes_nothing():
    """it depends on include/lsf.h, <cmath>, <cstdint>, <string>, fail() and the shared checks of lsf_host_args.hpp alone"""
    with open(HEADER) as f:
        assert "#include" not in f.read()
