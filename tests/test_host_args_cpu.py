"""The argument checks of every call (levelsetfortran_amd/csrc/lsf_host_args.hpp) on the CPU: tests/host_args/host_args_main.cpp runs a
table of argument lists through check_dims and every *_args_ok, and its output -- return code and lsf_last_error() text of every case
-- is the recorded tests/golden/host_args_messages.txt, line for line."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_args", "host_args_main.cpp")
HEADER = os.path.join(ROOT, "levelsetfortran_amd", "csrc", "lsf_host_args.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_args_messages.txt")


# the host compiler, and ROCm's clang++ as the fall-back where there is none: both are held to the record wherever both exist
COMPILERS = [c for c in (shutil.which("c++"), shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")) if c]


@pytest.fixture(scope="module", params=COMPILERS or [None], ids=lambda c: os.path.basename(c or "none"))
def lines(request, tmp_path_factory):
    cxx = request.param
    assert cxx, "no host C++ compiler (c++, or ROCm's clang++)"
    exe = str(tmp_path_factory.mktemp("host_args") / "host_args")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-o", exe, SRC], check=True)
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_every_case_gives_the_recorded_code_and_message(lines):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for n, (g, w) in enumerate(zip(lines, want), 1):
        assert g == w, f"line {n}"
    assert len(lines) == len(want)


def test_the_table_reaches_every_refusal_of_the_header(lines):
    """every piece of message text in the header -- a string literal of a line with fail( or grid_ok(, or of the line that continues
    one -- is part of some refused case's message"""
    with open(HEADER) as f:
        code = [ln for ln in f.read().splitlines() if "fail(" in ln or "grid_ok(" in ln or ln.lstrip().startswith('"')]
    pieces = [s for ln in code for s in re.findall(r'"([^"]+)"', ln)]
    assert len(pieces) >= 100
    messages = [ln.split(" | ", 2)[2] for ln in lines if " | 2 | " in ln]
    unreached = [s for s in pieces if not any(s in m for m in messages)]
    assert not unreached, unreached


def test_the_header_includes_nothing():
    """it depends on include/lsf.h, <cmath>, <cstdint>, <string> and fail() alone: the program above gives it nothing else"""
    with open(HEADER) as f:
        assert "#include" not in f.read()
