"""Regenerates tests/golden/host_args_messages.txt: the output of tests/host_args/host_args_main.cpp, one line per argument list
(case | return code | message).  The committed file was recorded from check_dims and the *_args_ok functions as they were moved,
unedited, into levelsetfortran_amd/csrc/lsf_host_args.hpp; tests/test_host_args_cpu.py holds every later version to it.  Run it
again only when a call's checks are meant to change, and review the diff of the text file line by line.

    python tests/golden/make_host_args_messages.py
"""
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "..", "host_args", "host_args_main.cpp")

if __name__ == "__main__":
    cxx = shutil.which("c++") or shutil.which("clang++", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "host_args")
        subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, SRC], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(HERE, "host_args_messages.txt"), "w") as f:
        f.write(out)
    print(len(out.splitlines()), "cases")
