"""The lean Estimate chain's host-checkable arithmetic (csrc/chain_owner_host.h: block ownership,
the opening split, the t-th qualifying row from per-block counts, the rotation rank and the run
table's fresh-copy constant): the stand-alone program tests/host/chain_owner_host_check.cpp, built
with the host sanitizers and run on the CPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_program_under_the_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "chain_owner_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "chain_owner_host_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert "chain owner host checks ok" in done.stdout
