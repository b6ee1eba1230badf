"""The native launch planner (csrc/plan.h) checked on the CPU.

tests/native/plan_check.cpp is a stand-alone program that includes only the
planner header; it is built here with the host compiler under
AddressSanitizer + UBSan and run as a plain executable.
"""

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "torchstore_amd" / "csrc"
SOURCE = ROOT / "tests" / "native" / "plan_check.cpp"


def _host_compiler():
    names = [os.environ.get("CXX"), "g++", "clang++", "c++",
             "/opt/rocm/llvm/bin/clang++"]
    for name in names:
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_planner_header_is_hip_free():
    """plan.h includes the three standard headers it is allowed and no more."""
    includes = [
        line.split()[1]
        for line in (CSRC / "plan.h").read_text().splitlines()
        if line.startswith("#include")
    ]
    assert sorted(includes) == ["<cstdint>", "<stdexcept>", "<vector>"]


def test_plan_check(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "plan_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{CSRC}", str(SOURCE), "-o", str(exe)],
        capture_output=True, text=True,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_check ok" in run.stdout
