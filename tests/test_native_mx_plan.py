"""``plan_mx`` of the native launch planner (csrc/plan.h) checked on the CPU.

tests/native/mx_plan_check.cpp is a stand-alone program that includes only
the planner header; it is built here with the host compiler under
AddressSanitizer + UBSan and run as a plain executable.
"""

import subprocess
from pathlib import Path

import pytest

from tests.test_native_plan import CSRC, ROOT, _host_compiler

SOURCE = ROOT / "tests" / "native" / "mx_plan_check.cpp"


def test_mx_plan_check(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "mx_plan_check"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{CSRC}", str(SOURCE), "-o", str(exe)],
        capture_output=True, text=True,
    )
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mx_plan_check ok" in run.stdout
