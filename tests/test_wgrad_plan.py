"""CPU check of the wgrad launchers' split-K plan: builds
tests/host/wgrad_plan_check.cpp (a stand-alone program around
ops/hip/wgrad_plan.h, the header the launchers themselves call) with
AddressSanitizer and UBSan and runs it.  No GPU involved."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "wgrad_plan_check.cpp")
INC = os.path.join(ROOT, "howtotrainyourmamlpytorch_amd", "ops", "hip")


def _compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


@pytest.mark.skipif(_compiler() is None, reason="no C++ compiler found")
def test_wgrad_plan_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wgrad_plan_check")
    cxx = _compiler()
    # the sanitizer runtimes are linked into the program (clang's default;
    # gcc links them dynamically unless told otherwise)
    static = ([] if "clang" in os.path.basename(cxx)
              else ["-static-libasan", "-static-libubsan"])
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", *static, "-I", INC, SRC,
           "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
