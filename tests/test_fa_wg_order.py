"""The workgroup order of the attention launches, checked on the host:
csrc/kernels/tests/fa_wg_order_test.cpp is a plain C++ program (no torch, no
HIP) over fa_wg_order of csrc/kernels/fa_layout.h, the function the three
kernels take their block from. It is built with the address and
undefined-behaviour sanitizers and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parent.parent / "csrc" / "kernels"


def test_fa_wg_order_program(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build csrc/kernels/tests/fa_wg_order_test.cpp")
    exe = tmp_path / "fa_wg_order_test"
    subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         str(KERNELS / "tests" / "fa_wg_order_test.cpp"), "-o", str(exe)],
        check=True,
    )
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "fa wg order ok" in proc.stdout
