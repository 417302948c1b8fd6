"""The address map of the fused QKV split + rotary kernels, checked on the
host: csrc/kernels/tests/qkv_layout_test.cpp is a plain C++ program (no torch,
no HIP) over the functions of csrc/kernels/qkv_layout.h, the ones the kernels
call. It is built with the address and undefined-behaviour sanitizers and run
as a child process. Out-of-range rotary positions are checked only here, on
`rope_pos_row`; no GPU test feeds them."""

import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parent.parent / "csrc" / "kernels"


def test_qkv_layout_program(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build csrc/kernels/tests/qkv_layout_test.cpp")
    exe = tmp_path / "qkv_layout_test"
    subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         str(KERNELS / "tests" / "qkv_layout_test.cpp"), "-o", str(exe)],
        check=True,
    )
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "qkv layout ok" in proc.stdout
