"""The document-mask bounds of the flash-attention kernels, checked on the
host: csrc/kernels/tests/fa_doc_bounds_test.cpp is a plain C++ program (no
torch, no HIP) that walks the tile loops of the forward, dkdv and dq kernels
with the bound functions of csrc/kernels/fa_layout.h, the ones the kernels
call. For layouts DocMask builds the kept elements are exactly the visible
ones; for arbitrary int32 contents every tile index stays inside the causal
kernel's range. It is built with the address and undefined-behaviour
sanitizers and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parent.parent / "csrc" / "kernels"


def test_fa_doc_bounds_program(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build csrc/kernels/tests/fa_doc_bounds_test.cpp")
    exe = tmp_path / "fa_doc_bounds_test"
    subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         str(KERNELS / "tests" / "fa_doc_bounds_test.cpp"), "-o", str(exe)],
        check=True,
    )
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "fa doc bounds ok" in proc.stdout
