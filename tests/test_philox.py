"""csrc/kernels/tests/philox_test.cpp (the Philox4x32-10 known answers and sr_bf16
over all 65536 draws; plain C++ over csrc/kernels/philox.h, no torch, no HIP),
built with the address and undefined-behaviour sanitizers and run as a child
process, as tests/test_table_layout.py does."""
import shutil
import subprocess
from pathlib import Path

SRC = Path(__file__).resolve().parent.parent / "csrc" / "kernels" / "tests" / "philox_test.cpp"


def test_philox_program(tmp_path):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build csrc/kernels/tests/philox_test.cpp"
    exe = tmp_path / "philox_test"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(SRC), "-o", str(exe)], check=True)
    proc = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0 and "philox ok" in proc.stdout, proc.stdout + proc.stderr
