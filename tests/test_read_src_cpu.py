"""gossamer_amd/csrc/goss_read_src.hpp under the system's C++ compiler and its address and undefined-behaviour
sanitizers: tests/read_src_check.cpp (its own main) built and run here -- ReadSrc's advance, launch arguments and
round-up to sixteen against the arithmetic they replace, for bytes at every misalignment, packed strings at positions
on and off group boundaries, and records of 12 and 20 bytes cut into chunks of whole multiples of 4096 slots."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_src_matches_the_old_arithmetic(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "read_src_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "gossamer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "read_src_check.cpp")],
                   check=True, timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert [l for l in out.splitlines() if l.startswith("ok ")] == ["ok bytes", "ok packed", "ok records 12", "ok records 20"], out[-3000:]
    assert "FAILED" not in out
