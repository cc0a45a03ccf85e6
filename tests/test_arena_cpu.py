"""gossamer_amd/csrc/goss_arena.hpp under the system's C++ compiler and its address and undefined-behaviour
sanitizers: tests/arena_check.cpp (its own main) built and run here -- an Arena over a few KB of host memory: both ends
align to 256 bytes, each refuses with GOSS_ERR_OOM and its own text where the two would cross, and an ArenaScope puts the
temporary end back on normal exit, on an exception, nested, and after an early rewind, and never touches the permanent
end."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_and_scope(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "arena_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "gossamer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "arena_check.cpp")],
                   check=True, timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert [l for l in out.splitlines() if l.startswith("ok ")] == ["ok align", "ok oom", "ok scope", "ok rewind"], out[-3000:]
    assert "FAILED" not in out
