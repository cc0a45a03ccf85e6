"""gossamer_amd/csrc/goss_knobs.hpp under the system's C++ compiler and its address and undefined-behaviour
sanitizers: tests/knobs_check.cpp (its own main) built and run here -- knobs_from_env against the acceptance rule of
every GOSS_GPU_* variable that goss_gpu_create reads (an accepted text, and the texts just outside the rule), stat_lookup
over every name goss_gpu_stat serves from the table, and Scoped on normal exit, on an exception and nested."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knobs_stats_and_scoped(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "knobs_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "gossamer_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "knobs_check.cpp")],
                   check=True, timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert [l for l in out.splitlines() if l.startswith("ok ")] == ["ok defaults", "ok knobs", "ok stats", "ok scoped"], out[-3000:]
    assert "FAILED" not in out
