"""gossamer_amd/csrc/goss_words.hpp under the system's C++ compiler: tests/words_check.cpp (its own main) built and run
here -- the image of a remainder is a bijection, home and second bucket differ for every table size, the marker of a
bucket lives where the counting kernel's comment says, the squeeze round-trips, and what the first level stores in
the squeeze form is rebuilt by the second level into today's remainder and digit.  Then the Python mirror
(tests/words_model.py) against the vectors the program prints."""
import os
import shutil
import subprocess

import pytest

import words_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("words") / "words_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "gossamer_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "words_check.cpp")], check=True, timeout=300)
    p = subprocess.run([exe], stdout=subprocess.PIPE, timeout=300)
    return p.returncode, p.stdout.decode()


def test_word_functions_hold_their_properties(check_output):
    rc, out = check_output
    assert rc == 0, out[-2000:]
    oks = [l for l in out.splitlines() if l.startswith("ok ")]
    assert len(oks) == 1 + 4 + 1 + 1, out[-2000:]
    assert "FAILED" not in out


def test_python_mirror_matches_the_header(check_output):
    rc, out = check_output
    vecs = [tuple(int(x) for x in l.split()[1:]) for l in out.splitlines() if l.startswith("vec ")]
    assert rc == 0 and len(vecs) == 64
    for x, mix, image, unimage, unpack, marker in vecs:
        assert wm.r32_mix(x) == mix and wm.r32_unmix(mix) == x
        assert wm.r32_image(x) == image and wm.r32_unimage(x) == unimage and wm.r32_unimage(image) == x
        assert wm.rem32_unpack_sq(x, 24) == unpack
        assert wm.r32_image_marker(x % 4096) == marker
    for nb in (512, 1024, 2048, 4096):
        for b in (0, 1, 2, 77, nb - 1):
            m = wm.r32_image_marker(b)
            h = wm.r32_image_home(m, nb)
            assert h == b ^ 1 and wm.r32_image_second(m, h, nb) == b ^ 2
