"""CPU-only: the whole `goss` command-line surface -- help, unknown and misspelt options, every missing mandatory option,
every numeric option with a non-number, the limit cases, the order in which competing errors win and the files the checks
leave behind -- replayed from tests/golden/cli_surface.json (tests/golden/make_cli_surface.py).  Every entry is decided
before a command object runs, so the answers are the same with and without a GPU."""
import difflib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import gossamer_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")          # (GOSS_BIN: a sanitizer build, tools/host_asan.sh)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_cli_surface as surface  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (os.path.exists(g.binding.LIB_PATH) and os.path.exists(GOSS)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])


@pytest.fixture(scope="module")
def entries():
    return surface.load()


def test_corpus_covers_every_command(entries):
    """The five entries every command has, and the rules that keep command objects out of the corpus."""
    argvs = [e["argv"] for e in entries]
    assert len(surface.COMMANDS) == 28
    for c in surface.COMMANDS:
        for tail in ([], ["-h"], ["--bogus"], ["--bogus", "-h"]):
            assert [c] + tail in argvs, (c, tail)
        if c not in surface.NO_G:
            assert any(a[:5] == [c, "-G", "a", "-G", "b"] for a in argvs), c
    for e in entries:
        assert surface.refuse(e["argv"], e["status"], e["stderr"], e["files"]) is None, e["argv"]
    assert argvs == [a for a, _ in surface.invocations()]


def test_goss_answers_as_recorded(entries):
    def replay(e):
        return surface.run_entry(GOSS, e["argv"], e["files"])

    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(replay, entries))
    wrong = []
    for e, now in zip(entries, got):
        for field, was, is_ in zip(("status", "stdout", "stderr", "listing"), (e["status"], e["stdout"], e["stderr"], e["listing"]), now):
            if was != is_:
                if isinstance(was, str):
                    was, is_ = "".join(difflib.unified_diff(was.splitlines(True), is_.splitlines(True), "recorded", "got", n=1)), ""
                wrong.append("goss %s: %s\n%s %s" % (" ".join(e["argv"][:12]), field, was, is_))
    assert not wrong, "%d differences in %d entries:\n%s" % (len(wrong), len(entries), "\n".join(wrong[:10]))
