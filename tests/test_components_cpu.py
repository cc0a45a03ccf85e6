"""count-components without a GPU: the model of components_model.py pinned to the reference's own loop, the exactness
of the printed doubles on the test inputs, and the command's registration and option errors."""
import os
import subprocess
from bisect import bisect_left

import pytest

import components_model as cm
import tips_cases
import tips_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOSS = os.environ.get("GOSS_BIN") or os.path.join(ROOT, "gossamer_amd", "goss")
READS = dict(genome_len=3000, coverage=20, error_rate=0.01, seed=3)


def reference_rows(edges, counts, K, marked=None):
    """GossCmdCountComponents.cc:89-127, 244-258 restated as it stands: one bitset, one stack of nodes, every marked
    edge out of a node and every marked edge into it (the reverse complements of the edges out of rc(node)).
    [(Size, Min, Max, Sum, Sum2)] per component in the order the scan opens them -- the start edge is added before
    follow() meets it still marked and adds it again."""
    n = len(edges)
    node_mask = (1 << (2 * K)) - 1
    rank = {e: i for i, e in enumerate(edges)}
    on = [True] * n if marked is None else list(marked)

    def begin_end(node):
        return bisect_left(edges, node << 2), bisect_left(edges, (node + 1) << 2)

    rows = []
    for i in range(n):
        if not on[i]:
            continue
        info = [0, (1 << 64) - 1, 0, 0, 0]

        def add(c):
            info[0] += 1
            info[1] = min(info[1], c)
            info[2] = max(info[2], c)
            info[3] = (info[3] + c) & cm.MASK64
            info[4] = (info[4] + c * c) & cm.MASK64

        add(counts[i])
        stack = [edges[i] >> 2]
        while stack:
            node = stack.pop()
            lo, hi = begin_end(node)
            for r in range(lo, hi):
                if on[r]:
                    on[r] = False
                    add(counts[r])
                    stack.append(edges[r] & node_mask)
            lo, hi = begin_end(tm.revcomp(node, K))
            for rrc in range(lo, hi):
                r = rank[tm.revcomp(edges[rrc], K + 1)]
                if on[r]:
                    on[r] = False
                    add(counts[r])
                    stack.append(edges[r] >> 2)
        rows.append(tuple(info))
    return rows


def rows_text(rows):
    import math
    out = ["Comp\tSize\tMin\tMax\tMean\tStd Dev\n"]
    for i, (size, lo, hi, s, s2) in enumerate(rows):
        out.append("%d\t%d\t%d\t%d\t%g\t%g\n" % (i, size, lo, hi, s / float(size), math.sqrt(float(size) * s2 - float(s) * s) / size))
    return "".join(out).encode()


_inputs = {}


def inputs(oracle):
    """[(name, edges, counts, K, marked or None)]: the hand-made graphs, the read graphs, and the read graph of K = 27
    under marks that a part of its reads leaves"""
    if not _inputs:
        got = []
        for K in (15, 30, 55):
            edges, counts, _ = tips_cases.combined_graph(K)
            got.append(("combined %d" % K, edges, counts, K, None))
        reads = tips_cases.error_reads(**READS)
        for K in (27, 33):
            edges, counts, _, _ = oracle.count([(oracle.LINE, "r", reads)], K + 1, 1)
            got.append(("reads %d" % K, edges, counts, K, None))
            if K == 27:
                part = "\n".join(reads.split("\n")[::7])
                got.append(("reads 27 marked", edges, counts, K, cm.marks(edges, K, part)[0]))
        _inputs["all"] = got
    return _inputs["all"]


def test_model_agrees_with_the_reference_loop(oracle):
    for name, edges, counts, K, marked in inputs(oracle):
        labels, table = cm.components(edges, counts, K, marked)
        rows = reference_rows(edges, counts, K, marked)
        assert len(rows) == len(table) >= 2, name
        for (size, lo, hi, s, s2), (start, n, tlo, thi, ts, ts2, _) in zip(rows, table):
            m = counts[start]
            assert (size, lo, hi, s, s2) == (n + 1, tlo, thi, (ts + m) & cm.MASK64, (ts2 + m * m) & cm.MASK64), name
        assert cm.reference_table(table, counts) == rows_text(rows), name
        # the labels say what the table says
        assert sum(1 for x in labels if x != cm.NONE) == sum(r[1] for r in table), name
        assert [labels.index(c) for c in range(len(table))] == [r[0] for r in table], name
        assert [r[0] for r in table] == sorted(r[0] for r in table), name
    assert any(marked is not None and not all(marked) for _, _, _, _, marked in inputs(oracle))


def test_printed_doubles_are_exact_on_the_test_inputs(oracle):
    """Every Size * Sum2 stays below 2^53: the expression under the root is computed exactly and is not negative, so
    '%g' of the Python float is what the stream prints for the C++ double."""
    for name, edges, counts, K, marked in inputs(oracle):
        for size, lo, hi, s, s2 in reference_rows(edges, counts, K, marked):
            assert size * s2 < 1 << 53 and s * s < 1 << 53, name
            assert size * s2 - s * s >= 0, name
            assert float(size) * s2 - float(s) * s == size * s2 - s * s, name


def run_goss(*args):
    p = subprocess.run([GOSS] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


def test_command_is_registered_and_checks_its_options(tmp_path):
    if not os.path.exists(GOSS):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gossamer_amd", "csrc"), "all"])
    rc, _, err = run_goss("count-components")
    assert rc == 1 and err.startswith("mandatory option graph-in was not given.\nuse\n\tgoss count-components -h\n"), err
    rc, _, err = run_goss("count-components", "-G", "a", "-G", "b")
    assert rc == 1 and err.startswith("mandatory option graph-in must be supplied exactly once.\n"), err
    rc, _, err = run_goss("count-components", "-G", "a", "--bogus")
    assert rc == 1 and err == "unknown option '--bogus'\nuse\n\tgoss count-components -h\nfor more usage information.\n"
    rc, _, err = run_goss("count-components", "-G", "a", "--line-in", str(tmp_path / "missing.txt"))
    assert rc == 1 and "\tcannot open file '%s' for reading\n" % (tmp_path / "missing.txt") in err
    rc, _, err = run_goss("help")
    assert "count-components  count connected components in the graph represented by the given reads\n" in err
    rc, _, err = run_goss("count-components", "-h")
    assert rc == 1 and "--graph-out" in err and "--line-in" in err
