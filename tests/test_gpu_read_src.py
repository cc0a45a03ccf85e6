"""The three kinds of input a count reads from -- bytes in HBM, packed bases, super-k-mer records (goss_read_src.hpp) --
pushed so that ONE push is cut into several chunks: every chunk but the first then begins at a source advanced from
the push's own (a byte address that keeps its misalignment, a position inside the packed arrays, a record further on).
40 000 reads of 150 bp over a genome of 50 000 bases: six million window starts, while 64 MB of arena hold 1.7 M of
one-word k-mers (37 bytes a key; 0.86 M graph edges' windows, 1.0 M two-word k-mers) -- four chunks and more, whose runs
of at most 10^5 keys stay far below the quarter of the arena at which they would be merged: ctx.stat("runs") after the
push is the number of chunks.  Everything against the oracle's files."""
import os

import pytest
import torch

import gossamer_amd as g

pytestmark = pytest.mark.gpu
MB = 1 << 20
NREADS, READ_LEN, GENOME = 40_000, 150, 50_000


@pytest.fixture(scope="module")
def reads():
    return g.synth_reads_host(NREADS, READ_LEN, GENOME, seed=21)


@pytest.fixture(scope="module")
def expected(oracle, reads):
    """(k, mode) -> (the oracle's files by suffix, its window count): built once per key space"""
    memo = {}

    def get(k, mode):
        if (k, mode) not in memo:
            build = oracle.build_graph if mode else oracle.build_kmer_set
            exp, nwin = build([(oracle.LINE, "r", reads)], k, out="o")
            memo[(k, mode)] = ({n[1:]: d for n, d in exp.items()}, nwin)
        return memo[(k, mode)]
    return get


def quarters(reads):
    per = NREADS // 4 * (READ_LEN + 1)
    return [reads[i * per:(i + 1) * per] for i in range(4)]


def on_device(data, off=0):
    """the bytes at `off` past a 16-byte boundary of device memory; returns (tensor kept alive, address)"""
    t = torch.zeros(len(data) + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[off:off + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return t, t.data_ptr() + off


def packed_on_device(ctx, data):
    t, ptr = on_device(data)
    groups = (len(data) + 15) // 16
    dc = torch.empty(groups, dtype=torch.int32, device="cuda")
    db = torch.empty(groups, dtype=torch.int16, device="cuda")
    ctx.pack_bases_device(ptr, len(data), dc.data_ptr(), db.data_ptr())
    return dc, db


def routed_records(k, mode, data):
    """the records of `data` in one part: (tensor, records, windows)"""
    t, ptr = on_device(data)
    rb = g.binding.record_bytes(k, mode)
    with g.Context(k, mode, hbm_budget=64 * MB) as rctx:
        one = torch.empty(rb, dtype=torch.uint8, device="cuda")
        need, _, _ = rctx.route_records(ptr, len(data), 1, one.data_ptr(), [0], [1])          # (too small: says what the part needs)
        buf = torch.empty(need[0] * rb, dtype=torch.uint8, device="cuda")
        recs, wins, ok = rctx.route_records(ptr, len(data), 1, buf.data_ptr(), [0], need)
    assert ok and recs == need
    return buf, recs[0], wins[0]


def finish_and_compare(ctx, exp, nwin):
    c = ctx.finish()
    assert c.windows == nwin
    got = ctx.emit()
    assert sorted(got) == sorted(exp)
    for name in exp:
        assert got[name] == exp[name], name


@pytest.mark.parametrize("off", [1, 7, 15])
@pytest.mark.parametrize("k,mode", [(25, g.MODE_KMER_SET), (27, g.MODE_GRAPH)])
def test_bytes_in_hbm_in_chunks_at_a_misalignment(expected, reads, k, mode, off):
    exp, nwin = expected(k, mode)
    t, ptr = on_device(reads, off)
    with g.Context(k, mode, hbm_budget=64 * MB) as ctx:
        ctx.push_device(ptr, len(reads))
        runs = ctx.stat("runs")
        print("chunks:", runs)
        assert runs >= 3
        finish_and_compare(ctx, exp, nwin)


@pytest.mark.parametrize("k", [25, 45])
def test_packed_bases_in_hbm_in_chunks(expected, reads, k):
    exp, nwin = expected(k, g.MODE_KMER_SET)
    with g.Context(k, g.MODE_KMER_SET, hbm_budget=64 * MB) as ctx:
        dc, db = packed_on_device(ctx, reads)
        ctx.push_packed_device(dc.data_ptr(), db.data_ptr(), len(reads))
        st = {n: ctx.stat(n) for n in ("runs", "packed_unpacked_chunks", "packed_fused_chunks")}
        print("plain:", st)
        assert st["runs"] >= 3 and st["packed_unpacked_chunks"] >= 3, st          # (every chunk unpacked from its own position)
        finish_and_compare(ctx, exp, nwin)
    # the fused kernels read the packed string as it is: an arena that holds chunks of the size they take (10^6 keys and more)
    os.environ["GOSS_GPU_FUSED_MIN"] = "0"
    try:
        with g.Context(k, g.MODE_KMER_SET, hbm_budget=160 * MB) as ctx:
            dc, db = packed_on_device(ctx, reads)
            ctx.push_packed_device(dc.data_ptr(), db.data_ptr(), len(reads))
            st = {n: ctx.stat(n) for n in ("runs", "packed_unpacked_chunks", "packed_fused_chunks", "fused_chunks")}
            print("fused:", st)
            assert st["packed_fused_chunks"] > 0, st
            finish_and_compare(ctx, exp, nwin)
    finally:
        os.environ.pop("GOSS_GPU_FUSED_MIN", None)


@pytest.mark.parametrize("k", [25, 45])          # 12-byte and 20-byte records
def test_records_in_chunks(expected, reads, k):
    exp, nwin = expected(k, g.MODE_KMER_SET)
    buf, nrec, win = routed_records(k, g.MODE_KMER_SET, reads)
    assert win == nwin
    with g.Context(k, g.MODE_KMER_SET, hbm_budget=64 * MB) as ctx:
        ctx.push_records(buf.data_ptr(), nrec, win)
        runs = ctx.stat("runs")
        print("chunks:", runs, "records:", nrec)
        assert runs >= 3
        finish_and_compare(ctx, exp, nwin)          # (windows too: a chunk boundary inside a record would lose or double some)


def test_one_context_takes_the_three_kinds_in_a_row(expected, reads):
    """packed, bytes, records, packed -- a quarter of the reads each: nothing of one push's kind survives into the next"""
    k = 25
    exp, nwin = expected(k, g.MODE_KMER_SET)
    q = quarters(reads)
    buf, nrec, win = routed_records(k, g.MODE_KMER_SET, q[2])
    with g.Context(k, g.MODE_KMER_SET, hbm_budget=64 * MB) as ctx:
        dc0, db0 = packed_on_device(ctx, q[0])
        ctx.push_packed_device(dc0.data_ptr(), db0.data_ptr(), len(q[0]))
        t1, ptr1 = on_device(q[1], 5)
        ctx.push_device(ptr1, len(q[1]))
        ctx.push_records(buf.data_ptr(), nrec, win)
        dc3, db3 = packed_on_device(ctx, q[3])
        ctx.push_packed_device(dc3.data_ptr(), db3.data_ptr(), len(q[3]))
        assert ctx.stat("runs") >= 4
        finish_and_compare(ctx, exp, nwin)


def test_a_packed_staging_buffer_is_routed(expected, reads):
    """A deferred context stages packed bases and a group of that one member routes them: the records, counted by the
    member itself, hold what the reads hold."""
    k = 25
    exp, nwin = expected(k, g.MODE_KMER_SET)
    with g.Context(k, g.MODE_KMER_SET, hbm_budget=512 * MB) as ctx:
        ctx.set_deferred(True)
        windows = 0
        for part in quarters(reads):
            ctx.push_packed_host(part)
            st = g.group_route_exchange([ctx])
            assert st["records"] > 0
            windows += st["windows"]
        assert windows == nwin
        finish_and_compare(ctx, exp, nwin)
