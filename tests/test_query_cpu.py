"""CPU side of the query objects (goss_gpu_object_*): the k-mer encoder of the binding, the exported symbols, and
the refusals that come before any device is touched."""
import ctypes as C
import random

import pytest

import gossamer_amd as g


def test_encode_kmers_matches_the_oracle(oracle):
    rng = random.Random(31)
    for k in (1, 4, 25, 31, 32, 45, 63):
        seqs = ["".join(rng.choice("ACGTacgt") for _ in range(k)) for _ in range(200)]
        enc = g.encode_kmers(seqs, k)
        if 2 * k <= 62:
            assert enc.shape == (200,)
            got = [int(x) for x in enc]
        else:
            assert enc.shape == (200, 2)
            got = [int(lo) | (int(hi) << 64) for lo, hi in enc]
        assert got == [oracle.kmer_value(s) for s in seqs]
        # the reverse strand, encoded, is the oracle's reverse complement; both normalise alike
        comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
        rcs = ["".join(comp[c] for c in reversed(s.upper())) for s in seqs]
        enc_rc = g.encode_kmers(rcs, k)
        got_rc = [int(x) for x in enc_rc] if 2 * k <= 62 else [int(lo) | (int(hi) << 64) for lo, hi in enc_rc]
        assert got_rc == [oracle.revcomp(v, k) for v in got]
        assert [oracle.normalize(v, k) for v in got] == [oracle.normalize(v, k) for v in got_rc]
    with pytest.raises(ValueError):
        g.encode_kmers(["ACGN"], 4)
    with pytest.raises(ValueError):
        g.encode_kmers(["ACG"], 4)


def test_object_symbols_are_exported():
    L = g.load()
    names = [s for s in g.SYMBOLS if s.startswith("goss_gpu_object_")]
    assert sorted(names) == sorted(["goss_gpu_object_open", "goss_gpu_object_open_emitted", "goss_gpu_object_close",
                                    "goss_gpu_object_last_error", "goss_gpu_object_info", "goss_gpu_object_rank",
                                    "goss_gpu_object_select", "goss_gpu_object_multiplicity", "goss_gpu_object_lookup",
                                    "goss_gpu_object_node_ranks"])
    for n in names:
        assert hasattr(L, n), n


def test_object_arguments_are_checked_before_the_device():
    L = g.load()
    h = C.c_void_p()
    L.goss_gpu_object_open.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_uint32]
    assert L.goss_gpu_object_open(C.byref(h), 0, None, 7, b"x", None, 0) == -1          # no such kind
    assert L.goss_gpu_object_open(C.byref(h), 0, None, 0, None, None, 0) == -1          # no base name
    L.goss_gpu_object_open_emitted.argtypes = [C.POINTER(C.c_void_p), C.c_void_p]
    assert L.goss_gpu_object_open_emitted(C.byref(h), None) == -1
    L.goss_gpu_object_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    assert L.goss_gpu_object_rank(None, None, 0, 0, None, None) == -1


def test_object_open_without_a_device_fails_loudly(oracle):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    files = oracle.write_kmer_set([1, 2, 3], 25, out="ks")
    with pytest.raises(g.GossGpuError) as e:
        g.Object.open(files, "ks", g.OBJECT_KMER_SET)
    assert e.value.status == -2          # GOSS_ERR_NO_DEVICE: there is no CPU fallback
