"""A model of goss_gpu_object_colour_reads and of `goss elect-reads` on top of it (`electus classify`, ElectApp.cc:406-451),
in plain Python integers over match_model.py (reads, windows, the FNV normal form).  Nothing here knows the library.

A k-mer set of sorted keys carries one colour word per rank: bit i says that reference i holds the k-mer.  Every valid
K-window of a read is looked up in its canonical form; the read's word is the OR of the words of the windows that are
present.  The decision is KmerFilter's: a single read matches when it has a window and its word has at least t bits; a
pair matches when its first mate does, or when its second mate has a window and the OR of both words is at least t --
as a number, which is what the reference compares at ElectApp.cc:443."""
import match_model as mm

SUFFIX = {"fasta": ".fasta", "fastq": ".fastq", "line": ".txt"}
KINDS = ("fasta", "fastq", "line")                # the order the kinds of input are processed in (ElectApp.cc:686-699)
MASK64 = (1 << 64) - 1


def popcount(x):
    return bin(x).count("1")


def read_word(read, K, rank_of, colours):
    """(word, windows) of one read: the loop of KmerFilter without its early return; rank_of: {key: rank}"""
    ws = mm.windows(read, K)
    word = 0
    for x in mm.canonical_many([(x, r) for _, x, r in ws]):
        r = rank_of.get(x)
        if r is not None:
            word |= colours[r]
    return word, len(ws)


def colour_reads(data, K, keys_sorted, colours):
    """(words[], windows[], by_count[65]) as goss_gpu_object_colour_reads answers"""
    assert list(keys_sorted) == sorted(set(keys_sorted)) and len(colours) == len(keys_sorted)
    assert all(0 <= c <= MASK64 for c in colours)
    rank_of = {x: i for i, x in enumerate(keys_sorted)}
    words, nwin, by_count = [], [], [0] * 65
    for b, e in mm.read_spans(data):
        m, w = read_word(data[b:e], K, rank_of, colours)
        words.append(m)
        nwin.append(w)
        by_count[popcount(m)] += 1
    return words, nwin, by_count


def elect_single(word, windows, t):
    """KmerFilter::push_back(GossReadPtr): the loop body runs once per window, so without a window nothing matches"""
    return windows >= 1 and popcount(word) >= t


def elect_pair(m1, w1, m2, w2, t, numeric_second_mate=True):
    """KmerFilter::push_back(ReadPair); numeric_second_mate=False: what was evidently meant"""
    both = m1 | m2
    return (w1 >= 1 and popcount(m1) >= t) or (w2 >= 1 and (both if numeric_second_mate else popcount(both)) >= t)


def elect(words, windows, t, pairs=False, numeric_second_mate=True):
    """what gossamer_amd.elect answers: one bool per read, or per pair of reads 2i and 2i + 1"""
    if not pairs:
        return [elect_single(m, w, t) for m, w in zip(words, windows)]
    return [elect_pair(words[i], windows[i], words[i + 1], windows[i + 1], t, numeric_second_mate) for i in range(0, len(words), 2)]


def file_name(prefix, fmt, half=None):
    """<prefix>[_1|_2]<suffix> (ElectApp.cc:553-558, 585-593)"""
    return prefix + ("_%d" % half if half else "") + SUFFIX[fmt]


def references(ref_sets):
    """(sorted union, colours) of the references' canonical k-mer sets, bit i for the i-th"""
    assert 1 <= len(ref_sets) <= 64
    keys = sorted(set().union(*ref_sets))
    return keys, [sum(1 << i for i, s in enumerate(ref_sets) if x in s) for x in keys]


def file_table(items, pairs, match_prefix, non_match_prefix):
    """[(name, kind, half, matched?)] of the files the command creates, in the order it creates them"""
    out = []
    for fmt in KINDS:
        if not any(f == fmt for f, _ in items):
            continue
        for half in ((1, 2) if pairs else (None,)):
            if match_prefix:
                out.append((file_name(match_prefix, fmt, half), fmt, half, True))
            if non_match_prefix:
                out.append((file_name(non_match_prefix, fmt, half), fmt, half, False))
    return out


def elect_reads(items, K, keys, colours, t=None, nrefs=None, pairs=False, match_prefix="", non_match_prefix="", numeric_second_mate=True):
    """({file name: bytes}, matched, unmatched) of goss elect-reads.  items: [(format, bytes)] in command-line order; each
    kind of input goes to files of its own suffix; t=None: the number of references"""
    if t is None:
        t = nrefs
    rank_of = {x: i for i, x in enumerate(keys)}
    files = {name: [] for name, _, _, _ in file_table(items, pairs, match_prefix, non_match_prefix)}
    matched = unmatched = 0

    def put(hit, fmt, half, read):
        prefix = match_prefix if hit else non_match_prefix
        if prefix:
            files[file_name(prefix, fmt, half)].append(read + b"\n")
    for fmt in KINDS:
        texts = [mm.PARSERS[fmt](t_) for f, t_ in items if f == fmt]
        if not pairs:
            for reads in texts:
                for r in reads:
                    hit = elect_single(*read_word(r, K, rank_of, colours), t)
                    matched, unmatched = matched + hit, unmatched + (not hit)
                    put(hit, fmt, None, r)
            continue
        if len(texts) % 2:
            raise ValueError("an even number of input files is required")
        for i in range(0, len(texts), 2):
            if len(texts[i]) != len(texts[i + 1]):
                raise ValueError("unequal read counts")
            hits = [elect_pair(*read_word(a, K, rank_of, colours), *read_word(b, K, rank_of, colours), t, numeric_second_mate)
                    for a, b in zip(texts[i], texts[i + 1])]
            matched, unmatched = matched + sum(hits), unmatched + len(hits) - sum(hits)
            for half in (1, 2):
                for hit, r in zip(hits, texts[i + half - 1]):
                    put(hit, fmt, half, r)
    return {n: b"".join(v) for n, v in files.items()}, matched, unmatched
