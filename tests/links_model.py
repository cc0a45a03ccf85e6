"""Pure-Python model of read links: the reads threaded over the linear segments of a graph.

Written from the semantics of the reference's thread-reads "mapping reads" stage (ReadLinker::push_back,
GossCmdThreadReads.cc:321-402, over KmerAligner::kmerSegment, KmerAligner.hh:169-229), not from its text.  The graph
is a set of edges, (K+1)-mers as Python ints with the first base in the most significant used bits; linear paths are
found by walking.  Python integers and dicts only.

  segment      a linear path as build-entry-edge-set defines them (entries_model.py), named by the rank of its first
               edge among the entry edges; an edge on a cycle of one-in-one-out nodes has none (NONE)
  windows      the forward (K+1)-windows of a read in order, restarting after any byte that is not one of ACGTacgt;
               never normalised, the reverse complement never looked up
  exact        a window is aligned iff it is an edge with a segment; its segment is that edge's
  carry        the reference's aligner: a window whose predecessor in the read was aligned, which is an edge, which
               leaves the node the predecessor enters, and which is the only edge to leave it, takes the predecessor's
               segment without a lookup.  The state is reset at every read (the reference never resets it)
  links        a hit is an aligned window on a unique segment.  gap counts the windows that are no hit; the first hit
               primes (b, gap = 0); a hit on b changes nothing; a hit on another segment s records (b, s, gap), then
               b = s and gap = 0.  table[(a, b)] = [records, sum of their gaps], unbounded integers
"""
NONE = 0xFFFFFFFF
MISS = 0xFFFFFFFF
NON_UNIQUE = 0x80000000

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def segments(edges, K):
    """(seg_of, starts): seg_of[i] = the entry rank of the linear path that holds edge i, or NONE; starts = the ranks
    of the entry edges in rank order"""
    node_mask = (1 << (2 * K)) - 1
    out_deg, in_deg = {}, {}
    for e in edges:
        out_deg[e >> 2] = out_deg.get(e >> 2, 0) + 1
        in_deg[e & node_mask] = in_deg.get(e & node_mask, 0) + 1
    rank = {e: i for i, e in enumerate(edges)}

    def plain(node):
        return in_deg.get(node, 0) == 1 and out_deg.get(node, 0) == 1

    starts = [i for i, e in enumerate(edges) if not plain(e >> 2)]
    seg_of = [NONE] * len(edges)
    for j, i in enumerate(starts):
        x = i
        while True:
            seg_of[x] = j
            to = edges[x] & node_mask
            if not plain(to):
                break
            nx = [rank[(to << 2) | b] for b in range(4) if ((to << 2) | b) in rank][0]
            if nx == i:
                break
            x = nx
    return seg_of, starts


def lines_of(text):
    """the reads of a batch: its lines ('\\n' alone ends a read; a '\\r' is a byte like any other)"""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    return text.split("\n")


def windows_of(read, K):
    """the valid forward (K+1)-windows of a read, as integers, in order"""
    out, run, val = [], 0, 0
    mask = (1 << (2 * (K + 1))) - 1
    for ch in read:
        c = _CODE.get(ch.upper())
        if c is None:
            run, val = 0, 0
            continue
        val = ((val << 2) | c) & mask
        run += 1
        if run >= K + 1:
            out.append(val)
    return out


class Model:
    def __init__(self, edges, K):
        self.K = K
        self.edges = list(edges)
        self.rank = {e: i for i, e in enumerate(self.edges)}
        self.seg_of, self.starts = segments(self.edges, K)
        self.entries = len(self.starts)
        self.out_deg = {}
        for e in self.edges:
            self.out_deg[e >> 2] = self.out_deg.get(e >> 2, 0) + 1

    def fresh(self, e):
        i = self.rank.get(e)
        return MISS if i is None else self.seg_of[i]

    def read_windows(self, read, carry):
        """[(segment or MISS, carried)] per window of one read"""
        node_mask = (1 << (2 * self.K)) - 1
        out = []
        valid, seg, prev = False, MISS, None
        for e in windows_of(read, self.K):
            carried = False
            if carry and valid and e in self.rank and (e >> 2) == (prev & node_mask) and self.out_deg[e >> 2] == 1:
                carried = True                         # (seg stays)
            else:
                seg = self.fresh(e)
                valid = seg != MISS
            prev = e
            out.append((seg if valid else MISS, carried))
        return out

    def thread_windows(self, text, unique=None, carry=True):
        """the answer per window of the batch, in read order: the segment, | NON_UNIQUE where it is not unique, or MISS"""
        out = []
        for read in lines_of(text):
            for seg, _ in self.read_windows(read, carry):
                if seg != MISS and unique is not None and not unique[seg]:
                    seg |= NON_UNIQUE
                out.append(seg)
        return out

    def read_links(self, batches, unique=None, carry=True):
        """(table, info): table = {(a, b): [count, gap_sum]}; info = dict(reads, windows, misses, carried, hits, records)"""
        table = {}
        info = dict(reads=0, windows=0, misses=0, carried=0, hits=0, records=0)
        for text in batches:
            if len(text) == 0:
                continue
            lines = lines_of(text)
            if lines and lines[-1] == "":
                lines.pop()                            # (the text ended in '\n': no read follows it)
            for read in lines:
                info["reads"] += 1
                primed, b, gap = False, None, 0
                ws = windows_of(read, self.K)
                for e, (seg, carried) in zip(ws, self.read_windows(read, carry)):
                    info["windows"] += 1
                    info["misses"] += e not in self.rank
                    info["carried"] += carried
                    if seg != MISS and (unique is None or unique[seg]):
                        info["hits"] += 1
                        if not primed:
                            primed, b, gap = True, seg, 0
                        elif seg != b:
                            row = table.setdefault((b, seg), [0, 0])
                            row[0] += 1
                            row[1] += gap
                            info["records"] += 1
                            b, gap = seg, 0
                    else:
                        gap += 1
        return table, info


def rows_of(table):
    """[(a, b, count, gap_sum)] ascending by (a, b)"""
    return [(a, b, c, s) for (a, b), (c, s) in sorted(table.items())]
