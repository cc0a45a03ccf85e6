// kernels_relative.hpp -- the two passes of the reference's `translucent` executable that need no traversal:
// trim-relative and merge-graph-with-reference, on the decoded edge list of a graph.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_subgraph.hpp.
//
// What it replaces:
//
//   trim-relative (TransCmdTrimRelative.cc:81-191).  One block of ranks per thread, each block starting at
//   beginRank(from(select(i * S))): a walk over the edges in rank order that collects the multiplicities of the
//   edges that leave one node -- they are adjacent, at most four -- and, for a node with two or more of them, culls
//   every edge whose multiplicity is below relCoverage times their sum (`pCounts[i] < thresh`, a uint32_t against a
//   double: strict), together with its reverse complement (rank(reverseComplement(select(r)))), all behind one mutex
//   for the zapped bits.  The blocks start at the first edge of a node, so no group is cut and the thread count
//   decides nothing (tests/relative_model.py keeps the loop as it stands and shows that).
//   Here one lane per edge finds its group among the ranks r - 3 .. r + 3, forms the 64-bit sum and evaluates
//   double(count) < double(sum) * rel: one conversion each, one IEEE multiplication, one comparison (the library is
//   built with -ffp-contract=off; there is nothing to contract).  The sum of four 32-bit counts is exact in a double.
//   The 64 decisions of a wave are one ballot and one store of its two bitmap words: the bitmaps are padded to whole
//   compaction tiles, so every wave owns whole words and the judge pass needs no atomic.
//   In-edges are not grouped: they are judged as the out-edges of the complementary node, so the set `below` is in
//   general not symmetric.  The mirror pass closes it: it runs over the set bits of `below` only -- a wave loads 64
//   words and its lanes share the bits of the non-zero ones, as subgraph_push_kernel does for its frontier --, forms
//   the reverse complement with revcomp() of goss_key.hpp, finds its rank with the bucket table and the bounded
//   binary search of the link pass (tips_lower_bound) and ORs that bit into `zap`, a copy of `below`.  Nothing else
//   of the link arrays is built.  `below` is only read there, so which edges are looked up, and the edge the call
//   is refused for when a reverse complement is absent (the lowest, by atomicMin), do not depend on scheduling.
//   The figures are sums of popcounts and integer atomics; what was removed only as a mirror image is the final
//   popcount less `below`, taken on the host.
//
//   merge-graph-with-reference (TransCmdMergeGraphWithReference.cc:47-114).  A two-pointer merge of two lazy
//   iterators that keeps the edges of graph-in that graph-ref holds too, each with the reference's multiplicity.
//   Here one lane per resident edge walks the reference as query_lookup_kernel does -- rd_sparse_access_rank for the
//   rank and the `present` flag, rd_vba_get for the multiplicity at that rank -- and writes the new count and, by
//   ballot, the bit "absent" of the removal bitmap.  Presence is the flag: an edge the reference holds with
//   multiplicity 0 stays, with 0.
//
// Both bitmaps feed tips_keep_count_kernel / tips_keep_write_kernel unchanged.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "kernels_query.hpp"
#include "kernels_tips.hpp"

namespace goss {

struct RelativeReport {
    unsigned long long forks;               // from-nodes with two or more out-edges
    unsigned long long below;               // edges below their own node's threshold
    unsigned long long bad;                 // ~0, or the lowest edge the pass cannot answer for: a flagged edge without
                                            // its reverse complement (mirror), a walk the reference cannot answer (recount)
};

// Judge pass: bit i of `below` = edge i leaves a node with two or more out-edges and double(count) < double(sum) * rel.
// Fixed grid, one wave per 64 ranks and step; the neighbours of a group that straddles a wave or a workgroup come from
// global memory like the edge itself.  `below` holds two 32-bit words per 64 ranks and is padded to whole tiles.
template <class K>
__global__ __launch_bounds__(kTB) void relative_judge_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ counts, uint64_t n,
                                                             double rel, uint32_t* __restrict__ below, RelativeReport* __restrict__ rep)
{
    __shared__ uint32_t sh[kWaves + 1];
    uint32_t forks = 0, culled = 0;                      // (lane 0 of every wave counts)
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; (i & ~63ULL) < n; i += (uint64_t)gridDim.x * kTB)
    {
        bool cull = false, head = false;
        if (i < n)
        {
            const K e = keys[i];
            const uint32_t c = counts[i];
            // the edges of from(e): at most four, adjacent.  (Loading both neighbours up front, before the two walks, was
            // measured 10 % slower over 1.1e8 edges: 0.82 against 0.75 ms.)
            uint64_t total = c;
            uint32_t pos = 0, size = 1;
            while (pos < 3u && i > pos && tips_same_from(keys[i - pos - 1u], e)) { total += counts[i - pos - 1u]; ++pos; }
            size += pos;
            for (uint32_t j = 1; j < 4u && size < 4u && i + j < n && tips_same_from(keys[i + j], e); ++j) { total += counts[i + j]; ++size; }
            if (size >= 2u)
            {
                head = pos == 0u;
                const double thresh = (double)total * rel;
                cull = (double)c < thresh;
            }
        }
        const uint64_t cb = __ballot(cull), hb = __ballot(head);
        if (lane_id() == 0)
        {
            const uint64_t w = (i >> 6) * 2;
            below[w] = (uint32_t)cb;
            below[w + 1] = (uint32_t)(cb >> 32);
            culled += __popcll(cb);
            forks += __popcll(hb);
        }
    }
    uint32_t tot;
    block_excl_scan<uint32_t>(forks, sh, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&rep->forks, (unsigned long long)tot);
    block_excl_scan<uint32_t>(culled, sh, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&rep->below, (unsigned long long)tot);
}

// Mirror pass: zap[rank(rc(E[e]))] |= 1 for every set bit e of `below` (read as 64-bit words; nwords of them).  Lane l
// of the wave takes bit l of each non-zero word.  An edge that is its own reverse complement, and a mirror image that
// is below its own threshold, have their bit already.
template <class K>
__global__ __launch_bounds__(kTB) void relative_mirror_kernel(const uint64_t* __restrict__ below, uint64_t nwords, const K* __restrict__ keys,
                                                              uint32_t n, uint32_t len, uint32_t bits, const uint32_t* __restrict__ table,
                                                              uint32_t* __restrict__ zap, RelativeReport* __restrict__ rep)
{
    const uint32_t lane = lane_id();
    for (uint64_t w0 = ((uint64_t)blockIdx.x * kTB + threadIdx.x) & ~63ULL; w0 < nwords; w0 += (uint64_t)gridDim.x * kTB)
    {
        const uint64_t w = w0 + lane;
        const unsigned long long mine = w < nwords ? below[w] : 0ULL;
        uint64_t todo = __ballot(mine != 0ULL);
        while (todo)
        {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const unsigned long long word = __shfl(mine, src);
            if ((word >> lane) & 1ULL)
            {
                const uint64_t e = (w0 + (uint32_t)src) * 64 + lane;          // (< n: the padding bits are zero)
                const K rc = revcomp(keys[e], len);
                const uint32_t r = tips_lower_bound(keys, n, len, bits, table, rc);
                if (r >= n || keys[r] != rc) atomicMin(&rep->bad, (unsigned long long)e);
                else if (!((below[r >> 6] >> (r & 63u)) & 1ULL)) atomicOr(&zap[r >> 5], 1u << (r & 31u));
            }
        }
    }
}

// Recount pass: counts_out[i] = the multiplicity the reference holds for edge i, bit i of `absent` = it holds none.
// Fixed grid, whole waves, two words per 64 ranks as above.  A walk the reference's index cannot answer leaves the
// lowest such rank in rep->bad.
template <class K>
__global__ __launch_bounds__(kTB) void relative_recount_kernel(QueryObj o, const K* __restrict__ keys, uint64_t n, uint32_t* __restrict__ counts_out,
                                                               uint32_t* __restrict__ absent, RelativeReport* __restrict__ rep)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; (i & ~63ULL) < n; i += (uint64_t)gridDim.x * kTB)
    {
        bool gone = false;
        if (i < n)
        {
            const K x = keys[i];
            uint64_t r = 0;
            uint32_t c = 0;
            bool p = false;
            if (!rd_sparse_access_rank<K>(o.s, x, &r, &p) || (p && !rd_vba_get(o.v, r, &c))) atomicMin(&rep->bad, (unsigned long long)i);
            counts_out[i] = c;
            gone = !p;
        }
        const uint64_t gb = __ballot(gone);
        if (lane_id() == 0)
        {
            const uint64_t w = (i >> 6) * 2;
            absent[w] = (uint32_t)gb;
            absent[w + 1] = (uint32_t)(gb >> 32);
        }
    }
}

}  // namespace goss
