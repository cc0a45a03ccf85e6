// kernels_subgraph.hpp -- build-subgraph on the decoded edge list of a graph: the marks of reads grown by a radius.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_components.hpp.
//
// What it replaces: GossCmdBuildSubgraph.cc:95-212 -- `radius` serial passes, each a scan over a dynamic_bitset of all
// edges whose every step is a rank / select walk of the Elias-Fano index.  With the link pass of kernels_tips.hpp
// (rcr, nxt, info) the neighbours of an edge are array arithmetic:
//
//   the edges that leave to(e)      [nxt[e], nxt[e] + out(to(e)))
//   the edges that enter from(e)    rcr[j] for j in [nxt[r], nxt[r] + out(to(r))), r = rcr[e]     (in(from e) = out(to(rc e)))
//
// What the reference computes (the graph is symmetric, or the command refuses, :141-146):
//
//   Marks (:178-191).  Every (K+1)-window of every read -- GossRead::Iterator(read, K + 1), the window rules of
//   components_mark_kernel -- and its reverse complement (ReverseComplementAdapter) is looked up.  The start set I is
//   therefore the forward marks and their mirror image: I[rcr[i]] |= I[i]  (subgraph_mirror_kernel).  Without a single
//   read the command fails with "No valid reads." (ReverseComplementAdapter.hh:77-86); reads that hit nothing give the
//   empty graph.
//
//   Node mode (SingleFollower, :56-72, the default).  P = I; `radius` times (:100-127): F = the edges not in I that
//   leave to(e) or enter from(e) for some e in P -- the siblings of e, the other edges out of from(e) and into to(e),
//   do not count -- then I |= F, P = F, and "pass <i> identified <|F|> additional edges." is logged, i from 0.  P is
//   symmetric, so the mirror images the reference sets explicitly (:66-69) are in F already.
//
//   Linear-path mode (SegmentFollower, :74-92, --linear-paths).  A segment is a maximal set of edges joined through
//   nodes with exactly one edge in and one out (Graph::linearPath forwards from e, Graph.tcc:19-46, together with the
//   walk forwards from rc(e)); a cycle whose nodes are all of that kind is one segment (the `ee == pBegin` break).
//   Per pass every segment that holds an edge of P, and its mirror segment, goes into I whole; F = the edges still
//   outside I that have a predecessor or a successor in such a segment (necessarily its last or first edge);
//   I |= F, P = F.  The logged number is the growth of I over the pass, the covered segments included.  The edges the
//   last pass adds stay single edges.  The reference writes fringe[k] = !interesting[k] as an assignment while
//   `interesting` changes within the pass (:65, :85-88), so ITS next `prev` depends on the scan order; I after every
//   pass does not: an edge that is in or out of `prev` by order lies on a path the same pass covered, and walks a
//   sub-path of it to the same two ends in the next one.  tests/test_subgraph_cpu.py pins that to the loop as it stands.
//
//   Radius 0 in either mode gives the mirrored marks only.  Output (:201-209): Graph::Builder(K, out, fac, |I|), the
//   edges of I in rank order with their multiplicities -- the keep compaction of kernels_tips.hpp over ~I.
//
// A pass is sparse: the frontier P is a bitmap that the push kernels read a word at a time (a zero word costs one
// load), the 64 lanes of a wave share the bits of a non-zero word, and everything is OR-ed with 32-bit vector atomics
// into a zeroed fringe that one settle launch folds into I.  Nothing depends on the order in which lanes run.
// The segments are the classes of a lock-free union-find (comp_find / comp_union of kernels_components.hpp) in which
// an edge hooks itself to its single successor: a cycle without a start is a class like any other.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hpp"
#include "kernels_tips.hpp"
#include "kernels_components.hpp"

namespace goss {

__device__ __forceinline__ bool subgraph_bit(const uint32_t* words, uint32_t i) { return (words[i >> 5] >> (i & 31u)) & 1u; }
__device__ __forceinline__ void subgraph_set(uint32_t* words, uint32_t i) { atomicOr(&words[i >> 5], 1u << (i & 31u)); }

// I[rcr[i]] |= I[i]: one lane per edge.  A bit another lane has just set is mirrored onto a bit that is set already.
__global__ __launch_bounds__(kTB) void subgraph_mirror_kernel(const uint32_t* __restrict__ rcr, uint32_t n, uint32_t* marks)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (!subgraph_bit(marks, i)) return;
    const uint32_t r = rcr[i];
    if (!subgraph_bit(marks, r)) subgraph_set(marks, r);
}

// Node mode, one pass: every edge e of the frontier P ORs into the fringe the edges that leave to(e) and the edges
// that enter from(e), those in I already left out.  Fixed grid; a wave loads 64 words of P per step and takes its
// non-zero words one after the other: lanes 0-31 take bit `lane` forwards, lanes 32-63 the same bit backwards.
__global__ __launch_bounds__(kTB) void subgraph_push_kernel(const uint32_t* __restrict__ P, uint64_t nwords,
                                                            const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                            const uint8_t* __restrict__ info, const uint32_t* __restrict__ I,
                                                            uint32_t* __restrict__ fringe)
{
    const uint32_t lane = lane_id();
    const uint32_t bit = lane & 31u;
    const bool back = lane >= 32u;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * kTB + threadIdx.x) & ~63ULL; w0 < nwords; w0 += (uint64_t)gridDim.x * kTB)
    {
        const uint64_t w = w0 + lane;
        const uint32_t mine = w < nwords ? P[w] : 0u;
        uint64_t todo = __ballot(mine != 0u);
        while (todo)
        {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t word = __shfl(mine, src);
            if ((word >> bit) & 1u)
            {
                const uint32_t e = (uint32_t)((w0 + (uint32_t)src) * 32u) + bit;
                const uint32_t a = back ? rcr[e] : e;
                const uint32_t g0 = nxt[a], gn = tips_out_to(info[a]);
                for (uint32_t j = 0; j < gn; ++j)
                {
                    const uint32_t t = back ? rcr[g0 + j] : g0 + j;
                    if (!subgraph_bit(I, t)) subgraph_set(fringe, t);
                }
            }
        }
    }
}

// The end of a pass, per word: f = fringe & ~I; I |= f; P = f; fringe = 0.  *added += the bits of f, or with TOTAL the
// bits of I (linear-path mode, where the pass has grown I by whole segments before: the host takes differences),
// summed over the wave's stride before one atomic.  The padding bits beyond the last edge are never set in the
// fringe, so they stay zero in I and P.
template <bool TOTAL>
__global__ __launch_bounds__(kTB) void subgraph_settle_kernel(uint32_t* __restrict__ I, uint32_t* __restrict__ P, uint32_t* __restrict__ fringe,
                                                              uint64_t nwords, unsigned long long* __restrict__ added)
{
    uint32_t c = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kTB + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t fr = fringe[w];
        uint32_t f = 0, i = 0;
        if (fr || TOTAL) i = I[w];
        if (fr)
        {
            f = fr & ~i;
            if (f) I[w] = i | f;
            fringe[w] = 0;
        }
        P[w] = f;
        c += __popc(TOTAL ? i | f : f);
    }
    c = tips_wave_sum(c);
    if (lane_id() == 0 && c) atomicAdd(added, (unsigned long long)c);
}

// Segment labels: after components_init_kernel (every edge its own root) an edge hooks itself to its single successor
// when to(i) has one edge out and one in; components_flatten_kernel then leaves label[i] = the smallest rank on the
// segment of i.
__global__ __launch_bounds__(kTB) void subgraph_hook_kernel(const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                            const uint8_t* __restrict__ info, uint32_t n, uint32_t* __restrict__ parent)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (tips_out_to(info[i]) != 1u || tips_group_size(info[rcr[i]]) != 1u) return;
    const uint32_t s = nxt[i];
    if (s != i) comp_union(parent, i, s);
}

// Linear-path mode, first launch of a pass: hit[label[e]] = hit[label[rcr[e]]] = 1 for every edge e of P.  The words
// of P are shared as in subgraph_push_kernel: lanes 0-31 take the edge, lanes 32-63 its reverse complement.
__global__ __launch_bounds__(kTB) void subgraph_hit_kernel(const uint32_t* __restrict__ P, uint64_t nwords, const uint32_t* __restrict__ rcr,
                                                           const uint32_t* __restrict__ label, uint8_t* __restrict__ hit)
{
    const uint32_t lane = lane_id();
    const uint32_t bit = lane & 31u;
    const bool back = lane >= 32u;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * kTB + threadIdx.x) & ~63ULL; w0 < nwords; w0 += (uint64_t)gridDim.x * kTB)
    {
        const uint64_t w = w0 + lane;
        const uint32_t mine = w < nwords ? P[w] : 0u;
        uint64_t todo = __ballot(mine != 0u);
        while (todo)
        {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint32_t word = __shfl(mine, src);
            if ((word >> bit) & 1u)
            {
                const uint32_t e = (uint32_t)((w0 + (uint32_t)src) * 32u) + bit;
                hit[label[back ? rcr[e] : e]] = 1;
            }
        }
    }
}

// Linear-path mode, second launch of a pass: one lane per edge, a wave ballots its 64 results into two words of I and
// two of the fringe, no atomics.  Edge k joins I when its segment is hit; else it joins the fringe when one of its up
// to four successors or four predecessors lies on a hit segment.  An edge in I already has nothing to do: its segment
// was hit whole, or it is a single edge of the last fringe, which this pass's hits cover.  `hit` is never cleared: the
// neighbours of a segment hit earlier joined I in that pass.
__global__ __launch_bounds__(kTB) void subgraph_cover_kernel(const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                             const uint8_t* __restrict__ info, const uint32_t* __restrict__ label,
                                                             const uint8_t* __restrict__ hit, uint32_t n, uint32_t* __restrict__ I,
                                                             uint32_t* __restrict__ fringe)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if ((i64 & ~63ULL) >= n) return;                     // (whole waves)
    const uint32_t lane = lane_id();
    const uint64_t w = (i64 >> 6) * 2;                   // the two words of this wave's 64 edges
    const uint64_t old = (uint64_t)I[w] | ((uint64_t)I[w + 1] << 32);
    bool cover = false, edge = false;
    if (i64 < n && !((old >> lane) & 1ULL))
    {
        const uint32_t k = (uint32_t)i64;
        cover = hit[label[k]] != 0;
        if (!cover)
        {
            const uint32_t g0 = nxt[k], gn = tips_out_to(info[k]);
            for (uint32_t j = 0; j < gn && !edge; ++j) edge = hit[label[g0 + j]] != 0;
            if (!edge)
            {
                const uint32_t r = rcr[k];
                const uint32_t h0 = nxt[r], hn = tips_out_to(info[r]);
                for (uint32_t j = 0; j < hn && !edge; ++j) edge = hit[label[rcr[h0 + j]]] != 0;
            }
        }
    }
    const uint64_t cb = __ballot(cover), eb = __ballot(edge);
    if (lane == 0)
    {
        if (cb)
        {
            const uint64_t now = old | cb;
            I[w] = (uint32_t)now;
            I[w + 1] = (uint32_t)(now >> 32);
        }
        if (eb)
        {
            fringe[w] = (uint32_t)eb;
            fringe[w + 1] = (uint32_t)(eb >> 32);
        }
    }
}

// Removal bitmap for tips_keep_count_kernel / tips_keep_write_kernel: bit i = edge i is not marked.  zap is padded to
// whole tiles (zap_words >= mark_words): the bits beyond the last edge are zero.
__global__ __launch_bounds__(kTB) void subgraph_zap_kernel(const uint32_t* __restrict__ marks, uint64_t mark_words, uint64_t n,
                                                           uint32_t* __restrict__ zap, uint64_t zap_words)
{
    const uint64_t w = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (w >= zap_words) return;
    uint32_t v = 0;
    if (w < mark_words && w * 32 < n)
    {
        v = ~marks[w];
        const uint64_t left = n - w * 32;
        if (left < 32) v &= (1u << left) - 1u;
    }
    zap[w] = v;
}

}  // namespace goss
