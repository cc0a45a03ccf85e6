// kernels_query.hpp -- batched queries against one KmerSet / Graph / SparseArray resident in HBM
// (goss_gpu_object_*): rank / presence, select, multiplicity, the fused lookup and a node's edge range; for an
// EntryEdgeSet also a path's length and the entry of its mirror path.
// One lane per query, grid-stride; no LDS.  A query is a chain of dependent global loads through the
// structure (d0 rank + index arrays, the sample, high-bits words, the low-bits columns of a group of one
// or two elements, and for a graph's count ord0 plus two more rank walks over ord1p / ord2p): latency,
// not bandwidth, bounds it ("Queries").
//
// A query that the object cannot answer -- a key outside the universe, a rank at or past the count, an
// index walk that runs into a damaged image -- writes nothing; the lowest such query index, with its
// reason in the low two bits, is kept in *bad (atomicMin) and the entry point fails naming it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "goss_reader.hpp"

namespace goss {

enum : uint32_t { kQueryNormalize = 1, kQueryIncoming = 2 };
enum : uint64_t { kQBadKey = 1, kQBadRank = 2, kQBadWalk = 3 };

// VariableByteArray (VariableByteArray.hh:120-247): byte 0 of every value in ord0; bits 8..15 of the
// values that ord1p lists in ord1; bits 16..31 of the ord1 entries that ord2p lists in ord2
struct RdVba {
    const uint8_t* ord0;
    const uint8_t* ord1;
    const uint16_t* ord2;
    RdSparse p1, p2;
};

struct QueryObj {
    RdSparse s;                 // the k-mers, the edges or the bare array
    RdVba v;                    // graph: the multiplicities
    uint32_t len;               // bases per key: K (k-mer set), K + 1 (graph edges); 0 = bare array
    uint32_t graph;
};

__device__ inline void q_fail(unsigned long long* bad, uint64_t i, uint64_t why) { atomicMin(bad, (unsigned long long)((i << 2) | why)); }

// VariableByteArray::operator[] (VariableByteArray.hh:227-247)
__device__ inline bool rd_vba_get(const RdVba& v, uint64_t i, uint32_t* out)
{
    uint32_t r = v.ord0[i];
    uint64_t r1, r2;
    bool p;
    if (!rd_sparse_access_rank<Key1>(v.p1, Key1{i}, &r1, &p)) return false;
    if (p)
    {
        r |= (uint32_t)v.ord1[r1] << 8;
        if (!rd_sparse_access_rank<Key1>(v.p2, Key1{r1}, &r2, &p)) return false;
        if (p) r |= (uint32_t)v.ord2[r2] << 16;
    }
    *out = r;
    return true;
}

// a caller's key: inside the universe, then (kQueryNormalize) its canonical form,
// position_type::normalize (RankSelect.hh:126-140)
template <class K>
__device__ inline bool q_key(const QueryObj& o, K& x, uint32_t flags)
{
    if (!rd_below(x, o.s.size_lo, o.s.size_hi)) return false;
    if (flags & kQueryNormalize) x = canonical(x, revcomp(x, o.len));
    return true;
}

// SparseArray::accessAndRank / rank (SparseArray.hh:262-309)
template <class K>
__global__ __launch_bounds__(256) void query_rank_kernel(QueryObj o, const K* __restrict__ keys, uint64_t n, uint32_t flags,
                                                         uint64_t* __restrict__ rank, uint8_t* __restrict__ present,
                                                         unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        K x = keys[i];
        if (!q_key(o, x, flags)) { q_fail(bad, i, kQBadKey); continue; }
        uint64_t r;
        bool p;
        if (!rd_sparse_access_rank<K>(o.s, x, &r, &p)) { q_fail(bad, i, kQBadWalk); continue; }
        if (rank) rank[i] = r;
        if (present) present[i] = p ? 1 : 0;
    }
}

// SparseArray::select (SparseArray.hh:311-325)
template <class K>
__global__ __launch_bounds__(256) void query_select_kernel(QueryObj o, const uint64_t* __restrict__ ranks, uint64_t n,
                                                           K* __restrict__ out, unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t r = ranks[i];
        if (r >= o.s.count) { q_fail(bad, i, kQBadRank); continue; }
        K x;
        if (!rd_sparse_select<K>(o.s, r, &x)) { q_fail(bad, i, kQBadWalk); continue; }
        out[i] = x;
    }
}

// Graph::multiplicity(rank) (Graph.hh:425-428); an opened graph has no removed edges, so
// SparseArrayView::originalRank is the identity
__global__ __launch_bounds__(256) void query_multiplicity_kernel(QueryObj o, const uint64_t* __restrict__ ranks, uint64_t n,
                                                                 uint32_t* __restrict__ out, unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t r = ranks[i];
        if (r >= o.s.count) { q_fail(bad, i, kQBadRank); continue; }
        uint32_t c;
        if (!rd_vba_get(o.v, r, &c)) { q_fail(bad, i, kQBadWalk); continue; }
        out[i] = c;
    }
}

// the fused hot path: accessAndRank, then (graph) multiplicity of that rank -- the count of each key, 0 when absent
// (Graph::multiplicity(const Edge&), Graph.hh:416-419; 1 / 0 for a k-mer set or a bare array)
template <class K>
__global__ __launch_bounds__(256) void query_lookup_kernel(QueryObj o, const K* __restrict__ keys, uint64_t n, uint32_t flags,
                                                           uint32_t* __restrict__ out, unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        K x = keys[i];
        if (!q_key(o, x, flags)) { q_fail(bad, i, kQBadKey); continue; }
        uint64_t r;
        bool p;
        if (!rd_sparse_access_rank<K>(o.s, x, &r, &p)) { q_fail(bad, i, kQBadWalk); continue; }
        uint32_t c = p ? 1u : 0u;
        if (p && o.graph && !rd_vba_get(o.v, r, &c)) { q_fail(bad, i, kQBadWalk); continue; }
        out[i] = c;
    }
}

// What an EntryEdgeSet holds beside its edges and counts (EntryEdgeSet.hh:100-125): the paths' lengths and, as the
// two columns of a 40-bit IntegerArray, the entry at which each path's mirror image starts.
struct QueryEntries {
    RdVba lengths;
    const uint8_t* ends_upr;
    const uint32_t* ends_lwr;
    uint64_t count;
};

// EntryEdgeSet::length(rank) (EntryEdgeSet.hh:113-118)
__global__ __launch_bounds__(256) void query_length_kernel(QueryEntries e, const uint64_t* __restrict__ ranks, uint64_t n,
                                                           uint32_t* __restrict__ out, unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t r = ranks[i];
        if (r >= e.count) { q_fail(bad, i, kQBadRank); continue; }
        uint32_t l;
        if (!rd_vba_get(e.lengths, r, &l)) { q_fail(bad, i, kQBadWalk); continue; }
        out[i] = l;
    }
}

// EntryEdgeSet::endRank(rank) (EntryEdgeSet.hh:120-125)
__global__ __launch_bounds__(256) void query_end_rank_kernel(QueryEntries e, const uint64_t* __restrict__ ranks, uint64_t n,
                                                             uint64_t* __restrict__ out, unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        const uint64_t r = ranks[i];
        if (r >= e.count) { q_fail(bad, i, kQBadRank); continue; }
        out[i] = ((uint64_t)e.ends_upr[r] << 32) | e.ends_lwr[r];
    }
}

__device__ inline Key2 q_wide(const Key1& k) { return Key2{k.lo, 0}; }
__device__ inline Key2 q_wide(const Key2& k) { return k; }
template <class K> __device__ inline K q_narrow(const Key2& k);
template <> __device__ inline Key1 q_narrow<Key1>(const Key2& k) { return Key1{k.lo}; }
template <> __device__ inline Key2 q_narrow<Key2>(const Key2& k) { return k; }

// GraphEssentials::beginEndRank (GraphEssentials.hh:88-96): the ranks of edges node.A and node.T + 1, i.e. of
// (node << 2) and (node << 2) + 4; out-degree = end - begin.  kQueryIncoming: the same for the node's reverse
// complement (inDegree, GraphEssentials.hh:74-77).  For the all-T node, (node << 2) + 4 is the edge universe
// 4^(K+1) itself: rank answers the count there without walking the index (SparseArray.hh:298-301).
// KN: the node's key layout (K bases), KE: the edges' (K + 1 bases) -- they differ for K = 31.
template <class KN, class KE>
__global__ __launch_bounds__(256) void query_node_ranks_kernel(QueryObj o, const KN* __restrict__ nodes, uint64_t n, uint32_t flags,
                                                               uint64_t* __restrict__ begin, uint64_t* __restrict__ end,
                                                               unsigned long long* bad)
{
    const uint32_t K = o.len - 1;
    const uint64_t nlo = 2 * K < 64 ? (1ULL << (2 * K)) : 0, nhi = 2 * K >= 64 ? (1ULL << (2 * K - 64)) : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    {
        KN x = nodes[i];
        if (!rd_below(x, nlo, nhi)) { q_fail(bad, i, kQBadKey); continue; }
        if (flags & kQueryNormalize) x = canonical(x, revcomp(x, K));
        if (flags & kQueryIncoming) x = revcomp(x, K);
        const Key2 w = q_wide(x);
        const Key2 e0{w.lo << 2, (w.hi << 2) | (w.lo >> 62)};
        const Key2 e1{e0.lo + 4, e0.hi + (e0.lo + 4 < e0.lo ? 1 : 0)};
        uint64_t b, e;
        bool p;
        if (!rd_sparse_access_rank<KE>(o.s, q_narrow<KE>(e0), &b, &p) || !rd_sparse_access_rank<KE>(o.s, q_narrow<KE>(e1), &e, &p))
        {
            q_fail(bad, i, kQBadWalk);
            continue;
        }
        if (begin) begin[i] = b;
        if (end) end[i] = e;
    }
}

}  // namespace goss
