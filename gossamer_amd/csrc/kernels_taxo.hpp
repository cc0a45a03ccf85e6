// kernels_taxo.hpp -- a taxonomy over the k-mers of a KmerSet (goss_gpu_object_taxo_*): the two reductions behind
// annotate-kmers and classify-reads, and the small kernels around them.
//
// The host numbers the tree in pre-order and uploads parent[p], last[p] (the largest number in p's subtree) and id[p].
// Then a is an ancestor-or-equal of b iff a <= b && b <= last[a], in a chain the deeper node is the larger number, and
// lca(a, b) climbs parent[] from min(a, b) until last[x] >= max(a, b).  A class on the device is p + 1, 0 = none, so a
// zero-filled array starts right; kTaxoMany marks a read whose classes are no chain.  Node ids exist only at the two
// ends: taxo_dense_kernel turns them into classes by a binary search of the sorted id table, taxo_ids_kernel back.
//
// Both reductions are semilattice joins (associative, commutative, idempotent), done with compare-and-swap loops that
// stop without writing when the word already holds the join: the result is the same whatever the order of arrival.
//   annotate: ann[r] = lca over the classes of the reads that hold k-mer r          (taxo_lca, match_reads_kernel)
//   classify: a read's word = the deepest of its classes if they are a chain, else kTaxoMany     (taxo_combine)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels_common.hpp"

namespace goss {

constexpr uint32_t kTaxoMany = 0xFFFFFFFFu;              // device form; the ABI's GOSS_TAXO_MANY is 0xFFFFFFFE
constexpr uint32_t kTaxoIdNone = 0xFFFFFFFFu, kTaxoIdMany = 0xFFFFFFFEu;
enum : uint32_t { kTaxoAllowNone = 1, kTaxoAllowMany = 2 };

// what the two taxonomy modes of match_reads_kernel read and write
struct TaxoView {
    const uint32_t* parent = nullptr;                    // [n] pre-order number of the parent; the root's is its own
    const uint32_t* last = nullptr;                      // [n] largest pre-order number in the subtree
    uint32_t* ann = nullptr;                             // [count] class per k-mer rank
    const uint32_t* read_class = nullptr;                // annotate: class per read of the batch
    unsigned long long* unann = nullptr;                 // taxon: hits at a rank without a class
};

// lca of two classes (both not none)
__device__ __forceinline__ uint32_t taxo_lca(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ last, uint32_t a, uint32_t b)
{
    uint32_t x = (a < b ? a : b) - 1;
    const uint32_t hi = (a < b ? b : a) - 1;
    while (last[x] < hi) x = parent[x];                  // (the root's last is n - 1: the climb ends there at the latest)
    return x + 1;
}

// the deeper of two classes when one is an ancestor-or-equal of the other, else kTaxoMany; none is the identity
__device__ __forceinline__ uint32_t taxo_combine(const uint32_t* __restrict__ last, uint32_t a, uint32_t b)
{
    if (a == 0 || a == b) return b;
    if (b == 0) return a;
    if (a == kTaxoMany || b == kTaxoMany) return kTaxoMany;
    const uint32_t lo = a < b ? a : b, hi = a < b ? b : a;
    return hi - 1 <= last[lo - 1] ? hi : kTaxoMany;
}

// *w = combine(*w, c), without a write where *w already is that (LDS or global)
__device__ __forceinline__ void taxo_combine_into(uint32_t* w, const uint32_t* __restrict__ last, uint32_t c)
{
    uint32_t old = __atomic_load_n(w, __ATOMIC_RELAXED);
    for (;;)
    {
        const uint32_t nw = taxo_combine(last, old, c);
        if (nw == old) return;
        const uint32_t seen = atomicCAS(w, old, nw);
        if (seen == old) return;
        old = seen;
    }
}

// *w = *w ? lca(*w, v) : v, without a write where *w already is that: the common case, every later k-mer of a genome
// whose ancestor sits there
__device__ __forceinline__ void taxo_lca_into(uint32_t* w, const uint32_t* __restrict__ parent, const uint32_t* __restrict__ last, uint32_t v)
{
    uint32_t old = __atomic_load_n(w, __ATOMIC_RELAXED);
    for (;;)
    {
        const uint32_t nw = old ? taxo_lca(parent, last, old, v) : v;
        if (nw == old) return;
        const uint32_t seen = atomicCAS(w, old, nw);
        if (seen == old) return;
        old = seen;
    }
}

// the class of node id x by the sorted id table, 0 when the tree has no such node
__device__ __forceinline__ uint32_t taxo_find(const uint32_t* __restrict__ sorted_id, const uint32_t* __restrict__ sorted_class, uint32_t n, uint32_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted_id[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted_id[lo] == x ? sorted_class[lo] : 0;
}

__device__ __forceinline__ bool taxo_to_class(const uint32_t* __restrict__ sorted_id, const uint32_t* __restrict__ sorted_class, uint32_t n,
                                              uint32_t allow, uint32_t x, uint32_t* c)
{
    if (x == kTaxoIdNone && (allow & kTaxoAllowNone)) { *c = 0; return true; }
    if (x == kTaxoIdMany && (allow & kTaxoAllowMany)) { *c = kTaxoMany; return true; }
    *c = taxo_find(sorted_id, sorted_class, n, x);
    return *c != 0;
}

__device__ __forceinline__ uint32_t taxo_to_id(const uint32_t* __restrict__ id, uint32_t c)
{
    return c == 0 ? kTaxoIdNone : c == kTaxoMany ? kTaxoIdMany : id[c - 1];
}

// out[i] = the class of node id in[i]; allow: which of the two sentinels pass (as none / many).  An id the tree lacks
// leaves the lowest such i in bad[0].
__global__ __launch_bounds__(256) void taxo_dense_kernel(const uint32_t* __restrict__ in, uint64_t z, const uint32_t* __restrict__ sorted_id,
                                                         const uint32_t* __restrict__ sorted_class, uint32_t n, uint32_t allow,
                                                         uint32_t* __restrict__ out, unsigned long long* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < z; i += (uint64_t)gridDim.x * blockDim.x)
    {
        uint32_t c;
        if (!taxo_to_class(sorted_id, sorted_class, n, allow, in[i], &c)) { atomicMin(&bad[0], (unsigned long long)i); c = 0; }
        out[i] = c;
    }
}

// the inverse: out[i] = the node id of class in[i], none and many as the ABI's sentinels (in place is fine)
__global__ __launch_bounds__(256) void taxo_ids_kernel(const uint32_t* in, uint64_t z, const uint32_t* __restrict__ id, uint32_t* out)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < z; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = taxo_to_id(id, in[i]);
}

// bins[c - 1] += 1 for every class c of in[0..z), none into bins[n], many into bins[n + 1].  Most entries fall into a
// handful of bins (the root, a few inner nodes), so the lanes of a wave that hold the same value are matched first --
// rounds of "the first lane left names its value, the lanes that hold it leave" -- and one lane adds their number.
__global__ __launch_bounds__(256) void taxo_tally_kernel(const uint32_t* __restrict__ in, uint64_t z, uint32_t n, unsigned long long* __restrict__ bins)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < z; i0 += stride)       // (wave-uniform trip count)
    {
        const uint64_t i = i0 + lane_id();
        const bool have = i < z;
        uint32_t bin = 0;
        if (have)
        {
            const uint32_t c = in[i];
            bin = c == 0 ? n : c == kTaxoMany ? n + 1 : c - 1;
        }
        uint64_t left = __ballot(have);
        while (left)
        {
            const uint32_t lead = (uint32_t)__ffsll((long long)left) - 1;
            const uint32_t v = (uint32_t)__shfl((int)bin, (int)lead, 64);
            const uint64_t same = __ballot(have && bin == v) & left;
            if (lane_id() == lead && v < n + 2) atomicAdd(&bins[v], (unsigned long long)__popcll(same));
            left &= ~same;
        }
    }
}

// out[i] = combine(a[i], b[i]) over node ids and the two sentinels (the mates of a pair); an id the tree lacks leaves
// the lowest such i in bad[0]
__global__ __launch_bounds__(256) void taxo_pair_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint64_t z,
                                                        const uint32_t* __restrict__ sorted_id, const uint32_t* __restrict__ sorted_class,
                                                        const uint32_t* __restrict__ last, const uint32_t* __restrict__ id, uint32_t n,
                                                        uint32_t* __restrict__ out, unsigned long long* __restrict__ bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < z; i += (uint64_t)gridDim.x * blockDim.x)
    {
        uint32_t ca, cb;
        const bool oka = taxo_to_class(sorted_id, sorted_class, n, kTaxoAllowNone | kTaxoAllowMany, a[i], &ca);
        const bool okb = taxo_to_class(sorted_id, sorted_class, n, kTaxoAllowNone | kTaxoAllowMany, b[i], &cb);
        if (!oka || !okb) { atomicMin(&bad[0], (unsigned long long)i); out[i] = kTaxoIdNone; continue; }
        out[i] = taxo_to_id(id, taxo_combine(last, ca, cb));
    }
}

}  // namespace goss
