// kernels_components.hpp -- count-components on the decoded edge list of a graph: the connected components of the
// marked edges, their figures, and the removal bitmap that keeps one component.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp.
//
// What it replaces: GossCmdCountComponents.cc:37-127, 171-311 -- a serial flood fill (one stack, one dynamic_bitset)
// whose every step is a rank / select walk of the Elias-Fano index.  Two marked edges belong together when they share
// a node in any role; with the link pass of kernels_tips.hpp (rcr, nxt, info) the edges that share a node with edge i
// are array arithmetic:
//
//   from(i)           the group [i - pos, i - pos + size)
//   to(i), entering   rcr[j'] for j' in the group of rcr[i]          (in(to(i)) = out(from(rc i)))
//   to(i), leaving    [nxt[i], nxt[i] + out(to(i)))
//
// Sharing a node is transitive among the edges of that node, so an edge hooks itself to the FIRST marked edge of each
// of the three sets and no more: every other member does the same, and the edges that enter from(i) see i in their
// third set.  The labelling is lock-free union-find (the ECL-CC scheme): parent[i] <= i always, a hook puts the larger
// of two roots under the smaller with one compare-and-swap, finds halve the path they climb.  Three launches over the
// edges whatever the graph's diameter; the root of a tree is its smallest rank -- the reference's `start` -- and the
// outcome is the same partition under any schedule.
//
// The figures are integer atomics on the component's record, so they do not depend on the order either.  The usual
// graph is one giant component, or a giant pair, and many small ones: a wave peels off the two labels its lowest lanes
// carry, reduces their lanes with shuffles and carries the sums along its stride; what is left goes lane by lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "goss_read_tile.hpp"
#include "kernels_tips.hpp"

namespace goss {

constexpr uint32_t kCompNone = 0xFFFFFFFFu;              // the label of an unmarked edge
constexpr uint32_t kCompPeel = 2;                        // labels a wave reduces with shuffles and carries along its stride

// goss_gpu_component (goss_gpu.h)
struct CompRec {
    unsigned long long s, s2, edges;
    uint32_t start, min, max, mirror;
};
static_assert(sizeof(CompRec) == 40, "component layout");

struct CompReport {
    unsigned long long windows, hits, marked, largest;
};

// bit i of the marks, or every edge when there are none
__device__ __forceinline__ bool comp_marked(const uint32_t* __restrict__ marks, uint32_t i)
{
    return !marks || ((marks[i >> 5] >> (i & 31u)) & 1u);
}

// ---- marking the edges that reads touch ----------------------------------------------------------------------------

// One workgroup per tile of kMatchTile byte positions, staged by goss_read_tile.hpp without the newline flags (2-bit
// codes and non-base flags in LDS bit arrays, a halo of 64 positions).  Every valid forward window of L = K + 1 bases is
// looked up among the sorted edges -- the forward key only: no reverse complement, no normalisation
// (GossCmdCountComponents.cc:231-239) -- and a hit sets the edge's bit.  rep->windows / hits: once per wave.
template <class K>
__global__ __launch_bounds__(kTB) void components_mark_kernel(const K* __restrict__ keys, uint32_t n, uint32_t L, uint32_t bits,
                                                              const uint32_t* __restrict__ table, const uint8_t* __restrict__ bases,
                                                              uint64_t nbytes, uint64_t ntiles, uint32_t aligned,
                                                              uint32_t* __restrict__ marks, CompReport* __restrict__ rep)
{
    __shared__ uint64_t s_codes[kMatchGroups / 4];       // 32 bases per word, first base lowest
    __shared__ uint64_t s_inv[kMatchGroups / 8];         // bit = not one of ACGTacgt (or beyond the input)

    const uint64_t tile = unit_block();
    if (tile >= ntiles) return;
    const uint64_t t0 = tile * kMatchTile;
    const uint32_t lane = lane_id();

    tile_stage<false>(bases, nbytes, t0, aligned, s_codes, s_inv, nullptr);
    __syncthreads();

    const uint64_t lmask = (1ULL << L) - 1;              // (L <= 63)
    uint32_t nwin = 0, nhit = 0;                         // (lane 0 counts)
    for (uint32_t it = 0; it < kMatchRuns / kWaves; ++it)
    {
        const uint32_t run = wave_id() * (kMatchRuns / kWaves) + it;
        const bool valid = tile_window_valid(s_inv, run, lane, lmask);
        const uint64_t vb = __ballot(valid);
        if (!vb) continue;
        bool hit = false;
        if (valid)
        {
            K x, rc;
            tile_window_keys<K>(s_codes, run * 64 + lane, L, &x, &rc);
            const uint32_t r = tips_lower_bound(keys, n, L, bits, table, x);
            if (r < n && keys[r] == x)
            {
                hit = true;
                atomicOr(&marks[r >> 5], 1u << (r & 31u));
            }
        }
        const uint64_t hb = __ballot(hit);
        nwin += (uint32_t)__popcll(vb);
        nhit += (uint32_t)__popcll(hb);
    }
    if (lane == 0)
    {
        if (nwin) atomicAdd(&rep->windows, (unsigned long long)nwin);
        if (nhit) atomicAdd(&rep->hits, (unsigned long long)nhit);
    }
}

// rep->marked += the bits set in words[0, nwords)
__global__ __launch_bounds__(kTB) void components_popcount_kernel(const uint32_t* __restrict__ words, uint64_t nwords,
                                                                  CompReport* __restrict__ rep)
{
    uint32_t c = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * kTB + threadIdx.x; w < nwords; w += (uint64_t)gridDim.x * kTB) c += __popc(words[w]);
    c = tips_wave_sum(c);
    if (lane_id() == 0 && c) atomicAdd(&rep->marked, (unsigned long long)c);
}

// ---- labelling -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t comp_load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The root of x's tree, halving the path on the way.  A concurrent hook or halving only ever replaces a parent by an
// ancestor, so whatever is read is an ancestor of x and the climb ends at a root of that moment.
__device__ __forceinline__ uint32_t comp_find(uint32_t* __restrict__ parent, uint32_t x)
{
    uint32_t cur = comp_load(&parent[x]);
    if (cur != x)
    {
        uint32_t prev = x, next;
        while (cur > (next = comp_load(&parent[cur])))
        {
            __atomic_store_n(&parent[prev], next, __ATOMIC_RELAXED);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// The trees of a and b become one: the larger root goes under the smaller.  A compare-and-swap that finds its root
// already hooked goes on from the parent it found there.
__device__ __forceinline__ void comp_union(uint32_t* __restrict__ parent, uint32_t a, uint32_t b)
{
    uint32_t u = comp_find(parent, a), v = comp_find(parent, b);
    while (u != v)
    {
        if (u < v) { const uint32_t t = u; u = v; v = t; }               // u: the larger
        const uint32_t seen = atomicCAS(&parent[u], u, v);
        if (seen == u) return;
        u = seen;
    }
}

__global__ __launch_bounds__(kTB) void components_init_kernel(const uint32_t* __restrict__ marks, uint32_t n, uint32_t* __restrict__ parent)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) parent[i] = comp_marked(marks, (uint32_t)i) ? (uint32_t)i : kCompNone;
}

__global__ __launch_bounds__(kTB) void components_hook_kernel(const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                              const uint8_t* __restrict__ info, const uint32_t* __restrict__ marks,
                                                              uint32_t n, uint32_t* __restrict__ parent)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    if (!comp_marked(marks, i)) return;
    const uint8_t fi = info[i];
    // the edges that leave from(i)
    {
        const uint32_t g0 = i - tips_group_pos(fi), gn = tips_group_size(fi);
        for (uint32_t j = 0; j < gn; ++j)
            if (comp_marked(marks, g0 + j))
            {
                if (g0 + j != i) comp_union(parent, i, g0 + j);
                break;
            }
    }
    // the edges that enter to(i): the reverse complements of the edges that leave rc(to(i)) = from(rc(i))
    {
        const uint32_t r = rcr[i];
        const uint8_t ri = info[r];
        const uint32_t g0 = r - tips_group_pos(ri), gn = tips_group_size(ri);
        for (uint32_t j = 0; j < gn; ++j)
        {
            const uint32_t e = rcr[g0 + j];
            if (comp_marked(marks, e))
            {
                if (e != i) comp_union(parent, i, e);
                break;
            }
        }
    }
    // the edges that leave to(i)
    {
        const uint32_t g0 = nxt[i], gn = tips_out_to(fi);
        for (uint32_t j = 0; j < gn; ++j)
            if (comp_marked(marks, g0 + j))
            {
                if (g0 + j != i) comp_union(parent, i, g0 + j);
                break;
            }
    }
}

// parent[i] = the root of i's tree.  sc, when given: sc[i] = 1 for a root, for the scan that numbers the components.
__global__ __launch_bounds__(kTB) void components_flatten_kernel(uint32_t* __restrict__ parent, uint32_t n, uint64_t* __restrict__ sc)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    uint32_t p = comp_load(&parent[i]);
    if (p != kCompNone)
    {
        uint32_t q;
        while ((q = comp_load(&parent[p])) != p) p = q;
        __atomic_store_n(&parent[i], p, __ATOMIC_RELAXED);
    }
    if (sc) sc[i] = p == i ? 1 : 0;
}

// ---- numbering and figures ---------------------------------------------------------------------------------------------

// label[i] = the index of i's component (roots below its root), kCompNone where unmarked; every root opens its record.
__global__ __launch_bounds__(kTB) void components_number_kernel(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ sc,
                                                                const uint32_t* __restrict__ rcr, uint32_t n,
                                                                uint32_t* __restrict__ label, CompRec* __restrict__ recs)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const uint32_t p = parent[i];
    if (p == kCompNone) { label[i] = kCompNone; return; }
    const uint32_t ci = (uint32_t)sc[p];
    label[i] = ci;
    if (p != i) return;
    const uint32_t pm = parent[rcr[i]];
    CompRec r;
    r.s = r.s2 = r.edges = 0;
    r.start = i; r.min = 0xFFFFFFFFu; r.max = 0;
    r.mirror = pm == kCompNone ? kCompNone : (uint32_t)sc[pm];
    recs[ci] = r;
}

__device__ __forceinline__ unsigned long long comp_wave_sum64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__device__ __forceinline__ void comp_add(CompRec* __restrict__ r, unsigned long long e, unsigned long long s, unsigned long long s2,
                                         uint32_t lo, uint32_t hi)
{
    atomicAdd(&r->edges, e);
    atomicAdd(&r->s, s);
    atomicAdd(&r->s2, s2);
    atomicMin(&r->min, lo);
    atomicMax(&r->max, hi);
}

// The sums of one label that a wave carries from one step of its stride to the next (every lane holds the same).
struct CompAcc {
    uint32_t label, lo, hi;
    unsigned long long edges, s, s2;
};

__device__ __forceinline__ void comp_flush(CompRec* __restrict__ recs, CompAcc& a)
{
    if (a.label != kCompNone && lane_id() == 0) comp_add(&recs[a.label], a.edges, a.s, a.s2, a.lo, a.hi);
    a.label = kCompNone; a.lo = 0xFFFFFFFFu; a.hi = 0; a.edges = a.s = a.s2 = 0;
}

// Fixed grid, every wave strides over the edges.  Per step the wave peels off the labels of its two lowest lanes
// (one ballot of the lanes that agree, shuffles for the five figures) and adds them to the two labels it carries;
// a label it does not carry takes the place of the one with fewer edges so far, which goes to its record with one
// atomic per figure.  The giant components of the usual graph are therefore added once per wave of the grid, not once
// per 64 edges: 1.1e8 edges in one component were 1.7e6 x 5 atomics on one record, 102 of the build's 117 ms.  The
// lanes left after the two rounds add for themselves.
__global__ __launch_bounds__(kTB) void components_figures_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ counts,
                                                                 uint32_t n, CompRec* __restrict__ recs)
{
    const uint32_t lane = lane_id();
    CompAcc acc[kCompPeel];
#pragma unroll
    for (uint32_t k = 0; k < kCompPeel; ++k) { acc[k].label = kCompNone; comp_flush(recs, acc[k]); }
    static_assert(kCompPeel == 2, "the choice of the slot below");
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; (i & ~63ULL) < n; i += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t ci = i < n ? label[i] : kCompNone;
        const uint32_t m = ci != kCompNone ? counts[i] : 0;
        uint64_t left = __ballot(ci != kCompNone);
        int used = -1;
        for (uint32_t round = 0; round < kCompPeel && left; ++round)
        {
            const int lead = __ffsll((unsigned long long)left) - 1;
            const uint32_t c = __shfl(ci, lead);
            const bool mine = ci == c;                               // (c is a real label: unmarked lanes never match)
            const uint64_t grp = __ballot(mine);
            left &= ~grp;
            const unsigned long long s = comp_wave_sum64(mine ? m : 0);
            const unsigned long long s2 = comp_wave_sum64(mine ? (unsigned long long)m * m : 0);
            uint32_t lo = mine ? m : 0xFFFFFFFFu, hi = mine ? m : 0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1)
            {
                const uint32_t ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
                lo = ol < lo ? ol : lo;
                hi = oh > hi ? oh : hi;
            }
            int k = acc[0].label == c ? 0 : acc[1].label == c ? 1 : -1;
            if (k < 0)
            {
                k = used >= 0 ? 1 - used : acc[0].edges <= acc[1].edges ? 0 : 1;
                if (k == 0) comp_flush(recs, acc[0]); else comp_flush(recs, acc[1]);
            }
            CompAcc& a = k == 0 ? acc[0] : acc[1];
            a.label = c;
            a.edges += (unsigned long long)__popcll(grp);
            a.s += s;
            a.s2 += s2;
            a.lo = lo < a.lo ? lo : a.lo;
            a.hi = hi > a.hi ? hi : a.hi;
            used = k;
        }
        if ((left >> lane) & 1ULL) comp_add(&recs[ci], 1, m, (unsigned long long)m * m, m, m);
    }
    comp_flush(recs, acc[0]);
    comp_flush(recs, acc[1]);
}

// rep->largest = the most edges a component has
__global__ __launch_bounds__(kTB) void components_largest_kernel(const CompRec* __restrict__ recs, uint64_t ncomp, CompReport* __restrict__ rep)
{
    unsigned long long v = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; i < ncomp; i += (uint64_t)gridDim.x * kTB)
        v = recs[i].edges > v ? recs[i].edges : v;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
    {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if (lane_id() == 0 && v) atomicMax(&rep->largest, v);
}

// ---- keeping one component ---------------------------------------------------------------------------------------------

// Removal bitmap for tips_keep_count_kernel / tips_keep_write_kernel: bit j = edge j lies neither in the component of
// edge e nor in that of rc(e).  parent is flattened; the bitmap is padded to whole tiles with zero bits by the caller.
__global__ __launch_bounds__(kTB) void components_zap_kernel(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rcr,
                                                             uint32_t n, uint32_t e, uint64_t* __restrict__ zap)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if ((i & ~63ULL) >= n) return;                       // (whole waves)
    const uint32_t a = parent[e], b = parent[rcr[e]];
    bool out = false;
    if (i < n)
    {
        const uint32_t p = parent[i];
        out = p != a && p != b;
    }
    const uint64_t bal = __ballot(out);
    if (lane_id() == 0) zap[i >> 6] = bal;
}

}  // namespace goss
