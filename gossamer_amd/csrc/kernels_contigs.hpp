// kernels_contigs.hpp -- print-contigs in its linear-segments form on the decoded edge list of a graph.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_tips.hpp.
//
// What it replaces: printLinearSegments (GossCmdPrintContigs.cc:49-193) and Graph::linearPath (Graph.tcc:21-46),
// one rank / select walk per base on one CPU thread.  Here the link pass of kernels_tips.hpp (rcr, nxt, info) turns
// the graph into disjoint lists:
//
//   start(i)  = !(out(from E[i]) == 1 && in(from E[i]) == 1) = !(group size at i == 1 && info[rcr[i]] & 7 == 1)
//   succ(i)   = out(to E[i]) == 1 && in(to E[i]) == 1        = info[i] & 7 == 1 && group size at rcr[i] == 1
//
// Every edge with a successor is the only predecessor of nxt[i], which is then no start: the edges fall into paths
// (a start, then successors) and cycles without a start.  The sequential loop of the reference, with its `seen`
// bitmap, takes the path that starts at i iff i <= rcr[end]: rcr[end] is the start of the mirror path and the only
// rank at which `seen` is consulted for this one.
//
// Position of every edge on its path is list ranking over the predecessor pointers: a bounded walk of `steps` pointers
// per lane (1 = none), then pointer doubling, one launch per round over the pairs the round before wrote.  No lane
// follows a path for a number of dependent loads that grows with the path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "kernels_tips.hpp"

namespace goss {

// Pointers a lane follows in the first ranking launch before doubling takes over (GOSS_GPU_CONTIGS_WALK overrides).
// 1 = doubling alone: a walk of 16, 64 or 256 pointers measured slower on fragmented graphs and on long paths alike
// (DESIGN.md section 4c).
constexpr uint32_t kContigsWalkSteps = 1;
// Steps of 64 path positions one wave reduces before it adds to a path's record (contigs_figures_kernel).
constexpr int kContigsFigSteps = 16;
// Output bytes one lane of contigs_text_kernel owns: one 16-byte store.
constexpr int kContigsTextRun = 16;
constexpr uint32_t kContigsGridBlocks = 2048;

enum { kCtgStart = 1, kCtgSucc = 2, kCtgTaken = 4 };                    // flag[i]
enum { kCtgOpen = 0, kCtgNew = 1, kCtgDone = 2 };                        // st[i]: resolved nowhere / in the current pairs / in both
enum { kSegIncludeFst = 1, kSegIncludeLst = 2, kSegPrinted = 4 };        // goss_gpu_segment.flags

struct ContigsReport {
    unsigned long long paths, taken, cycle_edges, longest, open, resolved;
};

// goss_gpu_segment (goss_gpu.h); while the paths are reduced, text_offset holds the path's first slot of `ord`.
struct SegRec {
    unsigned long long s, s2, text_offset, text_bytes, len;
    uint32_t first_rank, edges, min, max, flags, end_rank;
};

__device__ __forceinline__ unsigned long long ctg_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint32_t ctg_wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// flag[i], and pred[nxt[i]] = i for every edge that has a successor.
__global__ __launch_bounds__(kTB) void contigs_mark_kernel(const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                           const uint8_t* __restrict__ info, uint32_t n,
                                                           uint8_t* __restrict__ flag, uint32_t* __restrict__ pred)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const uint8_t mine = info[i], mirror = info[rcr[i]];
    const bool start = !(tips_group_size(mine) == 1u && tips_out_to(mirror) == 1u);
    const bool succ = tips_out_to(mine) == 1u && tips_group_size(mirror) == 1u;
    flag[i] = (uint8_t)((start ? kCtgStart : 0) | (succ ? kCtgSucc : 0));
    if (succ) pred[nxt[i]] = i;
}

// First ranking launch: every edge follows at most `steps` predecessor pointers.  pair = (ancestor, distance); an
// edge whose ancestor is a start is resolved.  `cur` gets every pair, `oth` the resolved ones (they are final).
// WEIGHTED (build-entry-edge-set) carries a u64 beside every pair: the multiplicities of the edge and of the d - 1
// edges between it and its ancestor, the ancestor itself left out.  Unweighted, counts / wcur / woth are null.
template <bool WEIGHTED>
__global__ __launch_bounds__(kTB) void contigs_walk_kernel(const uint32_t* __restrict__ pred, const uint8_t* __restrict__ flag,
                                                           const uint32_t* __restrict__ counts, uint32_t n, uint32_t steps,
                                                           uint2* __restrict__ cur, uint2* __restrict__ oth,
                                                           uint64_t* __restrict__ wcur, uint64_t* __restrict__ woth,
                                                           uint8_t* __restrict__ st, ContigsReport* __restrict__ rep)
{
    uint32_t open = 0;
    for (uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t j = (uint32_t)i64;
        uint32_t p = j, d = 0;
        uint64_t w = 0;
        bool done = flag[j] & kCtgStart;
        while (!done && d < steps)
        {
            if constexpr (WEIGHTED) w += counts[p];
            p = pred[p];
            ++d;
            done = flag[p] & kCtgStart;
        }
        const uint2 v = make_uint2(p, d);
        cur[j] = v;
        if constexpr (WEIGHTED) wcur[j] = w;
        if (done) { oth[j] = v; if constexpr (WEIGHTED) woth[j] = w; } else ++open;
        st[j] = done ? kCtgDone : kCtgOpen;
    }
    const unsigned long long tot = ctg_wave_sum(open);
    if (lane_id() == 0 && tot) atomicAdd(&rep->open, tot);
}

// One doubling round: (a, d) of an open edge becomes (ancestor of a, d + distance of a), read from the pairs of
// the round before (WEIGHTED: and w[j] += w[a]).  An edge resolved in the round before is copied once more, so that
// both arrays hold it.
template <bool WEIGHTED>
__global__ __launch_bounds__(kTB) void contigs_double_kernel(const uint2* __restrict__ in, uint2* __restrict__ out,
                                                             const uint8_t* __restrict__ flag, uint8_t* __restrict__ st,
                                                             uint32_t n, ContigsReport* __restrict__ rep,
                                                             const uint64_t* __restrict__ win, uint64_t* __restrict__ wout)
{
    uint32_t fresh = 0;
    for (uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t j = (uint32_t)i64;
        const uint8_t s = st[j];
        if (s == kCtgDone) continue;
        const uint2 v = in[j];
        uint64_t w;
        if constexpr (WEIGHTED) w = win[j];
        if (s == kCtgNew) { out[j] = v; if constexpr (WEIGHTED) wout[j] = w; st[j] = kCtgDone; continue; }
        const uint2 a = in[v.x];
        out[j] = make_uint2(a.x, v.y + a.y);
        if constexpr (WEIGHTED) wout[j] = w + win[v.x];
        if (flag[a.x] & kCtgStart) { st[j] = kCtgNew; ++fresh; }
    }
    const unsigned long long tot = ctg_wave_sum(fresh);
    if (lane_id() == 0 && tot) atomicAdd(&rep->resolved, tot);
}

// The last edge of every path tells the path's start its rank and the path's length; edges left open lie on cycles.
__global__ __launch_bounds__(kTB) void contigs_ends_kernel(const uint2* __restrict__ pd, const uint8_t* __restrict__ flag,
                                                           const uint8_t* __restrict__ st, uint32_t n,
                                                           uint32_t* __restrict__ end_of, uint32_t* __restrict__ len_of,
                                                           ContigsReport* __restrict__ rep)
{
    uint32_t cyc = 0;
    for (uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t j = (uint32_t)i64;
        if (st[j] == kCtgOpen) { ++cyc; continue; }
        if (flag[j] & kCtgSucc) continue;
        const uint2 v = pd[j];
        end_of[v.x] = j;
        len_of[v.x] = v.y + 1u;
    }
    const unsigned long long tot = ctg_wave_sum(cyc);
    if (lane_id() == 0 && tot) atomicAdd(&rep->cycle_edges, tot);
}

// The rule per path.  sc[i] = (1 << 32 | edges) for a taken start, else 0: one scan numbers the taken paths and lays
// them out in `ord`.
__global__ __launch_bounds__(kTB) void contigs_decide_kernel(uint8_t* __restrict__ flag, const uint32_t* __restrict__ rcr,
                                                             const uint32_t* __restrict__ end_of, const uint32_t* __restrict__ len_of,
                                                             uint32_t n, uint64_t* __restrict__ sc, ContigsReport* __restrict__ rep)
{
    uint32_t paths = 0, taken = 0, longest = 0;
    for (uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t i = (uint32_t)i64;
        const uint8_t f = flag[i];
        uint64_t v = 0;
        if (f & kCtgStart)
        {
            const uint32_t m = len_of[i];
            ++paths;
            longest = m > longest ? m : longest;
            if (i <= rcr[end_of[i]])
            {
                ++taken;
                v = (1ULL << 32) | m;
                flag[i] = (uint8_t)(f | kCtgTaken);
            }
        }
        sc[i] = v;
    }
    const unsigned long long p = ctg_wave_sum(paths), t = ctg_wave_sum(taken);
    const uint32_t l = ctg_wave_max(longest);
    if (lane_id() == 0)
    {
        if (p) atomicAdd(&rep->paths, p);
        if (t) atomicAdd(&rep->taken, t);
        if (l) atomicMax(&rep->longest, (unsigned long long)l);
    }
}

// Records of the taken paths, in rank order of their starts.
__global__ __launch_bounds__(kTB) void contigs_paths_kernel(const uint8_t* __restrict__ flag, const uint64_t* __restrict__ sc,
                                                            const uint32_t* __restrict__ end_of, const uint32_t* __restrict__ len_of,
                                                            uint32_t n, SegRec* __restrict__ recs)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n || !(flag[i64] & kCtgTaken)) return;
    const uint64_t v = sc[i64];
    SegRec r;
    r.s = 0; r.s2 = 0; r.text_offset = v & 0xFFFFFFFFULL; r.text_bytes = 0; r.len = 0;
    r.first_rank = (uint32_t)i64; r.edges = len_of[i64]; r.min = 0xFFFFFFFFu; r.max = 0; r.flags = 0; r.end_rank = end_of[i64];
    recs[v >> 32] = r;
}

// ord[first slot of the path + position] = rank, for the edges of the taken paths: one 4-byte scatter per edge.
__global__ __launch_bounds__(kTB) void contigs_order_kernel(const uint2* __restrict__ pd, const uint8_t* __restrict__ flag,
                                                            const uint8_t* __restrict__ st, const uint64_t* __restrict__ sc,
                                                            uint32_t n, uint32_t* __restrict__ ord)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n || st[i64] == kCtgOpen) return;
    const uint2 v = pd[i64];
    if (!(flag[v.x] & kCtgTaken)) return;
    ord[(uint32_t)sc[v.x] + v.y] = (uint32_t)i64;
}

// min, max, sum and sum of squares of the multiplicities per path.  `ord` is sorted by (path, position), so a path is
// a run of slots: a wave reduces 64 slots by runs with shuffles, carries the run that is still open at its last lane
// into the next step, and adds to a path's record only when a run closes or its kContigsFigSteps steps are over: a path
// of 10^6 edges adds about a thousand times, not once per edge.
__global__ __launch_bounds__(kTB) void contigs_figures_kernel(const uint32_t* __restrict__ ord, uint32_t total,
                                                              const uint32_t* __restrict__ counts, const uint2* __restrict__ pd,
                                                              const uint64_t* __restrict__ sc, SegRec* __restrict__ recs)
{
    const uint32_t lane = lane_id();
    const uint64_t wave = ((uint64_t)blockIdx.x * kTB + threadIdx.x) >> 6;
    const uint64_t k0 = wave * (64ULL * kContigsFigSteps);
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    uint32_t cid = kNone, cmin = 0, cmax = 0;                      // the carried run (the same in every lane)
    unsigned long long cs = 0, cs2 = 0;
    auto flush = [&](uint32_t id, uint32_t mn, uint32_t mx, unsigned long long s, unsigned long long s2) {
        SegRec* r = recs + id;
        atomicMin(&r->min, mn);
        atomicMax(&r->max, mx);
        atomicAdd(&r->s, s);
        atomicAdd(&r->s2, s2);
    };
    for (int it = 0; it < kContigsFigSteps; ++it)
    {
        const uint64_t k = k0 + (uint64_t)it * 64 + lane;
        const bool valid = k < total;
        if (__ballot(valid) == 0) break;
        uint32_t id = kNone, c = 0;
        if (valid)
        {
            const uint32_t j = ord[k];
            c = counts[j];
            id = (uint32_t)(sc[pd[j].x] >> 32);
        }
        const uint32_t prev = __shfl_up(id, 1);
        const uint64_t heads = __ballot(lane == 0 || prev != id);
        const uint32_t first = 63u - (uint32_t)__clzll((long long)(heads & ((2ULL << lane) - 1ULL)));
        uint32_t mn = c, mx = c;
        unsigned long long s = c, s2 = (unsigned long long)c * c;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1)
        {
            const uint32_t omn = __shfl_up(mn, d), omx = __shfl_up(mx, d);
            const unsigned long long os = __shfl_up(s, d), os2 = __shfl_up(s2, d);
            if (lane >= first + d)
            {
                mn = omn < mn ? omn : mn; mx = omx > mx ? omx : mx;
                s += os; s2 += os2;
            }
        }
        const bool tail = lane == 63u || (((heads >> 1) >> lane) & 1ULL);
        const uint32_t id0 = __shfl(id, 0);
        if (cid != kNone)
        {
            if (cid != id0) { if (lane == 0) flush(cid, cmin, cmax, cs, cs2); }
            else if (first == 0)
            {
                mn = cmin < mn ? cmin : mn; mx = cmax > mx ? cmax : mx;
                s += cs; s2 += cs2;
            }
        }
        if (tail && lane != 63u && id != kNone) flush(id, mn, mx, s, s2);
        cid = __shfl(id, 63); cmin = __shfl(mn, 63); cmax = __shfl(mx, 63);
        cs = __shfl(s, 63); cs2 = __shfl(s2, 63);
    }
    if (cid != kNone && lane == 0) flush(cid, cmin, cmax, cs, cs2);
}

// key >> 2 and key & mask(2 * K): the nodes of an edge of K + 1 bases
__device__ __forceinline__ Key1 ctg_from(const Key1& e) { Key1 r; r.lo = e.lo >> 2; return r; }
__device__ __forceinline__ Key2 ctg_from(const Key2& e) { Key2 r; r.lo = (e.lo >> 2) | (e.hi << 62); r.hi = e.hi >> 2; return r; }
__device__ __forceinline__ Key1 ctg_to(const Key1& e, uint32_t K) { Key1 r; r.lo = e.lo & ((1ULL << (2u * K)) - 1ULL); return r; }
__device__ __forceinline__ Key2 ctg_to(const Key2& e, uint32_t K)
{
    Key2 r = e;
    const uint32_t bits = 2u * K;                                 // < 128
    if (bits < 64u) { r.hi = 0; r.lo &= (1ULL << bits) - 1ULL; }
    else if (bits < 128u) r.hi &= bits == 64u ? 0ULL : ((1ULL << (bits - 64u)) - 1ULL);
    return r;
}

// Steps 4-6 per taken path: the include flags (canonical form of the two end nodes), the printed length, the two
// filters; pass[t] and bytes[t] feed the scans that number the segments and lay out the text.
template <class K>
__global__ __launch_bounds__(kTB) void contigs_select_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ rcr,
                                                             const uint8_t* __restrict__ info, SegRec* __restrict__ recs,
                                                             uint64_t npaths, uint32_t Kn, uint64_t min_length,
                                                             uint64_t min_coverage, uint32_t line, uint64_t* __restrict__ pass,
                                                             uint64_t* __restrict__ bytes)
{
    const uint64_t t = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (t >= npaths) return;
    SegRec* r = recs + t;
    const uint32_t first = r->first_rank, end = r->end_rank;
    const K fst = ctg_from(keys[first]), lst = ctg_to(keys[end], Kn);
    const bool inc_f = tips_out_to(info[rcr[first]]) == 0u || canonical(fst, revcomp(fst, Kn)) == fst;
    const bool inc_l = tips_out_to(info[end]) == 0u || canonical(lst, revcomp(lst, Kn)) != lst;
    uint64_t len = (uint64_t)r->edges + Kn;
    if (!inc_f) len -= Kn;
    if (len >= Kn && !inc_l) len -= Kn;
    const bool printed = len >= min_length && (uint64_t)r->min >= min_coverage;
    uint64_t b = 0;
    if (printed && len) b = len + (line ? (len + line - 1) / line : 1);
    r->len = len;
    r->text_bytes = b;
    r->flags = (inc_f ? kSegIncludeFst : 0u) | (inc_l ? kSegIncludeLst : 0u) | (printed ? kSegPrinted : 0u);
    pass[t] = printed ? 1 : 0;
    bytes[t] = b;
}

// The printed paths become the segments, numbered in rank order; base[s] = the path's first slot of `ord`.
__global__ __launch_bounds__(kTB) void contigs_compact_kernel(const SegRec* __restrict__ recs, uint64_t npaths,
                                                              const uint64_t* __restrict__ pass, const uint64_t* __restrict__ bytes,
                                                              SegRec* __restrict__ segs, uint32_t* __restrict__ base)
{
    const uint64_t t = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (t >= npaths) return;
    SegRec r = recs[t];
    if (!(r.flags & kSegPrinted)) return;
    const uint64_t s = pass[t];
    base[s] = (uint32_t)r.text_offset;
    r.text_offset = bytes[t];
    segs[s] = r;
}

// The bodies of all segments back to back, line ends in place.  A lane owns kContigsTextRun consecutive output bytes
// and writes them with one store; each byte is a function of (segment, offset in the segment) alone.
//   byte q of a segment with lines of `line` bases (0 = one line): q / (line + 1) full lines lie before it; column
//   `line`, or the segment's last byte, is the line end; else base number skip + lines * line + column of the path's
//   edges + K bases: the first K + 1 come from the first edge, every later one is the last base of an edge.
template <class K>
__global__ __launch_bounds__(kTB) void contigs_text_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ ord,
                                                           const SegRec* __restrict__ segs, const uint32_t* __restrict__ base,
                                                           uint64_t nsegs, uint64_t total, uint32_t Kn, uint32_t line,
                                                           uint8_t* __restrict__ text)
{
    const uint64_t o = ((uint64_t)blockIdx.x * kTB + threadIdx.x) * kContigsTextRun;
    if (o >= total) return;
    uint64_t lo = 0, hi = nsegs;                         // the last segment that begins at or before o
    while (lo < hi)
    {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (segs[mid].text_offset <= o) lo = mid + 1; else hi = mid;
    }
    uint64_t s = lo - 1;                                 // (segment 0 begins at 0)
    uint64_t off = segs[s].text_offset, nb = segs[s].text_bytes;
    uint64_t skip = (segs[s].flags & kSegIncludeFst) ? 0 : Kn;
    K e0 = keys[segs[s].first_rank];
    uint32_t b0 = base[s];
    uint32_t w[kContigsTextRun / 4] = {};
#pragma unroll
    for (int b = 0; b < kContigsTextRun; ++b)
    {
        const uint64_t at = o + b;
        uint32_t ch = 0;
        if (at < total)
        {
            while (at - off >= nb)
            {
                ++s;
                off = segs[s].text_offset; nb = segs[s].text_bytes;
                skip = (segs[s].flags & kSegIncludeFst) ? 0 : Kn;
                e0 = keys[segs[s].first_rank];
                b0 = base[s];
            }
            const uint64_t q = at - off;
            const uint64_t lines = line ? q / (line + 1u) : 0;
            const uint64_t col = q - lines * (line + 1u);
            if (q + 1 == nb || (line && col == line)) ch = '\n';
            else
            {
                const uint64_t p = skip + lines * line + col;
                const uint32_t code = p <= Kn ? (uint32_t)key_shr64(e0, 2u * (Kn - (uint32_t)p)) & 3u
                                              : (uint32_t)keys[ord[b0 + (uint32_t)(p - Kn)]].lo & 3u;
                ch = (0x54474341u >> (8u * code)) & 0xFFu;          // "ACGT"
            }
        }
        w[b >> 2] |= ch << (8 * (b & 3));
    }
    *(uint4*)(text + o) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace goss
