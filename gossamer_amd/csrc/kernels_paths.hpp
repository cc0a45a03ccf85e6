// kernels_paths.hpp -- trim-paths and clip-links on the decoded edge list of a graph: the two per-path cleaners
// beside prune-tips.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_tips.hpp.
//
// What it replaces: GossCmdTrimPaths.cc:78-248 (one Block per thread: select(i), inDegree, linearPath, rank of every
// reverse complement, one mutex for the zapped bits) and GossCmdClipLinks.cc:50-174 (one serial loop: outDegree,
// linearPath, beginEndRank and multiplicity of both end nodes' edges).  Both read the graph as given and OR bits into a
// separate bitset, so the removed set does not depend on the order of the starts; here the link pass of
// kernels_tips.hpp (rcr, nxt, info) answers every degree and one thread per start walks those arrays:
//
//   trim-paths   start: in(from(e)) == 0   (tips_flag_kernel)     goes iff l <= 2K [and, with the cutoff flag, no
//                                                                  edge of the path has a multiplicity >= cutoff]
//   clip-links   start: out(from(e)) >= 2  (paths_flag_kernel)    goes iff l <= 2K, 3 c(e) < S_out and 3 c(last) < S_in
//
// S_out = sum of the multiplicities of the group of e; S_in = sum of counts[rcr[r]] over the group of rcr[last]; both
// sums are u32 and wrap as the reference's do (GossCmdClipLinks.cc:53,67).  double(c) / double(s) < 1.0 / 3.0 is
// 3 c < s in 64 bits for s != 0 (at 3 c == s both sides round to the same double; otherwise they differ by at least
// 1 / (3 * 2^32)), and false for s == 0 (the quotient is +inf, or NaN for c == 0).
// Only rcr / nxt / info / counts are read; no kernel of the pass writes them.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kernels_common.hpp"
#include "kernels_tips.hpp"

namespace goss {

// The device report of both passes.  tips_flag_kernel, tips_gather_kernel and the link pass write `candidates`,
// `cursor` and `missing_rc` through a TipsReport*, so those three sit where TipsReport has them.
//   trim-paths: hits = paths, edges = zapped (sum of 2 l), why[0] = spared by the cutoff
//   clip-links: hits = links, edges = edges (sum of l),    why[0] = major at the fork, why[1] = major at the join
struct PathsReport {
    unsigned long long edges_before, edges_after, candidates, hits, edges;
    unsigned long long too_long, why[2], unused[3];
    unsigned long long missing_rc;          // ~0 = none
    unsigned long long cursor;              // append position of the candidate list
};
static_assert(sizeof(PathsReport) == sizeof(TipsReport) && offsetof(PathsReport, candidates) == offsetof(TipsReport, candidates) &&
              offsetof(PathsReport, missing_rc) == offsetof(TipsReport, missing_rc) &&
              offsetof(PathsReport, cursor) == offsetof(TipsReport, cursor), "the shared kernels write through a TipsReport");

// Candidate pass 1 of clip-links: bit i of `cand` = out(from(E[i])) >= 2; their number into the report.  Built like
// tips_flag_kernel: fixed grid, one report add per workgroup.
__global__ __launch_bounds__(kTB) void paths_flag_kernel(const uint8_t* __restrict__ info, uint32_t n, uint64_t* __restrict__ cand,
                                                         PathsReport* __restrict__ rep)
{
    __shared__ uint32_t sh[kWaves + 1];
    uint32_t mine = 0;                                 // (lane 0 of every wave counts)
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; (i & ~63ULL) < n; i += (uint64_t)gridDim.x * kTB)
    {
        const bool is = i < n && tips_group_size(info[i]) > 1u;
        const uint64_t bal = __ballot(is);
        if (lane_id() == 0) { cand[i >> 6] = bal; mine += __popcll(bal); }
    }
    uint32_t tot;
    block_excl_scan<uint32_t>(mine, sh, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&rep->candidates, (unsigned long long)tot);
}

enum { kPathNone = 0, kPathGoes, kPathTooLong, kPathWhy0, kPathWhy1 };

// u32 sum, wrapping, of counts[at(g0 + j)] over the group that `member` lies in
template <bool THROUGH_RC>
__device__ __forceinline__ uint32_t paths_group_sum(uint32_t member, const uint8_t* __restrict__ info, const uint32_t* __restrict__ rcr,
                                                    const uint32_t* __restrict__ counts)
{
    const uint8_t mi = info[member];
    const uint32_t g0 = member - tips_group_pos(mi), gn = tips_group_size(mi);
    uint32_t s = 0;
    for (uint32_t j = 0; j < gn; ++j) s += counts[THROUGH_RC ? rcr[g0 + j] : g0 + j];
    return s;
}

__device__ __forceinline__ bool paths_minor(uint32_t c, uint32_t s) { return s != 0u && 3ULL * c < (unsigned long long)s; }

// trim-paths (GossCmdTrimPaths.cc:87-148): the length alone decides; with `use_cutoff` (GOSS_PATHS_CUTOFF) a path that
// holds an edge of multiplicity >= cutoff is spared.
struct TrimPaths {
    uint32_t cutoff, use_cutoff;
    static constexpr uint32_t kPerEdge = 2;            // zapCount += 2 l
    __device__ __forceinline__ bool meets(const uint32_t* __restrict__ counts, uint32_t e) const
    {
        return use_cutoff && counts[e] >= cutoff;
    }
    __device__ __forceinline__ uint32_t judge(uint32_t, uint32_t, bool met, const uint32_t*, const uint8_t*, const uint32_t*) const
    {
        return met ? kPathWhy0 : kPathGoes;
    }
};

// clip-links (GossCmdClipLinks.cc:121-155): minor among the edges that leave from(beg), then minor among those that
// enter to(last).  A start that fails both is counted at the fork.
struct ClipLinks {
    static constexpr uint32_t kPerEdge = 1;            // edgesZapped += l
    __device__ __forceinline__ bool meets(const uint32_t*, uint32_t) const { return false; }
    __device__ __forceinline__ uint32_t judge(uint32_t beg, uint32_t last, bool, const uint32_t* __restrict__ rcr,
                                              const uint8_t* __restrict__ info, const uint32_t* __restrict__ counts) const
    {
        if (!paths_minor(counts[beg], paths_group_sum<false>(beg, info, rcr, counts))) return kPathWhy0;
        if (!paths_minor(counts[last], paths_group_sum<true>(rcr[last], info, rcr, counts))) return kPathWhy1;
        return kPathGoes;
    }
};

// Walk pass: one thread per start, in the shape of tips_walk_kernel.  The path is followed once to classify, at most
// 2K + 1 edges far, and once to mark; the report is added to once per wave and class.
template <class Rule>
__global__ __launch_bounds__(kTB) void paths_walk_kernel(const uint32_t* __restrict__ list, uint64_t ncand, uint32_t n, uint32_t K,
                                                         const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                         const uint8_t* __restrict__ info, const uint32_t* __restrict__ counts,
                                                         uint32_t* __restrict__ zap, PathsReport* __restrict__ rep, Rule rule)
{
    const uint64_t t = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    const uint32_t beg = t < ncand ? list[t] : 0xFFFFFFFFu;
    uint32_t cls = kPathNone, l = 1;
    if (beg < n)
    {
        const uint32_t maxl = 2u * K;
        // Graph::linearPath (Graph.tcc:19-46)
        uint32_t e = beg;
        bool met = rule.meets(counts, beg);
        for (;;)
        {
            if (tips_out_to(info[e]) != 1u || tips_group_size(info[rcr[e]]) != 1u) break;
            const uint32_t e2 = nxt[e];
            if (e2 == beg) break;
            e = e2;
            if (++l > maxl) { cls = kPathTooLong; break; }
            met = met || rule.meets(counts, e);
        }
        if (cls == kPathNone) cls = rule.judge(beg, e, met, rcr, info, counts);
    }
    const bool goes = cls == kPathGoes;
    {
        const uint32_t edges = tips_wave_sum(goes ? Rule::kPerEdge * l : 0u);
        const uint64_t b0 = __ballot(goes), b1 = __ballot(cls == kPathTooLong);
        const uint64_t b2 = __ballot(cls == kPathWhy0), b3 = __ballot(cls == kPathWhy1);
        if (lane_id() == 0)
        {
            if (b0) atomicAdd(&rep->hits, (unsigned long long)__popcll(b0));
            if (edges) atomicAdd(&rep->edges, (unsigned long long)edges);
            if (b1) atomicAdd(&rep->too_long, (unsigned long long)__popcll(b1));
            if (b2) atomicAdd(&rep->why[0], (unsigned long long)__popcll(b2));
            if (b3) atomicAdd(&rep->why[1], (unsigned long long)__popcll(b3));
        }
    }
    if (!goes) return;
    uint32_t e = beg;
    for (uint32_t s = 0; s < l; ++s)
    {
        const uint32_t r = rcr[e];
        atomicOr(&zap[e >> 5], 1u << (e & 31u));
        atomicOr(&zap[r >> 5], 1u << (r & 31u));
        e = nxt[e];
    }
}

}  // namespace goss
