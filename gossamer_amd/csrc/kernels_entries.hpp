// kernels_entries.hpp -- build-entry-edge-set on the decoded edge list of a graph: one record per edge whose from-node
// is not one-in-one-out (the path's length, its rounded mean multiplicity, the record of the mirror path).
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_contigs.hpp.
//
// What it replaces: EntryEdgeSet::build (EntryEdgeSet.cc:154-287) -- per entry edge a Graph::linearPath walk
// (Graph.tcc:19-46) that asks the Elias-Fano index for every step, then a second pass of rank(rc(end)) per entry.
// Here the link pass of kernels_tips.hpp (rcr, nxt, info) and contigs_mark_kernel (flag, pred) give the lists, and the
// ranking is the WEIGHTED instantiation of contigs_walk_kernel / contigs_double_kernel (kernels_contigs.hpp): the last
// edge e of a path, once resolved, holds pair[e] = (a, d) and w[e], and knows the whole path: start = a, len = d + 1,
// sum = w[e] + counts[a].  No edge is ordered by (path, position) and no address takes one atomic per edge of a long
// path.  A prefix sum over the start flags numbers the entries; the last edge of every path then writes the path's
// record where its start goes, and ends = prefix[rcr[e]]: rc(e) leaves a node that is not one-in-one-out exactly when
// e has no successor.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "kernels_contigs.hpp"

namespace goss {

// sc[i] = 1 for an entry edge: one scan numbers the entries (sc[n] becomes their number).
__global__ __launch_bounds__(kTB) void entries_flags_kernel(const uint8_t* __restrict__ flag, uint32_t n, uint64_t* __restrict__ sc)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) sc[i] = (flag[i] & kCtgStart) ? 1 : 0;
}

// The entry edges' values, in rank order.
template <class K>
__global__ __launch_bounds__(kTB) void entries_keys_kernel(const K* __restrict__ keys, const uint8_t* __restrict__ flag,
                                                           const uint64_t* __restrict__ sc, uint32_t n, K* __restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n && (flag[i] & kCtgStart)) out[sc[i]] = keys[i];
}

// The last edge of every path writes the path's record at its start's number:
//   len = edges visited, cnt = (uint32_t)round(double(sum) / double(len)) -- boost::math::round, half away from zero
//   (EntryEdgeSet.cc:85-86) --, ends = the number of rc(last edge) among the entries, as the two columns of a 40-bit
//   IntegerArray (value >> 32 in a byte, the low 32 bits).  Edges left open lie on cycles without a start.
__global__ __launch_bounds__(kTB) void entries_paths_kernel(const uint2* __restrict__ pd, const uint64_t* __restrict__ w,
                                                            const uint8_t* __restrict__ flag, const uint8_t* __restrict__ st,
                                                            const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ counts,
                                                            const uint64_t* __restrict__ sc, uint32_t n,
                                                            uint32_t* __restrict__ len_out, uint32_t* __restrict__ cnt_out,
                                                            uint8_t* __restrict__ ends_upr, uint32_t* __restrict__ ends_lwr,
                                                            ContigsReport* __restrict__ rep)
{
    uint32_t cyc = 0, longest = 0;
    for (uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x; i64 < n; i64 += (uint64_t)gridDim.x * kTB)
    {
        const uint32_t j = (uint32_t)i64;
        if (st[j] == kCtgOpen) { ++cyc; continue; }
        if (flag[j] & kCtgSucc) continue;
        const uint2 v = pd[j];
        const uint32_t len = v.y + 1u;
        const uint64_t sum = w[j] + counts[v.x];
        const uint64_t at = sc[v.x], mirror = sc[rcr[j]];
        len_out[at] = len;
        cnt_out[at] = (uint32_t)::round((double)sum / (double)len);
        ends_upr[at] = (uint8_t)(mirror >> 32);
        ends_lwr[at] = (uint32_t)mirror;
        longest = len > longest ? len : longest;
    }
    const unsigned long long c = ctg_wave_sum(cyc);
    const uint32_t l = ctg_wave_max(longest);
    if (lane_id() == 0)
    {
        if (c) atomicAdd(&rep->cycle_edges, c);
        if (l) atomicMax(&rep->longest, (unsigned long long)l);
    }
}

}  // namespace goss
