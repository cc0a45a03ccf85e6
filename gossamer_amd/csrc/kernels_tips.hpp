// kernels_tips.hpp -- prune-tips on the decoded edge list of a graph: the first traversal on the device.
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, in this order.
//
// What it replaces: GossCmdPruneTips.cc:82-225 (one Block per thread: select(i), inDegree, linearPath,
// beginEndRank, multiplicity, rank of the reverse complement, all behind one mutex for the zapped bits) and
// Graph::remove(bitset) (Graph.cc).  Every rank/select there is a walk of the Elias-Fano index; here the
// edge list is decoded and sorted in HBM, and one "link pass" turns every degree the walk asks for into
// array arithmetic:
//
//   rcr[i]   u32  rank of rc(E[i])
//   nxt[i]   u32  rank of the first edge out of to(E[i])
//   info[i]  u8   bits 0-2 out(to(E[i])) (0..4), bits 3-4 out(from(E[i])) - 1, bits 5-6 position of E[i]
//                 among the edges of from(E[i]) (they are adjacent in the sorted list)
//
//   out(to(e))   = info[e] & 7                 in(to(e))   = out(from(rc e)) = group size at rcr[e]
//   out(from(e)) = group size at e             in(from(e)) = out(to(rc e))   = info[rcr[e]] & 7
//
// All decisions of one iteration read these arrays and the counts, which no kernel of the iteration
// writes; removals are bits OR-ed into a bitmap that is applied afterwards.  The result therefore does not
// depend on the order in which walkers run.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "kernels_runs.hpp"

namespace goss {

// goss_gpu_tips_report (goss_gpu.h), then the first edge index whose reverse complement is absent.
struct TipsReport {
    unsigned long long edges_before, edges_after, candidates, tips, zapped;
    unsigned long long too_long, both_joined, isolated, outweighed, joined_at_begin, joined_at_end;
    unsigned long long missing_rc;          // ~0 = none
    unsigned long long cursor;              // append position of the candidate list
};

// (e << 2) & mask(2*len): the smallest edge value that leaves to(e)
__device__ __forceinline__ Key1 tips_to_first(const Key1& e, uint32_t len)
{
    Key1 r;
    r.lo = (e.lo << 2) & ((1ULL << (2u * len)) - 1ULL);          // len <= 31 for one-word keys
    return r;
}
__device__ __forceinline__ Key2 tips_to_first(const Key2& e, uint32_t len)
{
    Key2 r;
    r.lo = e.lo << 2;
    r.hi = (e.hi << 2) | (e.lo >> 62);
    const uint32_t bits = 2u * len;                               // 64 <= bits <= 128 for two-word keys
    if (bits < 128u) r.hi &= bits <= 64u ? 0ULL : ((1ULL << (bits - 64u)) - 1ULL);
    return r;
}

// from(a) == from(b)
__device__ __forceinline__ bool tips_same_from(const Key1& a, const Key1& b) { return ((a.lo ^ b.lo) >> 2) == 0; }
__device__ __forceinline__ bool tips_same_from(const Key2& a, const Key2& b) { return a.hi == b.hi && ((a.lo ^ b.lo) >> 2) == 0; }

// The first `bits` bits of a len-mer (bits <= 32, bits <= 2*len).
template <class K>
__device__ __forceinline__ uint32_t tips_bucket(const K& k, uint32_t len, uint32_t bits)
{
    return bits ? (uint32_t)key_shr64(k, 2u * len - bits) : 0u;
}

// Bucket table over the first `bits` bits: table[b] = rank of the first key whose bucket is >= b, for
// b in [0, 2^bits]; table[2^bits] = n.  Every boundary between two neighbours of the sorted list is filled
// by the wave of the thread that sees it, 64 entries per step, so that one long gap (skewed keys) costs
// gap/64 steps of one wave and not gap stores of one lane.
template <class K>
__global__ __launch_bounds__(kTB) void tips_table_kernel(const K* __restrict__ keys, uint32_t n, uint32_t len, uint32_t bits,
                                                         uint32_t* __restrict__ table)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    // entries (first, last] get the value i
    uint32_t first = 0, last = 0;
    bool have = false;
    if (i < n)
    {
        const uint32_t b = tips_bucket(keys[i], len, bits);
        if (i == 0) { first = 0; last = b; have = true; table[0] = 0; }
        else
        {
            const uint32_t bp = tips_bucket(keys[i - 1], len, bits);
            if (bp < b) { first = bp; last = b; have = true; }
        }
    }
    const uint32_t lane = lane_id();
    uint64_t todo = __ballot(have);
    while (todo)
    {
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t f = __shfl(first, src), l = __shfl(last, src);
        const uint32_t v = (uint32_t)__shfl((unsigned int)i, src);
        for (uint64_t e = (uint64_t)f + 1 + lane; e <= l; e += 64) table[e] = v;
    }
    // the tail: everything above the last key's bucket is n (its own wave, after the loop above)
    const uint64_t lastw = ((uint64_t)(n - 1) >> 6) << 6;
    if (i >= lastw && i < lastw + 64)
    {
        const uint32_t bl = tips_bucket(keys[n - 1], len, bits);
        const uint64_t top = 1ULL << bits;
        for (uint64_t e = (uint64_t)bl + 1 + lane; e <= top; e += 64) table[e] = n;
    }
}

// lower_bound(keys, x): through the bucket table when there is one (bits > 0), else over the whole list.
template <class K>
__device__ __forceinline__ uint32_t tips_lower_bound(const K* __restrict__ keys, uint32_t n, uint32_t len, uint32_t bits,
                                                     const uint32_t* __restrict__ table, const K& x)
{
    uint32_t lo = 0, hi = n;
    if (bits)
    {
        const uint32_t b = tips_bucket(x, len, bits);
        lo = table[b];
        hi = table[b + 1];
    }
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Link pass: one thread per edge, two searches.
template <class K>
__global__ __launch_bounds__(kTB) void tips_link_kernel(const K* __restrict__ keys, uint32_t n, uint32_t len, uint32_t bits,
                                                        const uint32_t* __restrict__ table, uint32_t* __restrict__ rcr,
                                                        uint32_t* __restrict__ nxt, uint8_t* __restrict__ info,
                                                        TipsReport* __restrict__ rep)
{
    const uint64_t i64 = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i64 >= n) return;
    const uint32_t i = (uint32_t)i64;
    const K e = keys[i];
    // the edges of from(e): at most four, adjacent
    uint32_t pos = 0, size = 1;
    while (pos < 3u && i > pos && tips_same_from(keys[i - pos - 1u], e)) ++pos;
    size += pos;
    for (uint32_t j = 1; j < 4u && size < 4u && (uint64_t)i + j < n && tips_same_from(keys[i + j], e); ++j) ++size;
    // the reverse complement's rank
    const K rc = revcomp(e, len);
    uint32_t r = tips_lower_bound(keys, n, len, bits, table, rc);
    if (r >= n || keys[r] != rc)
    {
        atomicMin(&rep->missing_rc, (unsigned long long)i);
        r = i;                                        // (stays inside the arrays; the iteration is abandoned)
    }
    rcr[i] = r;
    // the edges out of to(e)
    const K t = tips_to_first(e, len);
    const uint32_t q = tips_lower_bound(keys, n, len, bits, table, t);
    uint32_t deg = 0;
    while (deg < 4u && (uint64_t)q + deg < n && tips_same_from(keys[q + deg], t)) ++deg;
    nxt[i] = q < n ? q : i;
    info[i] = (uint8_t)(deg | ((size - 1u) << 3) | (pos << 5));
}

__device__ __forceinline__ uint32_t tips_out_to(uint8_t info) { return info & 7u; }
__device__ __forceinline__ uint32_t tips_group_size(uint8_t info) { return ((info >> 3) & 3u) + 1u; }
__device__ __forceinline__ uint32_t tips_group_pos(uint8_t info) { return (info >> 5) & 3u; }

// Sum over the wave, in every lane.
__device__ __forceinline__ uint32_t tips_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// The two candidate kernels run on a fixed grid (kTipsGridBlocks workgroups) and add to the report once per workgroup: one
// atomic per wave on one address was most of their time (7 ms each over 1.1e8 edges, 0.6 % of them candidates).
constexpr uint32_t kTipsGridBlocks = 2048;

// Candidate pass 1: bit i of `cand` = in(from(E[i])) == 0; their number into the report.  One wave per 64 edges.
__global__ __launch_bounds__(kTB) void tips_flag_kernel(const uint32_t* __restrict__ rcr, const uint8_t* __restrict__ info, uint32_t n,
                                                        uint64_t* __restrict__ cand, TipsReport* __restrict__ rep)
{
    __shared__ uint32_t sh[kWaves + 1];
    uint32_t mine = 0;                                 // (lane 0 of every wave counts)
    for (uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x; (i & ~63ULL) < n; i += (uint64_t)gridDim.x * kTB)
    {
        const bool is = i < n && tips_out_to(info[rcr[i]]) == 0u;
        const uint64_t bal = __ballot(is);
        if (lane_id() == 0) { cand[i >> 6] = bal; mine += __popcll(bal); }
    }
    uint32_t tot;
    block_excl_scan<uint32_t>(mine, sh, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&rep->candidates, (unsigned long long)tot);
}

// Candidate pass 2: the ranks of the flagged edges, packed (in any order: the walkers are independent).  A
// workgroup takes a contiguous piece of the bitmap, one word per thread and step: it counts its bits, reserves its
// stretch of the list with one atomic and writes.
__global__ __launch_bounds__(kTB) void tips_gather_kernel(const uint64_t* __restrict__ cand, uint64_t nwords, uint64_t words_per_block,
                                                          uint32_t* __restrict__ list, uint64_t cap, TipsReport* __restrict__ rep)
{
    __shared__ uint32_t sh[kWaves + 1];
    __shared__ unsigned long long base;
    const uint64_t w0 = (uint64_t)blockIdx.x * words_per_block;
    const uint64_t w1 = w0 + words_per_block < nwords ? w0 + words_per_block : nwords;
    uint32_t mine = 0;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kTB) mine += __popcll(cand[w]);
    uint32_t tot;
    const uint32_t before = block_excl_scan<uint32_t>(mine, sh, &tot);
    if (tot == 0) return;                              // (the whole workgroup)
    if (threadIdx.x == 0) base = atomicAdd(&rep->cursor, (unsigned long long)tot);
    __syncthreads();
    uint64_t o = base + before;
    for (uint64_t w = w0 + threadIdx.x; w < w1; w += kTB)
    {
        uint64_t bits = cand[w];
        while (bits)
        {
            const uint32_t b = (uint32_t)__ffsll((unsigned long long)bits) - 1u;
            bits &= bits - 1;
            if (o < cap) list[o] = (uint32_t)(w * 64 + b);
            ++o;
        }
    }
}

// Walk pass: one thread per candidate (GossCmdPruneTips.cc:93-225).  The path is followed twice -- once to
// classify, once to mark -- instead of being kept in a per-thread array.  The report is added to once per wave
// and class.
enum { kTipNone = 0, kTipTooLong, kTipBoth, kTipIsolated, kTipOutweighed, kTipAtBegin, kTipAtEnd };

__global__ __launch_bounds__(kTB) void tips_walk_kernel(const uint32_t* __restrict__ list, uint64_t ncand, uint32_t n, uint32_t K,
                                                        const uint32_t* __restrict__ rcr, const uint32_t* __restrict__ nxt,
                                                        const uint8_t* __restrict__ info, const uint32_t* __restrict__ counts,
                                                        uint32_t* __restrict__ zap, TipsReport* __restrict__ rep)
{
    const uint64_t t = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    uint32_t beg = t < ncand ? list[t] : 0xFFFFFFFFu;
    uint32_t cls = kTipNone, l = 1;
    if (beg < n)
    {
        const uint32_t maxl = 2u * K;
        // Graph::linearPath (Graph.tcc:19-46)
        uint32_t e = beg;
        for (;;)
        {
            if (tips_out_to(info[e]) != 1u || tips_group_size(info[rcr[e]]) != 1u) break;
            const uint32_t e2 = nxt[e];
            if (e2 == beg) break;
            e = e2;
            if (++l > maxl) { cls = kTipTooLong; break; }
        }
        if (cls == kTipNone)
        {
            const uint32_t end = e;
            const bool begCon = tips_group_size(info[beg]) > 1u;                   // (in(from(beg)) is 0 here)
            const uint32_t rend = rcr[end];
            const bool endCon = tips_group_size(info[rend]) > 1u || tips_out_to(info[end]) > 0u;
            if (begCon && endCon) cls = kTipBoth;
            else if (!begCon && !endCon) cls = kTipIsolated;
            else
            {
                // the edges out of the attaching node: the group of rc(end) (node rc(to(end))) or of beg (node from(beg))
                const uint32_t at = endCon ? rend : beg;
                const uint32_t c = counts[endCon ? end : beg];
                const uint8_t ai = info[at];
                const uint32_t g0 = at - tips_group_pos(ai), gn = tips_group_size(ai);
                cls = endCon ? kTipAtEnd : kTipAtBegin;
                for (uint32_t j = 0; j < gn; ++j)
                    if (counts[g0 + j] < c) cls = kTipOutweighed;
            }
        }
    }
    const bool tip = cls == kTipAtBegin || cls == kTipAtEnd;
    {
        const uint32_t lane = lane_id();
        const uint32_t zapped = tips_wave_sum(tip ? 2u * l : 0u);
        const uint64_t b1 = __ballot(cls == kTipTooLong), b2 = __ballot(cls == kTipBoth), b3 = __ballot(cls == kTipIsolated);
        const uint64_t b4 = __ballot(cls == kTipOutweighed), b5 = __ballot(cls == kTipAtBegin), b6 = __ballot(cls == kTipAtEnd);
        if (lane == 0)
        {
            if (b1) atomicAdd(&rep->too_long, (unsigned long long)__popcll(b1));
            if (b2) atomicAdd(&rep->both_joined, (unsigned long long)__popcll(b2));
            if (b3) atomicAdd(&rep->isolated, (unsigned long long)__popcll(b3));
            if (b4) atomicAdd(&rep->outweighed, (unsigned long long)__popcll(b4));
            if (b5) atomicAdd(&rep->joined_at_begin, (unsigned long long)__popcll(b5));
            if (b6) atomicAdd(&rep->joined_at_end, (unsigned long long)__popcll(b6));
            if (b5 | b6) atomicAdd(&rep->tips, (unsigned long long)__popcll(b5 | b6));
            if (zapped) atomicAdd(&rep->zapped, (unsigned long long)zapped);
        }
    }
    if (!tip) return;
    uint32_t e = beg;
    for (uint32_t s = 0; s < l; ++s)
    {
        const uint32_t r = rcr[e];
        atomicOr(&zap[e >> 5], 1u << (e & 31u));
        atomicOr(&zap[r >> 5], 1u << (r & 31u));
        e = nxt[e];
    }
}

// Compaction by the removal bitmap, in the tiles of select_count_kernel / select_write_kernel
// (kernels_runs.hpp): a tile of kRedTile items is kRedTile/32 words of the bitmap, which is padded to whole
// tiles with zero bits.
__global__ __launch_bounds__(kTB) void tips_keep_count_kernel(const uint32_t* __restrict__ zap, uint64_t n,
                                                              uint64_t* __restrict__ tile_counts)
{
    __shared__ uint32_t sh[kWaves + 1];
    constexpr uint32_t kWords = kRedTile / 32;
    static_assert(kWords <= kTB, "one bitmap word per thread");
    const uint64_t base = (uint64_t)blockIdx.x * kRedTile;
    uint32_t c = 0;
    if (threadIdx.x < kWords) c = __popc(zap[(uint64_t)blockIdx.x * kWords + threadIdx.x]);
    uint32_t tot;
    block_excl_scan<uint32_t>(c, sh, &tot);
    if (threadIdx.x == 0)
    {
        const uint64_t items = n - base < (uint64_t)kRedTile ? n - base : (uint64_t)kRedTile;
        tile_counts[blockIdx.x] = items - tot;
    }
}

template <class K>
__global__ __launch_bounds__(kTB) void tips_keep_write_kernel(const K* __restrict__ keys, const uint32_t* __restrict__ counts,
                                                              uint64_t n, const uint32_t* __restrict__ zap,
                                                              const uint64_t* __restrict__ tile_offsets,
                                                              K* __restrict__ out_keys, uint32_t* __restrict__ out_counts)
{
    __shared__ uint32_t cnt[kRedItems * kWaves];
    const uint64_t base = (uint64_t)blockIdx.x * kRedTile;
    const uint32_t lane = lane_id(), w = wave_id();
    const uint64_t lt_mask = (1ULL << lane) - 1ULL;
    uint32_t flags = 0;
#pragma unroll
    for (int j = 0; j < kRedItems; ++j)
    {
        const uint64_t i = base + (uint64_t)j * kTB + threadIdx.x;
        const bool keep = i < n && !((zap[i >> 5] >> (i & 31u)) & 1u);
        if (keep) flags |= 1u << j;
        const uint64_t bal = __ballot(keep);
        if (lane == 0) cnt[j * kWaves + w] = __popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x < 64)
    {
        uint32_t c = cnt[threadIdx.x];
        uint32_t inc = wave_incl_scan(c);
        cnt[threadIdx.x] = inc - c;
    }
    __syncthreads();
    const uint64_t tile_off = tile_offsets[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kRedItems; ++j)
    {
        const bool keep = (flags >> j) & 1u;
        const uint64_t bal = __ballot(keep);
        if (keep)
        {
            const uint64_t i = base + (uint64_t)j * kTB + threadIdx.x;
            const uint64_t o = tile_off + cnt[j * kWaves + w] + __popcll(bal & lt_mask);
            out_keys[o] = keys[i];
            out_counts[o] = counts[i];
        }
    }
}

}  // namespace goss
