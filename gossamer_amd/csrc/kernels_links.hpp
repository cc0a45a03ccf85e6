// kernels_links.hpp -- read links: the reads threaded over the linear segments of a graph, and the table of the changes
// from one segment to the next (the "mapping reads" stage of thread-reads).
// Part of the kernel set of libgossgpu.so (gfx950); included through goss_kernels.hpp, after kernels_components.hpp.
//
// What it replaces: ReadLinker::push_back (GossCmdThreadReads.cc:321-402) over KmerAligner::kmerSegment
// (KmerAligner.hh:169-229) -- per forward (K+1)-window of every read one rank / select walk back along the linear path
// to its entry edge, then a serial state machine per read.  Here
//
//   seg_of[e]   the entry rank of the linear path that holds edge e, from the list ranking of graph_passes.hpp:
//               pair[e] = (start, distance) and the prefix sum over the start flags; kLinkNone on a cycle without a start
//   slots       one per BYTE of the batch, in read order.  A slot that starts a valid window holds the window's edge
//               rank or a miss; every other slot is the identity of every scan below, and a '\n' slot is a barrier
//               that resets the state: nothing per read lives in LDS or registers across a tile edge
//   scans       one three-phase scan (tile aggregates, one workgroup over the aggregates, tiles again) over a 64-bit
//               state with a non-commutative composition, instantiated four times:
//                 LinkPrevOp    the slot of the previous window of the read (only a window behind an 'N' needs it)
//                 LinkCarryOp   the aligner's state: valid / segment, with the carry of KmerAligner.hh:174-195
//                 LinkHitOp     windows that are no hit so far; the segment of the previous hit
//                 LinkEmitOp    the count at the previous change; records so far (the compaction)
//               and once more as a plain count to compact the windows (LinkPackOp)
//   reduction   the records (a << 32 | b, gap) sorted by the radix sort of count_path.hpp, then one segmented reduce
//               with two 64-bit sums per row: a wave reduces its runs with shuffles and adds once per run
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"
#include "goss_read_tile.hpp"
#include "kernels_tips.hpp"
#include "kernels_contigs.hpp"

namespace goss {

constexpr uint32_t kLinkNone = 0xFFFFFFFFu;              // seg_of: the edge lies on no linear path with an entry edge
constexpr uint32_t kLinkMiss = 0xFFFFFFFFu;              // a window that was not aligned (the same value: such an edge is a miss)
constexpr uint32_t kLinkPass = 0xFFFFFFFEu;              // "as before" in the states of the scans
constexpr uint32_t kLinkNoWin = 0xFFFFFFFEu;             // a slot that starts no window
constexpr uint32_t kLinkNonUnique = 0x80000000u;         // on a window's segment: the segment is not unique
enum { kLinkNl = 1, kLinkA = 2, kLinkRunStart = 4 };     // slot flags: '\n'; A_i; A_i but for from(e_i) = to(e_prev), to be compared

constexpr uint32_t kLinkItems = 8;                       // slots per lane in a scan
constexpr uint32_t kLinkTile = kTB * kLinkItems;

// goss_gpu_link_row (goss_gpu_links.h)
struct LinkRow { uint32_t a, b; unsigned long long count, gap_sum; };
static_assert(sizeof(LinkRow) == 24, "link row layout");

struct LinkReport {
    unsigned long long carried, hits, records, windows, misses, none, lines;    // (the first three: a scan's counters)
};

// ---- the segment of every edge -----------------------------------------------------------------------------------------

// seg_of[j] = the number of j's start among the entries (sc: the scanned start flags), kLinkNone where the ranking left
// j open; single[j] = 1 where j is the only edge that leaves its from-node.
__global__ __launch_bounds__(kTB) void links_segments_kernel(const uint2* __restrict__ pd, const uint8_t* __restrict__ st,
                                                             const uint64_t* __restrict__ sc, const uint8_t* __restrict__ info, uint32_t n,
                                                             uint32_t* __restrict__ seg_of, uint8_t* __restrict__ single,
                                                             LinkReport* __restrict__ rep)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    bool none = false;
    if (i < n)
    {
        none = st[i] == kCtgOpen;
        seg_of[i] = none ? kLinkNone : (uint32_t)sc[pd[i].x];
        single[i] = tips_group_size(info[i]) == 1u ? 1 : 0;
    }
    const uint64_t b = __ballot(none);
    if (lane_id() == 0 && b) atomicAdd(&rep->none, (unsigned long long)__popcll(b));
}

// ---- windows -------------------------------------------------------------------------------------------------------------

// The staging and lookup of components_mark_kernel, with the newline flags.  Per slot p of the tile: win[p] = the rank
// of the window's edge, kLinkMiss, or kLinkNoWin; flags[p] as the enum says.  The window before p in the same read is
// p - 1 exactly when byte p - 1 is a base (the window at p is valid); from(e_p) = to(e_{p-1}) then holds by itself.
template <class K>
__global__ __launch_bounds__(kTB) void links_windows_kernel(const K* __restrict__ keys, uint32_t n, uint32_t L, uint32_t bits,
                                                            const uint32_t* __restrict__ table, const uint8_t* __restrict__ single,
                                                            const uint8_t* __restrict__ bases, uint64_t nbytes, uint64_t ntiles,
                                                            uint32_t aligned, uint32_t* __restrict__ win, uint8_t* __restrict__ flags,
                                                            LinkReport* __restrict__ rep)
{
    __shared__ uint64_t s_codes[kMatchGroups / 4];
    __shared__ uint64_t s_inv[kMatchGroups / 8];
    __shared__ uint64_t s_nl[kMatchRuns];

    const uint64_t tile = unit_block();
    if (tile >= ntiles) return;
    const uint64_t t0 = tile * kMatchTile;
    const uint32_t lane = lane_id();

    tile_stage<true>(bases, nbytes, t0, aligned, s_codes, s_inv, s_nl);
    __syncthreads();

    const uint64_t lmask = (1ULL << L) - 1;              // (L <= 63)
    uint32_t nwin = 0, nmiss = 0, nline = 0;             // (lane 0 counts)
    for (uint32_t it = 0; it < kMatchRuns / kWaves; ++it)
    {
        const uint32_t run = wave_id() * (kMatchRuns / kWaves) + it;
        nline += (uint32_t)__popcll(s_nl[run]);
        const uint32_t q = run * 64 + lane;
        const uint64_t p = t0 + q;
        const bool valid = p < nbytes && tile_window_valid(s_inv, run, lane, lmask);
        uint32_t w = kLinkNoWin;
        uint32_t f = ((s_nl[run] >> lane) & 1ULL) ? kLinkNl : 0;
        if (valid)
        {
            K x, rc;
            tile_window_keys<K>(s_codes, q, L, &x, &rc);
            const uint32_t r = n ? tips_lower_bound(keys, n, L, bits, table, x) : 0u;
            w = kLinkMiss;
            if (r < n && keys[r] == x)
            {
                w = r;
                if (single[r])
                {
                    bool adjacent;
                    if (q) adjacent = !((s_inv[(q - 1) >> 6] >> ((q - 1) & 63u)) & 1ULL);
                    else
                    {
                        const uint32_t c = p ? (bases[p - 1] | 0x20u) : 0u;
                        adjacent = c == 'a' || c == 'c' || c == 'g' || c == 't';
                    }
                    f |= adjacent ? kLinkA : kLinkRunStart;
                }
            }
        }
        if (p < nbytes) { win[p] = w; flags[p] = (uint8_t)f; }
        const uint64_t vb = __ballot(valid), mb = __ballot(valid && w == kLinkMiss);
        nwin += (uint32_t)__popcll(vb);
        nmiss += (uint32_t)__popcll(mb);
    }
    if (lane == 0)
    {
        if (nwin) atomicAdd(&rep->windows, (unsigned long long)nwin);
        if (nmiss) atomicAdd(&rep->misses, (unsigned long long)nmiss);
        if (nline) atomicAdd(&rep->lines, (unsigned long long)nline);
    }
}

// ---- the scan ------------------------------------------------------------------------------------------------------------
//
// An Op gives: identity(), load(p) -- the element of slot p --, compose(l, r) -- l first, then r; associative, not
// commutative --, and emit(p, before, mine, cnt): `before` is the composition of the elements of every slot below p.
// cnt[3] are counters of the lane; the kernel adds them to op.counters[0..2] where that is not null.

template <class Op>
__device__ __forceinline__ uint2 links_wave_incl(uint2 v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        uint2 o;
        o.x = __shfl_up(v.x, d, 64);
        o.y = __shfl_up(v.y, d, 64);
        if ((int)lane_id() >= d) v = Op::compose(o, v);
    }
    return v;
}

// The composition of the lanes below this one across the workgroup, and of all of them.  sh: kWaves elements.
template <class Op>
__device__ __forceinline__ uint2 links_block_excl(uint2 v, uint2* sh, uint2* total)
{
    const uint2 inc = links_wave_incl<Op>(v);
    uint2 ex;
    ex.x = __shfl_up(inc.x, 1, 64);
    ex.y = __shfl_up(inc.y, 1, 64);
    if (lane_id() == 0) ex = Op::identity();
    if (lane_id() == 63) sh[wave_id()] = inc;
    __syncthreads();
    uint2 base = Op::identity(), tot = Op::identity();
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
    {
        const uint2 s = sh[w];
        if ((int)wave_id() > w) base = Op::compose(base, s);
        tot = Op::compose(tot, s);
    }
    __syncthreads();
    *total = tot;
    return Op::compose(base, ex);
}

template <class Op>
__global__ __launch_bounds__(kTB) void links_scan_reduce_kernel(Op op, uint64_t n, uint2* __restrict__ agg)
{
    __shared__ uint2 sh[kWaves];
    const uint64_t p0 = (uint64_t)blockIdx.x * kLinkTile + (uint64_t)threadIdx.x * kLinkItems;
    uint2 v = Op::identity();
#pragma unroll
    for (uint32_t j = 0; j < kLinkItems; ++j)
        if (p0 + j < n) v = Op::compose(v, op.load(p0 + j));
    uint2 tot;
    links_block_excl<Op>(v, sh, &tot);
    if (threadIdx.x == 0) agg[blockIdx.x] = tot;
}

// One workgroup: agg[t] becomes the composition of the aggregates of the tiles below t.
template <class Op>
__global__ __launch_bounds__(kTB) void links_scan_tiles_kernel(uint2* __restrict__ agg, uint64_t ntiles)
{
    __shared__ uint2 sh[kWaves];
    uint2 carry = Op::identity();
    for (uint64_t base = 0; base < ntiles; base += kTB)
    {
        const uint64_t t = base + threadIdx.x;
        const uint2 v = t < ntiles ? agg[t] : Op::identity();
        uint2 tot;
        const uint2 ex = links_block_excl<Op>(v, sh, &tot);
        if (t < ntiles) agg[t] = Op::compose(carry, ex);
        carry = Op::compose(carry, tot);
    }
}

template <class Op>
__global__ __launch_bounds__(kTB) void links_scan_apply_kernel(Op op, uint64_t n, const uint2* __restrict__ agg)
{
    __shared__ uint2 sh[kWaves];
    const uint64_t p0 = (uint64_t)blockIdx.x * kLinkTile + (uint64_t)threadIdx.x * kLinkItems;
    uint2 e[kLinkItems];
    uint2 v = Op::identity();
#pragma unroll
    for (uint32_t j = 0; j < kLinkItems; ++j)
    {
        e[j] = p0 + j < n ? op.load(p0 + j) : Op::identity();
        v = Op::compose(v, e[j]);
    }
    uint2 tot;
    uint2 run = Op::compose(agg[blockIdx.x], links_block_excl<Op>(v, sh, &tot));
    uint32_t cnt[3] = {0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kLinkItems; ++j)
    {
        if (p0 + j < n) op.emit(p0 + j, run, e[j], cnt);
        run = Op::compose(run, e[j]);
    }
    if (op.counters)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            const uint32_t s = tips_wave_sum(cnt[k]);
            if (lane_id() == 0 && s) atomicAdd(&op.counters[k], (unsigned long long)s);
        }
    }
}

// ---- the states ------------------------------------------------------------------------------------------------------------

// A copy: x = a value, or kLinkPass.
__device__ __forceinline__ uint32_t links_copy(uint32_t l, uint32_t r) { return r == kLinkPass ? l : r; }

// The slot of the previous window of the read (kLinkMiss: none), for the windows flagged kLinkRunStart: the K bases
// behind that window's first are compared with the first K of this one -- to(e_prev) = from(e_i), case ignored -- and
// the flag becomes kLinkA or nothing.
struct LinkPrevOp {
    const uint32_t* win;
    uint8_t* flags;
    const uint8_t* bases;
    uint32_t k;
    unsigned long long* counters;
    static __device__ __forceinline__ uint2 identity() { return make_uint2(kLinkPass, 0); }
    static __device__ __forceinline__ uint2 compose(uint2 l, uint2 r) { return make_uint2(links_copy(l.x, r.x), 0); }
    __device__ __forceinline__ uint2 load(uint64_t p) const
    {
        if (win[p] != kLinkNoWin) return make_uint2((uint32_t)p, 0);
        return make_uint2((flags[p] & kLinkNl) ? kLinkMiss : kLinkPass, 0);
    }
    __device__ __forceinline__ void emit(uint64_t p, uint2 before, uint2, uint32_t*) const
    {
        const uint8_t f = flags[p];
        if (!(f & kLinkRunStart)) return;
        bool same = before.x != kLinkPass && before.x != kLinkMiss;
        for (uint32_t j = 0; same && j < k; ++j)
            same = ((bases[(uint64_t)before.x + 1 + j] ^ bases[p + j]) & 0xDFu) == 0;
        flags[p] = (uint8_t)((f & ~kLinkRunStart) | (same ? kLinkA : 0));
    }
};

// The aligner.  A state s is a segment or kLinkMiss (not valid); an element is the function
//   s valid ? (x == kLinkPass ? s : x) : y
// window with A_i: (pass, fresh); window without: (fresh, fresh); '\n': (miss, miss); no window: (pass, miss).
__device__ __forceinline__ uint32_t links_carry_apply(uint2 f, uint32_t s) { return s != kLinkMiss ? (f.x == kLinkPass ? s : f.x) : f.y; }

struct LinkCarryOp {
    const uint32_t* win;
    const uint8_t* flags;
    const uint32_t* seg_of;
    const uint32_t* unique;           // a bit per entry, or null: every segment is unique
    uint32_t* segu;                   // out: the window's segment (| kLinkNonUnique), kLinkMiss, kLinkNoWin
    unsigned long long* counters;     // [0] carried windows
    static __device__ __forceinline__ uint2 identity() { return make_uint2(kLinkPass, kLinkMiss); }
    static __device__ __forceinline__ uint2 compose(uint2 l, uint2 r)
    {
        return make_uint2(l.x == kLinkPass ? r.x : links_carry_apply(r, l.x), links_carry_apply(r, l.y));
    }
    __device__ __forceinline__ uint2 load(uint64_t p) const
    {
        const uint32_t w = win[p];
        const uint8_t f = flags[p];
        if (w == kLinkNoWin) return (f & kLinkNl) ? make_uint2(kLinkMiss, kLinkMiss) : identity();
        const uint32_t fresh = w == kLinkMiss ? kLinkMiss : seg_of[w];
        return make_uint2((f & kLinkA) ? kLinkPass : fresh, fresh);
    }
    __device__ __forceinline__ void emit(uint64_t p, uint2 before, uint2 mine, uint32_t* cnt) const
    {
        if (win[p] == kLinkNoWin) { segu[p] = kLinkNoWin; return; }
        const uint32_t prev = links_carry_apply(before, kLinkMiss);
        uint32_t s = links_carry_apply(mine, prev);
        if (mine.x == kLinkPass && prev != kLinkMiss) ++cnt[0];
        if (s != kLinkMiss && unique && !((unique[s >> 5] >> (s & 31u)) & 1u)) s |= kLinkNonUnique;
        segu[p] = s;
    }
};

// Exact mode: every window in the graph takes the segment of its own edge.
__global__ __launch_bounds__(kTB) void links_exact_kernel(const uint32_t* __restrict__ win, const uint32_t* __restrict__ seg_of,
                                                          const uint32_t* __restrict__ unique, uint64_t n, uint32_t* __restrict__ segu)
{
    const uint64_t p = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (p >= n) return;
    uint32_t s = win[p];
    if (s != kLinkNoWin && s != kLinkMiss)
    {
        s = seg_of[s];
        if (s != kLinkMiss && unique && !((unique[s >> 5] >> (s & 31u)) & 1u)) s |= kLinkNonUnique;
    }
    segu[p] = s;
}

// The windows, compacted in read order: x counts them.
struct LinkPackOp {
    const uint32_t* segu;
    uint32_t* out;
    unsigned long long* counters;
    static __device__ __forceinline__ uint2 identity() { return make_uint2(0, 0); }
    static __device__ __forceinline__ uint2 compose(uint2 l, uint2 r) { return make_uint2(l.x + r.x, 0); }
    __device__ __forceinline__ uint2 load(uint64_t p) const { return make_uint2(segu[p] != kLinkNoWin ? 1u : 0u, 0); }
    __device__ __forceinline__ void emit(uint64_t p, uint2 before, uint2 mine, uint32_t*) const
    {
        if (mine.x) out[before.x] = segu[p];
    }
};

__device__ __forceinline__ bool links_is_hit(uint32_t s) { return s != kLinkNoWin && s != kLinkMiss && !(s & kLinkNonUnique); }

// The linker, first half.  x: windows that are no hit; y: the segment of the last hit of the read (a copy; '\n' sets
// kLinkMiss).  A hit whose segment differs from the last hit's -- or that has none before it: the hit that primes --
// resets the gap: pa[p] = the segment before (kLinkMiss for the priming hit), nh[p] = the windows that were no hit
// below p; every other slot gets pa[p] = kLinkPass.
struct LinkHitOp {
    const uint32_t* segu;
    const uint8_t* flags;
    uint32_t* pa;
    uint32_t* nh;
    unsigned long long* counters;     // [1] hits, [2] records ([0] is the carry scan's)
    static __device__ __forceinline__ uint2 identity() { return make_uint2(0, kLinkPass); }
    static __device__ __forceinline__ uint2 compose(uint2 l, uint2 r) { return make_uint2(l.x + r.x, links_copy(l.y, r.y)); }
    __device__ __forceinline__ uint2 load(uint64_t p) const
    {
        const uint32_t s = segu[p];
        if (s == kLinkNoWin) return make_uint2(0, (flags[p] & kLinkNl) ? kLinkMiss : kLinkPass);
        return links_is_hit(s) ? make_uint2(0, s) : make_uint2(1, kLinkPass);
    }
    __device__ __forceinline__ void emit(uint64_t p, uint2 before, uint2, uint32_t* cnt) const
    {
        const uint32_t s = segu[p];
        uint32_t a = kLinkPass;
        if (links_is_hit(s))
        {
            ++cnt[1];
            const uint32_t last = before.y == kLinkPass ? kLinkMiss : before.y;
            if (last != s)
            {
                a = last;
                nh[p] = before.x;
                if (last != kLinkMiss) ++cnt[2];
            }
        }
        pa[p] = a;
    }
};

// The linker, second half.  x: nh of the last reset (a copy); y: records so far.  A reset with a segment before it
// writes its record: (a << 32 | b, the windows that were no hit since the reset before).
struct LinkEmitOp {
    const uint32_t* segu;
    const uint32_t* pa;
    const uint32_t* nh;
    unsigned long long* rec_keys;
    uint32_t* rec_gaps;
    unsigned long long* counters;
    static __device__ __forceinline__ uint2 identity() { return make_uint2(kLinkPass, 0); }
    static __device__ __forceinline__ uint2 compose(uint2 l, uint2 r) { return make_uint2(links_copy(l.x, r.x), l.y + r.y); }
    __device__ __forceinline__ uint2 load(uint64_t p) const
    {
        const uint32_t a = pa[p];
        if (a == kLinkPass) return identity();
        return make_uint2(nh[p], a != kLinkMiss ? 1u : 0u);
    }
    __device__ __forceinline__ void emit(uint64_t p, uint2 before, uint2 mine, uint32_t*) const
    {
        if (!mine.y) return;
        rec_keys[before.y] = ((unsigned long long)pa[p] << 32) | segu[p];
        rec_gaps[before.y] = mine.x - before.x;          // (the priming hit of the read lies before: before.x is a count)
    }
};

// ---- the reduction -------------------------------------------------------------------------------------------------------

// head[i] = 1 where record i opens a row (the records are sorted).
__global__ __launch_bounds__(kTB) void links_heads_kernel(const unsigned long long* __restrict__ keys, uint64_t n, uint64_t* __restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// rows zeroed by the caller; row = the heads scanned (exclusive, n + 1 values): row[i + 1] counts the heads up to and
// including record i, whose row is therefore row[i + 1] - 1.  A wave reduces its 64 records by runs of one row with
// shuffles; the last lane of every run adds the run's two sums to the row, the first record of a row writes its a and b.
__global__ __launch_bounds__(kTB) void links_rows_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ gaps,
                                                         const uint64_t* __restrict__ row, uint64_t n, LinkRow* __restrict__ rows)
{
    const uint64_t i = (uint64_t)blockIdx.x * kTB + threadIdx.x;
    if ((i & ~63ULL) >= n) return;                       // (whole waves)
    const bool live = i < n;
    const uint32_t lane = lane_id();
    const uint64_t r = live ? row[i + 1] - 1 : ~0ULL;
    unsigned long long cnt = live ? 1 : 0, gap = live ? gaps[i] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const unsigned long long oc = __shfl_up(cnt, d, 64), og = __shfl_up(gap, d, 64);
        const uint64_t orow = __shfl_up(r, d, 64);
        if ((int)lane >= d && orow == r) { cnt += oc; gap += og; }
    }
    const uint64_t next = __shfl_down(r, 1, 64);
    if (!live) return;
    if (lane == 63 || next != r)
    {
        atomicAdd(&rows[r].count, cnt);
        atomicAdd(&rows[r].gap_sum, gap);
    }
    if (row[i + 1] == row[i] + 1)                        // (record i opens its row)
    {
        rows[r].a = (uint32_t)(keys[i] >> 32);
        rows[r].b = (uint32_t)keys[i];
    }
}

}  // namespace goss
