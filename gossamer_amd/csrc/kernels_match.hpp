// kernels_match.hpp -- reads against one KmerSet / Graph resident in HBM (goss_gpu_object_match_reads): from base
// bytes to per-read window and hit counts in one pass, the window keys never leaving the registers.
//
// The input is cut into tiles of 2,048 byte positions, one workgroup each, whatever the reads are: a read is the
// stretch between two '\n', so the read a position belongs to is the number of '\n' before it -- a count per tile
// (match_count_newlines_kernel), one device scan, and inside the tile a popcount over a 64-bit mask.  A read of a
// million bases is 489 tiles on 489 workgroups like any other million bytes.
//
// A tile is staged once, by goss_read_tile.hpp (tile_stage<true>): 2-bit codes, non-base flags and newline flags in
// three LDS bit arrays, the tile's 2,048 positions plus a halo of 64.  The window that starts at a position is valid
// when its L flag bits are clear (tile_window_valid) and its key and reverse complement are a funnel shift of two or
// three LDS words (tile_window_keys): normalising costs one more base-4 reversal, no loop over L.  What is left is the
// walk, rd_sparse_access_rank on the object's k-mers / edges only: the multiplicity arrays are never touched.
//
// A wave takes 8 consecutive runs of 64 positions.  The reads inside a run are lane intervals between newline bits:
// ballots of "valid" and "present" are cut by each interval's first lane (popcount under the interval's mask) and
// added to per-read counters in LDS; after the tile, the non-zero counters go to the output arrays with one vector
// atomic each (a read that spans tiles receives several).  Integer sums: the result does not depend on the order.
//
// GOSS_MATCH_ANY: a lane skips its walk when its read's LDS counter is already non-zero (earlier runs of this tile;
// for the tile's first read also what earlier tiles left in hits[]), and inside a run every eighth window walks
// first -- the other seven follow only where their read is still unmatched after that ballot.
//
// What only some modes read arrives in one MatchAux: the two bitmaps, the taxonomy's view.
//
// Classify mode (goss_gpu_object_classify_reads) is the count mode's walk with the rank kept: a hit at rank r reads bit r
// of the two bitmaps, c = 2 * aux.lhs[r] + aux.rhs[r], and the read's word is the OR of 1 << c over its hits -- four
// ballots a run cut by the same lane intervals, one LDS atomicOr per interval, one global atomicOr per read and tile.
//
// The two taxonomy modes (goss_gpu_object_taxo_annotate / _classify_reads, kernels_taxo.hpp) also keep the rank and read
// aux.tx.  Annotate: the read's class comes from a per-read array (tx.read_class), and a hit at rank r joins it into
// ann[r] by lca with a compare-and-swap loop that does not write where ann[r] already is the join; windows and hits
// are counted as in count mode.  Taxon: a
// hit reads ann[r] (a rank without a class is counted and otherwise ignored), the classes of a read's lanes in a run
// are joined by taxo_combine -- one ballot finds the usual case, all of them the same class, which is one LDS
// compare-and-swap join by one lane; otherwise the hit lanes join one by one -- and after the tile one global join per
// read and tile.  Both joins are order-free, so the arrays do not depend on the scheduling.
//
// Colour mode (goss_gpu_object_colour_reads) is the classify mode's walk with one 8-byte load per hit, aux.colours[r],
// and a 64-bit word per read: s_hit holds 64-bit words in this instantiation only (MatchHitWord).  The OR over a lane
// interval takes the taxon mode's shape: consecutive windows of a read usually bring the same word, so one ballot asks
// whether any hit lane differs from the first hit lane of its interval; if none does, that lane ORs its word into LDS.
// Otherwise an inclusive OR scan runs up the lanes in six shuffle steps on both halves, a step taken only from a lane
// of the same interval, and the interval's last lane ORs what it holds.  After the tile one global 64-bit atomicOr per
// read and tile with a non-zero word.  hits[] is then an array of 64-bit words.
//
// A walk that cannot answer (damaged image) leaves the lowest such byte position in bad[0]; a read whose window
// count reaches 2^32 - 1 leaves its index in bad[1].
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "goss_read_tile.hpp"
#include "goss_reader.hpp"
#include "kernels_common.hpp"
#include "kernels_query.hpp"
#include "kernels_taxo.hpp"

namespace goss {

enum : uint32_t { kMatchNormalize = 1, kMatchAny = 4 };
// what hits[] receives: a sum, 1 / 0, a 4-bit mask, a sum (and ann[] the lca), the join of the classes, a 64-bit word
enum : int { kModeCount = 0, kModeAny = 1, kModeClassify = 2, kModeAnnotate = 3, kModeTaxon = 4, kModeColour = 5 };

// a read's accumulator in LDS: 32 bits but for the colour mode's word
template <int MODE> struct MatchHitWord { typedef uint32_t type; };
template <> struct MatchHitWord<kModeColour> { typedef unsigned long long type; };

// what only some modes read: kModeClassify the two bitmaps (bit r = rank r), kModeAnnotate / kModeTaxon the taxonomy,
// kModeColour the word per rank
struct MatchAux {
    const uint64_t* lhs = nullptr;
    const uint64_t* rhs = nullptr;
    TaxoView tx;
    const uint64_t* colours = nullptr;
};

// tiles[t] = number of '\n' in tile t; one wave per tile
__global__ __launch_bounds__(256) void match_count_newlines_kernel(const uint8_t* __restrict__ bases, uint64_t nbytes, uint64_t ntiles,
                                                                   uint64_t* __restrict__ tiles, uint32_t aligned)
{
    const uint64_t t = (uint64_t)unit_block() * kWaves + wave_id();
    if (t >= ntiles) return;
    uint32_t n = 0;
#pragma unroll
    for (uint32_t it = 0; it < kMatchTile / 512; ++it)
    {
        const uint64_t pos = t * kMatchTile + it * 512 + lane_id() * 8;
        if (pos >= nbytes) continue;
        const uint64_t w = match_load8(bases, nbytes, pos, aligned);
        n += __popc(newline_flags((uint32_t)w)) + __popc(newline_flags((uint32_t)(w >> 32)));
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) n += __shfl_xor(n, d, 64);
    if (lane_id() == 0) tiles[t] = n;
}

// out[0..2] += sums over the reads: windows, hits, reads with a hit (hits NULL: the windows only); starts[reads] = end
__global__ __launch_bounds__(256) void match_sums_kernel(const uint32_t* __restrict__ windows, const uint32_t* __restrict__ hits, uint64_t reads,
                                                         unsigned long long* __restrict__ out, uint64_t* __restrict__ starts, uint64_t end)
{
    unsigned long long w = 0, h = 0, m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < reads; i += (uint64_t)gridDim.x * blockDim.x)
    {
        w += windows[i];
        const uint32_t x = hits ? hits[i] : 0;
        h += x;
        m += x ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1)
    {
        w += __shfl_xor(w, d, 64);
        h += __shfl_xor(h, d, 64);
        m += __shfl_xor(m, d, 64);
    }
    if (lane_id() == 0)
    {
        if (w) atomicAdd(&out[0], w);
        if (h) atomicAdd(&out[1], h);
        if (m) atomicAdd(&out[2], m);
    }
    if (starts && blockIdx.x == 0 && threadIdx.x == 0) starts[reads] = end;
}

// classes[i] & 15 counted into out[0..15]: an LDS histogram per block, one global add per non-zero bin
__global__ __launch_bounds__(256) void classify_sums_kernel(const uint32_t* __restrict__ classes, uint64_t reads, unsigned long long* __restrict__ out)
{
    __shared__ uint32_t s_bin[16];
    if (threadIdx.x < 16) s_bin[threadIdx.x] = 0;
    __syncthreads();
    // (32-bit bins: a block of a grid of 2,048 sees 2^32 reads only in an input of 2^43)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < reads; i += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(&s_bin[classes[i] & 15u], 1u);
    __syncthreads();
    if (threadIdx.x < 16 && s_bin[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s_bin[threadIdx.x]);
}

template <class K, int MODE>
__global__ __launch_bounds__(256) void match_reads_kernel(QueryObj o, const uint8_t* __restrict__ bases, uint64_t nbytes, uint64_t ntiles,
                                                          const uint64_t* __restrict__ tile_read, uint32_t flags, uint32_t aligned,
                                                          uint32_t* __restrict__ windows, uint32_t* __restrict__ hits,
                                                          uint64_t* __restrict__ starts, unsigned long long* __restrict__ bad, MatchAux aux)
{
    const uint64_t* __restrict__ lhs = aux.lhs;
    const uint64_t* __restrict__ rhs = aux.rhs;
    const TaxoView& tx = aux.tx;
    constexpr bool ANY = MODE == kModeAny, CLS = MODE == kModeClassify, ANN = MODE == kModeAnnotate, TAX = MODE == kModeTaxon;
    constexpr bool COL = MODE == kModeColour;
    typedef typename MatchHitWord<MODE>::type HitWord;
    __shared__ uint64_t s_codes[kMatchGroups / 4];       // 32 bases per word, first base lowest
    __shared__ uint64_t s_inv[kMatchGroups / 8];         // bit = not one of ACGTacgt (or beyond the input)
    __shared__ uint64_t s_nl[kMatchRuns];                // bit = '\n'
    __shared__ uint32_t s_pre[kMatchRuns + 1];           // newlines before each run; [kMatchRuns] = in the tile
    __shared__ uint32_t s_win[kMatchTile + 1];           // per read that touches the tile
    __shared__ HitWord s_hit[kMatchTile + 1];
    __shared__ uint32_t s_prev_nl;                       // the byte before the tile is '\n'

    const uint64_t tile = unit_block();
    if (tile >= ntiles) return;
    const uint64_t t0 = tile * kMatchTile;
    const uint64_t read0 = tile_read[tile];              // the read the tile's first position belongs to
    const uint32_t L = o.len;
    const uint32_t lane = lane_id();

    tile_stage<true>(bases, nbytes, t0, aligned, s_codes, s_inv, s_nl);
    if (threadIdx.x == 0) s_prev_nl = t0 && bases[t0 - 1] == '\n';
    __syncthreads();
    if (threadIdx.x < 64)
    {
        const uint32_t v = lane < kMatchRuns ? (uint32_t)__popcll(s_nl[lane]) : 0;
        const uint32_t inc = wave_incl_scan_u32(v);
        if (lane < kMatchRuns) s_pre[lane] = inc - v;
        if (lane == kMatchRuns - 1) s_pre[kMatchRuns] = inc;
    }
    __syncthreads();
    const uint32_t nloc = s_pre[kMatchRuns] + 1;         // reads with a position in the tile
    for (uint32_t i = threadIdx.x; i < nloc; i += kTB)
    {
        s_win[i] = 0;
        s_hit[i] = ANY && i == 0 ? __atomic_load_n(&hits[read0], __ATOMIC_RELAXED) : 0;
    }
    __syncthreads();

    const uint64_t lmask = (1ULL << L) - 1;              // (L <= 63)
    uint32_t unann = 0;                                  // TAX: this wave's hits at ranks without a class
    for (uint32_t it = 0; it < kMatchRuns / kWaves; ++it)
    {
        const uint32_t run = wave_id() * (kMatchRuns / kWaves) + it;
        const uint32_t q = run * 64 + lane;
        const uint64_t p = t0 + q;
        const uint64_t nlw = s_nl[run];
        const uint64_t below = nlw & ((1ULL << lane) - 1), rest = nlw >> lane;
        const uint32_t local = s_pre[run] + (uint32_t)__popcll(below);
        // the lanes of this lane's read inside the run: after the last newline below, up to the next newline
        const uint32_t first = below ? 64u - (uint32_t)__clzll((long long)below) : 0u;
        const uint32_t last = rest ? lane + (uint32_t)__ffsll((long long)rest) - 1u : 63u;
        const uint64_t seg = (~0ULL >> (63u - last)) & (~0ULL << first);

        if (starts && p < nbytes)
        {
            const bool begins = lane ? ((nlw >> (lane - 1)) & 1) : run ? (s_nl[run - 1] >> 63) : (t0 == 0 || s_prev_nl);
            if (begins) starts[read0 + local] = p;
        }

        const bool valid = tile_window_valid(s_inv, run, lane, lmask);
        const uint64_t vb = __ballot(valid);
        if (!vb) continue;

        bool done = ANY && __atomic_load_n(&s_hit[local], __ATOMIC_RELAXED) != 0;
        uint64_t hb = 0;
        uint32_t cls = 0;                                // CLS, TAX: the class of this lane's hit
        unsigned long long cw = 0;                       // COL: the word of this lane's hit
#pragma unroll
        for (uint32_t ph = 0; ph < (ANY ? 2u : 1u); ++ph)
        {
            const bool go = valid && !done && (!ANY || ((lane & 7u) == 0) == (ph == 0));
            bool hit = false;
            if (go)
            {
                K x, rc;
                tile_window_keys<K>(s_codes, q, L, &x, &rc);
                if (flags & kMatchNormalize) x = canonical(x, rc);
                uint64_t r;
                if (!rd_sparse_access_rank<K>(o.s, x, &r, &hit)) { q_fail(bad, p, kQBadWalk); hit = false; }
                if (CLS && hit)
                {
                    if (r >= o.s.count) { q_fail(bad, p, kQBadWalk); hit = false; }      // (the bitmaps end at count)
                    else cls = (uint32_t)((lhs[r >> 6] >> (r & 63)) & 1) << 1 | (uint32_t)((rhs[r >> 6] >> (r & 63)) & 1);
                }
                if (COL && hit)
                {
                    if (r >= o.s.count) { q_fail(bad, p, kQBadWalk); hit = false; }      // (colours[] ends at count)
                    else cw = aux.colours[r];
                }
                if ((ANN || TAX) && hit)
                {
                    if (r >= o.s.count) { q_fail(bad, p, kQBadWalk); hit = false; }      // (ann[] ends at count)
                    else if (ANN) taxo_lca_into(&tx.ann[r], tx.parent, tx.last, tx.read_class[read0 + local]);
                    else cls = __atomic_load_n(&tx.ann[r], __ATOMIC_RELAXED);
                }
            }
            const uint64_t b = __ballot(hit);
            hb |= b;
            if (ANY) done = done || (b & seg) != 0;
        }

        uint32_t mask = 0;
        if (CLS && hb)
        {
            const bool hit = (hb >> lane) & 1;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (__ballot(hit && cls == j) & seg) mask |= 1u << j;
        }
        if constexpr (COL)
        {
            if (hb)
            {
                // every lane learns the word of the first hit lane of its read; a wave none of whose hit lanes differs
                // from that sends one word per read
                const uint64_t mine = hb & seg;
                const uint32_t lead = mine ? (uint32_t)__ffsll((long long)mine) - 1u : lane;
                const unsigned long long c0 = __shfl(cw, (int)lead, 64);
                if (!__ballot(((hb >> lane) & 1) && cw != c0))
                {
                    if (lane == lead && mine && c0) atomicOr(&s_hit[local], c0);
                }
                else
                {
                    // an inclusive OR scan up the lanes, cut at each read's first lane (a lane without a hit holds 0)
                    unsigned long long v = cw;
#pragma unroll
                    for (uint32_t d = 1; d < 64; d <<= 1)
                    {
                        const unsigned long long u = __shfl_up(v, d, 64);
                        if (lane >= first + d) v |= u;
                    }
                    if (lane == last && v) atomicOr(&s_hit[local], v);
                }
            }
        }
        if constexpr (TAX) if (hb)
        {
            const bool hit = (hb >> lane) & 1;
            unann += (uint32_t)__popcll(__ballot(hit && cls == 0));
            const uint64_t cb = __ballot(hit && cls != 0);                   // the lanes that bring a class
            if (cb)
            {
                // every lane learns the class of the first such lane of its read; a read whose lanes all agree sends one
                const uint64_t mine = cb & seg;
                const uint32_t lead = mine ? (uint32_t)__ffsll((long long)mine) - 1u : lane;
                const uint32_t c0 = (uint32_t)__shfl((int)cls, (int)lead, 64);
                const bool differs = hit && cls != 0 && cls != c0;
                const bool mixed = (__ballot(differs) & seg) != 0;
                if (mine && (mixed ? hit && cls != 0 : lane == lead)) taxo_combine_into(&s_hit[local], tx.last, cls);
            }
        }
        if (lane == first)
        {
            const uint32_t nw = (uint32_t)__popcll(vb & seg), nh = (uint32_t)__popcll(hb & seg);
            if (nw) atomicAdd(&s_win[local], nw);
            if constexpr (CLS) { if (mask) atomicOr(&s_hit[local], mask); }
            else if constexpr (!TAX && !COL) { if (nh) atomicAdd(&s_hit[local], nh); }
        }
    }
    __syncthreads();
    if (TAX && lane == 0 && unann) atomicAdd(tx.unann, (unsigned long long)unann);      // (a ballot's count: the same in every lane)

    for (uint32_t i = threadIdx.x; i < nloc; i += kTB)
    {
        const uint32_t nw = s_win[i];
        const HitWord nh = s_hit[i];
        if (nw)
        {
            const uint32_t old = atomicAdd(&windows[read0 + i], nw);
            if ((uint64_t)old + nw >= 0xFFFFFFFFULL) atomicMin(&bad[1], (unsigned long long)(read0 + i));
        }
        if (nh)
        {
            if constexpr (ANY) atomicOr(&hits[read0 + i], 1u);
            else if constexpr (CLS) atomicOr(&hits[read0 + i], nh);
            else if constexpr (TAX) taxo_combine_into(&hits[read0 + i], tx.last, nh);
            else if constexpr (COL) atomicOr(reinterpret_cast<unsigned long long*>(hits) + read0 + i, nh);
            else atomicAdd(&hits[read0 + i], nh);
        }
    }
}

}  // namespace goss
