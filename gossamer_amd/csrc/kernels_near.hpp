// kernels_near.hpp -- compute-near-kmers (GossCmdComputeNearKmers.cc:58-121): the gray set of a k-mer set that carries
// a left and a right membership bit per k-mer.  A k-mer that belongs to one side only is gray when one of its
// neighbours -- its key with a mask flipped -- is in the set and belongs to the other side only; a gray k-mer loses
// both bits, every other k-mer keeps its own.
//
// One wave takes 64 consecutive words of each bitmap, one per lane: 4096 ranks.  The candidates of a word are the set
// bits of lhs ^ rhs; a scan over the lanes numbers the chunk's candidates, and the wave works through them 64 at a time,
// so every lane has a candidate however few of the ranks are candidates.  Each lane finds its candidate's word and bit
// from the per-word counts in LDS, selects its key once, and the wave walks the distinct masks in a wave-uniform loop:
// every lane that still looks does one accessAndRank of its flipped key and, on a hit, reads the two OLD bits of the
// rank it found.  A lane that has found its neighbour stops; the loop ends when a ballot says nobody looks any more.
// Gray lanes set their bit in the wave's gray words in LDS; at the end of the chunk every lane stores its own word of
// each output with the gray bits cleared: no atomics on the bitmaps in global memory, no order between waves.  The
// output arrays are not the input arrays, so no wave ever reads a bit that this launch has cleared (in a chain
// left - right - left all three are gray).
//
// The masks (b = 1..3, j = 0..K-1):
//   as the reference shifts them   b << j: the K + 1 single bits 0..K and the K pairs 3 << j (2 << j == 1 << (j + 1))
//   kNearWholeBases                b << 2j: 3K masks, one substitution of one base each
// The flipped key is looked up as it is; with kNearNormalize it is mapped to its canonical form first (q_key).
//
// A lane whose index walk cannot answer (a damaged image) reports its rank through *bad as the query kernels do
// (q_fail) and clears nothing; the entry point then fails the call.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "goss_reader.hpp"
#include "kernels_common.hpp"
#include "kernels_query.hpp"

namespace goss {

enum : uint32_t { kNearWholeBases = 1, kNearNormalize = 2 };

// x ^ (bits << pos), bits < 4, pos + 1 < 64 * words
__device__ inline Key1 near_flip(const Key1& x, uint32_t pos, uint64_t bits) { return Key1{x.lo ^ (bits << pos)}; }
__device__ inline Key2 near_flip(const Key2& x, uint32_t pos, uint64_t bits)
{
    if (pos >= 64) return Key2{x.lo, x.hi ^ (bits << (pos - 64))};
    return Key2{x.lo ^ (bits << pos), pos == 63 ? x.hi ^ (bits >> 1) : x.hi};
}

// position of the k-th (from 0) set bit of x, k < popcount(x)
__device__ inline uint32_t near_select_bit(uint64_t x, uint32_t k)
{
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t width = 32; width; width >>= 1)
    {
        const uint32_t c = (uint32_t)__popcll(x & ((1ULL << width) - 1));
        if (k >= c) { k -= c; x >>= width; pos += width; }
    }
    return pos;
}

template <class K>
__global__ __launch_bounds__(256) void near_kmers_kernel(QueryObj o, const uint64_t* __restrict__ lhs, const uint64_t* __restrict__ rhs,
                                                         uint32_t flags, uint64_t* __restrict__ lhs_out, uint64_t* __restrict__ rhs_out,
                                                         unsigned long long* __restrict__ gray, unsigned long long* bad)
{
    // per wave: the chunk's lhs words, candidate words and gray words, and the candidates before each word
    __shared__ unsigned long long s_lhs[4][64], s_cand[4][64], s_gray[4][64];
    __shared__ uint32_t s_before[4][64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u, len = o.len;
    lds_vu64 sl = (lds_vu64)s_lhs[wv], sc = (lds_vu64)s_cand[wv], sg = (lds_vu64)s_gray[wv];
    lds_vu32 sb = (lds_vu32)s_before[wv];
    const uint64_t count = o.s.count, nwords = (count + 63) >> 6, nchunks = (nwords + 63) >> 6;
    const uint32_t nmasks = (flags & kNearWholeBases) ? 3 * len : 2 * len + 1;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    unsigned long long total = 0;
    for (uint64_t chunk = (uint64_t)blockIdx.x * 4 + wv; chunk < nchunks; chunk += waves)
    {
        const uint64_t w = chunk * 64 + lane;
        uint64_t lw = 0, rw = 0;
        if (w < nwords)
        {
            const uint64_t valid = (w == nwords - 1 && (count & 63)) ? (1ULL << (count & 63)) - 1 : ~0ULL;
            lw = lhs[w] & valid;
            rw = rhs[w] & valid;
        }
        const uint64_t cand = lw ^ rw;
        const uint32_t mine_n = (uint32_t)__popcll(cand), upto = wave_incl_scan(mine_n);
        const uint32_t ncand = (uint32_t)__shfl((int)upto, 63, 64);
        __builtin_amdgcn_wave_barrier();                             // (the last pass has read its words)
        sl[lane] = lw; sc[lane] = cand; sg[lane] = 0; sb[lane] = upto - mine_n;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t c0 = 0; c0 < ncand; c0 += 64)                  // (wave-uniform)
        {
            const uint32_t c = c0 + lane;
            bool look = c < ncand, found = false;
            uint32_t j = 0, b = 0;
            uint64_t i = 0, mine = 0;
            K x{};
            if (look)
            {
                // the last word with at most c candidates before it holds candidate c
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if (sb[j + step] <= c) j += step;
                b = near_select_bit(sc[j], c - sb[j]);
                i = (chunk * 64 + j) * 64 + b;
                mine = (sl[j] >> b) & 1;
                if (!rd_sparse_select<K>(o.s, i, &x)) { q_fail(bad, i, kQBadWalk); look = false; }
            }
            for (uint32_t t = 0; t < nmasks; ++t)
            {
                uint32_t pos;
                uint64_t bits;
                if (flags & kNearWholeBases) { pos = 2 * (t / 3); bits = t % 3 + 1; }
                else if (t <= len) { pos = t; bits = 1; }
                else { pos = t - len - 1; bits = 3; }
                if (look)
                {
                    K y = near_flip(x, pos, bits);
                    uint64_t r;
                    bool p = false;
                    // (a flipped key lies below 4^K: q_key's range check never fires for an intact set)
                    if (q_key(o, y, (flags & kNearNormalize) ? kQueryNormalize : 0))
                    {
                        if (!rd_sparse_access_rank<K>(o.s, y, &r, &p)) { q_fail(bad, i, kQBadWalk); look = false; p = false; }
                    }
                    if (p)
                    {
                        const uint64_t lr = (lhs[r >> 6] >> (r & 63)) & 1, rr = (rhs[r >> 6] >> (r & 63)) & 1;
                        if (lr != rr && lr != mine) { found = true; look = false; }
                    }
                }
                if (!__ballot(look)) break;
            }
            if (found) atomicOr(&s_gray[wv][j], 1ULL << b);
        }
        __builtin_amdgcn_wave_barrier();
        const uint64_t g = sg[lane];
        if (w < nwords)
        {
            lhs_out[w] = lw & ~g;
            rhs_out[w] = rw & ~g;
        }
        total += (unsigned long long)__popcll(g);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d, 64);
    if (lane == 0 && total) atomicAdd(gray, total);
}

}  // namespace goss
