// kernels_pool.hpp -- pool-samples: the sample x k-mer membership of S samples over a union of z k-mers as a bit
// matrix of S rows of W = ceil(z / 64) u64 words (row i word w bit b: k-mer 64 w + b is in sample i), the common
// k-mers of every pair of samples as popcount(row_i & row_j) summed along the rows, and the rows as the positions
// i * z + r of the reference's index (GossCmdPoolSamples.cc).  Integer adds only: exact whatever the scheduling.
#pragma once

#include "kernels_common.hpp"

namespace goss {

// ---- masks -> bit rows ---------------------------------------------------------------------------------------------
// A wave takes kPoolRowsWords consecutive words: 64 masks per word, one per lane; the ballot of bit i over the wave IS
// word w of row first + i, and lane i keeps it.  After kPoolRowsWords words lane i holds 64 consecutive bytes of its
// row and stores them word by word (a cache line per lane).  Masks at or beyond z read as 0, so the bits of the last
// word beyond z are 0 in every row.  The popcount of every row (the sample's size) is added up on the way, over all the
// groups a wave takes (the grid has a workgroup per kWaves * kPoolRowsTurns groups, and its waves stride over them), and
// leaves as one 64-bit atomic per row and wave -- one per row and GROUP kept 2 * 10^5 atomics on each of 32 words waiting
// for each other at z = 10^8, and the kernel ten times over its memory time.
constexpr int kPoolRowsWords = 8;
constexpr int kPoolRowsTurns = 32;                                // groups of a wave

__global__ __launch_bounds__(kTB) void pool_rows_kernel(const uint32_t* __restrict__ masks, uint64_t z, uint64_t W, uint32_t first,
                                                        uint32_t nbits, unsigned long long* __restrict__ rows,
                                                        unsigned long long* __restrict__ sizes)
{
    const uint32_t lane = lane_id();
    const uint64_t ngroups = (W + kPoolRowsWords - 1) / kPoolRowsWords;
    unsigned long long ones = 0;
    // (whole waves take a group or leave: the ballots below see full waves)
    for (uint64_t grp = (uint64_t)blockIdx.x * kWaves + wave_id(); grp < ngroups; grp += (uint64_t)gridDim.x * kWaves)
    {
        const uint64_t w0 = grp * kPoolRowsWords;
        unsigned long long keep[kPoolRowsWords];
#pragma unroll
        for (int j = 0; j < kPoolRowsWords; ++j)
        {
            const uint64_t idx = (w0 + j) * 64 + lane;
            const uint32_t m = idx < z ? masks[idx] : 0u;
            unsigned long long mine = 0;
            for (uint32_t i = 0; i < nbits; ++i)
            {
                const unsigned long long b = __ballot((m >> i) & 1u);
                if (lane == i) mine = b;
            }
            keep[j] = mine;
            ones += (unsigned long long)__popcll(mine);
        }
        if (lane < nbits)
        {
            unsigned long long* row = rows + (uint64_t)(first + lane) * W;
#pragma unroll
            for (int j = 0; j < kPoolRowsWords; ++j)
                if (w0 + j < W) row[w0 + j] = keep[j];
        }
    }
    if (lane < nbits && ones) atomicAdd(sizes + first + lane, ones);
}

// ---- rows -> pair counts -------------------------------------------------------------------------------------------
// inter[i][j] = sum over w of popcount(row_i[w] & row_j[w]) for i <= j.  A workgroup takes a tile of kPoolTile rows i
// x kPoolTile rows j (tile_i <= tile_j only) and every kPoolPairWords-word block of the rows that falls to it
// (blockIdx.y, then on by gridDim.y).  It stages the two row pieces in LDS kPoolStage words at a time, word-major
// ([word][row], a row of kPoolTile + 2 u64 so that 16-byte reads stay aligned): a thread owns a 4 x 4 patch of the tile,
// reads its four i-words and four j-words of a staged word as two 32-byte reads each (the j reads of a wave are 512
// consecutive bytes, the i reads four broadcasts) and does sixteen AND + popcount + add into registers.  The counts of
// a workgroup fit 32 bits while it visits fewer than 2^26 words, which the launch guarantees; at its end one 64-bit
// atomicAdd per pair.  Rows at or beyond S and words at or beyond W are staged as zeros.
constexpr int kPoolTile = 64;
constexpr int kPoolPatch = 4;
constexpr int kPoolStage = 32;                                   // words of every row staged at a time
constexpr int kPoolPairWords = 128;                              // words of a row per visit of a workgroup
constexpr int kPoolLdsRow = kPoolTile + 2;
static_assert(kPoolTile == kPoolPatch * 16 && kTB == 16 * 16, "a thread per 4 x 4 patch");
static_assert(kPoolPairWords % kPoolStage == 0, "whole stages");

__global__ __launch_bounds__(kTB) void pool_pairs_kernel(const unsigned long long* __restrict__ rows, uint32_t S, uint64_t W,
                                                         uint32_t ntiles, unsigned long long* __restrict__ inter)
{
    __shared__ __attribute__((aligned(16))) unsigned long long sa[kPoolStage * kPoolLdsRow];
    __shared__ __attribute__((aligned(16))) unsigned long long sb[kPoolStage * kPoolLdsRow];
    // tile pair number -> (ti <= tj), row-major over the upper triangle
    uint32_t ti = 0, rest = blockIdx.x;
    while (rest >= ntiles - ti) { rest -= ntiles - ti; ++ti; }
    const uint32_t tj = ti + rest;
    const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15u;
    uint32_t acc[kPoolPatch][kPoolPatch];
#pragma unroll
    for (int a = 0; a < kPoolPatch; ++a)
#pragma unroll
        for (int b = 0; b < kPoolPatch; ++b) acc[a][b] = 0;
    const uint64_t nblocks = (W + kPoolPairWords - 1) / kPoolPairWords;
    for (uint64_t blk = blockIdx.y; blk < nblocks; blk += gridDim.y)
    {
        for (int st = 0; st < kPoolPairWords / kPoolStage; ++st)
        {
            const uint64_t wbase = blk * kPoolPairWords + (uint64_t)st * kPoolStage;
            if (wbase >= W) break;                              // (uniform over the workgroup)
            // stage: consecutive lanes read consecutive words of one row
            for (uint32_t e = threadIdx.x; e < (uint32_t)(kPoolTile * kPoolStage); e += kTB)
            {
                const uint32_t r = e / kPoolStage, w = e % kPoolStage;
                const uint64_t gw = wbase + w;
                const uint32_t ri = ti * kPoolTile + r, rj = tj * kPoolTile + r;
                sa[w * kPoolLdsRow + r] = (ri < S && gw < W) ? rows[(uint64_t)ri * W + gw] : 0ULL;
                sb[w * kPoolLdsRow + r] = (rj < S && gw < W) ? rows[(uint64_t)rj * W + gw] : 0ULL;
            }
            __syncthreads();
#pragma unroll 4
            for (int w = 0; w < kPoolStage; ++w)
            {
                unsigned long long va[kPoolPatch], vb[kPoolPatch];
#pragma unroll
                for (int a = 0; a < kPoolPatch; ++a) va[a] = sa[w * kPoolLdsRow + ty * kPoolPatch + a];
#pragma unroll
                for (int b = 0; b < kPoolPatch; ++b) vb[b] = sb[w * kPoolLdsRow + tx * kPoolPatch + b];
#pragma unroll
                for (int a = 0; a < kPoolPatch; ++a)
#pragma unroll
                    for (int b = 0; b < kPoolPatch; ++b) acc[a][b] += (uint32_t)__popcll(va[a] & vb[b]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int a = 0; a < kPoolPatch; ++a)
#pragma unroll
        for (int b = 0; b < kPoolPatch; ++b)
        {
            const uint32_t i = ti * kPoolTile + ty * kPoolPatch + a, j = tj * kPoolTile + tx * kPoolPatch + b;
            if (i <= j && j < S && acc[a][b]) atomicAdd(inter + (uint64_t)i * S + j, (unsigned long long)acc[a][b]);
        }
}

// ---- rows -> the index's positions ---------------------------------------------------------------------------------
// Unit u = row * nblk + b is the b-th kPoolPosWords-word block of a row (a thread per word).  pool_ones_kernel counts
// the unit's set bits; scanned over all units in that order the counts are where every unit's positions begin in the
// one sample-major array; pool_positions_kernel scans the words' popcounts inside the unit and every thread writes
// row * z + 64 w + b for the set bits b of its word, in increasing order.
constexpr int kPoolPosWords = 128;

__global__ __launch_bounds__(kPoolPosWords) void pool_ones_kernel(const unsigned long long* __restrict__ rows, uint64_t W, uint64_t nblk,
                                                                  uint64_t nunits, unsigned long long* __restrict__ ones)
{
    __shared__ uint32_t sh[kPoolPosWords / 64 + 1];
    const uint64_t u = unit_block();
    if (u >= nunits) return;
    const uint64_t row = u / nblk, w = (u % nblk) * kPoolPosWords + threadIdx.x;
    const uint32_t c = w < W ? (uint32_t)__popcll(rows[row * W + w]) : 0u;
    uint32_t total;
    (void)block_excl_scan_n<uint32_t, kPoolPosWords / 64>(c, sh, &total);
    if (threadIdx.x == 0) ones[u] = total;
}

__global__ __launch_bounds__(kPoolPosWords) void pool_positions_kernel(const unsigned long long* __restrict__ rows, uint64_t z, uint64_t W,
                                                                       uint64_t nblk, uint64_t nunits,
                                                                       const unsigned long long* __restrict__ begin,
                                                                       unsigned long long* __restrict__ pos)
{
    __shared__ uint32_t sh[kPoolPosWords / 64 + 1];
    const uint64_t u = unit_block();
    if (u >= nunits) return;
    const uint64_t row = u / nblk, w = (u % nblk) * kPoolPosWords + threadIdx.x;
    unsigned long long bits = w < W ? rows[row * W + w] : 0ULL;
    uint32_t total;
    const uint32_t before = block_excl_scan_n<uint32_t, kPoolPosWords / 64>((uint32_t)__popcll(bits), sh, &total);
    unsigned long long* out = pos + begin[u] + before;
    const unsigned long long base = row * z + w * 64;           // (row * z + rank < S * z < 2^64: the host refuses the rest)
    while (bits)
    {
        const uint32_t b = (uint32_t)__ffsll((long long)bits) - 1u;
        *out++ = base + b;
        bits &= bits - 1;
    }
}

}  // namespace goss
