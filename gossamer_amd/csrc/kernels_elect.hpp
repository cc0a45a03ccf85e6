// kernels_elect.hpp -- what goss_gpu_object_colour_reads needs beside the pass over the reads (kernels_match.hpp,
// kModeColour): the colour words of a KmerSet made from a pool's index, and the reads counted by the bits of their word.
//
// elect_colours_from_index_kernel: the index of pool-samples is a SparseArray over S * z positions that holds i * z + r
// for every k-mer of sample i at rank r of the union of z k-mers.  One lane per stored position, grid-stride: the
// position comes from the device select the queries use (rd_sparse_select), and 1 << (p / z) is ORed into
// colours[p % z] with one vector atomic.  OR is order-free: the array is the same bytes on every run.  A position the
// walk cannot give, or one at or past S * z (S <= 64), leaves the lowest such index in *bad (q_fail) and writes nothing.
//
// elect_sums_kernel: popcount(words[i]) counted into out[0..64]: an LDS histogram per block, one global add per
// non-zero bin, as classify_sums_kernel counts the masks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "goss_reader.hpp"
#include "kernels_query.hpp"

namespace goss {

__global__ __launch_bounds__(256) void elect_colours_from_index_kernel(RdSparse idx, uint64_t z, uint32_t S, unsigned long long* __restrict__ colours,
                                                                       unsigned long long* bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < idx.count; i += (uint64_t)gridDim.x * blockDim.x)
    {
        Key1 p;
        if (!rd_sparse_select<Key1>(idx, i, &p)) { q_fail(bad, i, kQBadWalk); continue; }
        const uint64_t s = p.lo / z;
        if (s >= S) { q_fail(bad, i, kQBadKey); continue; }         // (at or past the universe S * z: a damaged image)
        atomicOr(&colours[p.lo % z], 1ULL << s);
    }
}

__global__ __launch_bounds__(256) void elect_sums_kernel(const uint64_t* __restrict__ words, uint64_t reads, unsigned long long* __restrict__ out)
{
    __shared__ uint32_t s_bin[65];
    if (threadIdx.x < 65) s_bin[threadIdx.x] = 0;
    __syncthreads();
    // (32-bit bins: as classify_sums_kernel)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < reads; i += (uint64_t)gridDim.x * blockDim.x)
        atomicAdd(&s_bin[__popcll(words[i])], 1u);
    __syncthreads();
    if (threadIdx.x < 65 && s_bin[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)s_bin[threadIdx.x]);
}

}  // namespace goss
