// pool_path.hpp -- pool-samples: the host passes over the bit rows of kernels_pool.hpp.
// Part of goss_gpu.hip (included there, inside its unnamed namespace, after graph_passes.hpp).  The rows and the
// samples' sizes are the context's held result (Held::Pool), from goss_gpu_pool_begin until goss_gpu_pool_release or
// any entry point that is not one of the pool's: bottom to top the rows (S * W u64, zeroed), the sizes (S u64), then
// from pool_top on what goss_gpu_pool_emit_index left -- the positions and the SparseArray's file images.
#pragma once

inline uint64_t pool_words(uint64_t z) { return (z + 63) / 64; }

void pool_begin(goss_gpu_ctx* c, uint32_t nsets, uint64_t z)
{
    ensure_arena(c);
    const uint64_t W = pool_words(z);
    // the rows must fit the budget as it is: S * W * 8 bytes, and no count of ours is near 2^64
    if (W > (~0ULL >> 4) / nsets) throw StatusError{GOSS_ERR_OOM, "pool_begin: the rows do not fit the HBM budget"};
    const uint64_t bytes = (uint64_t)nsets * W * 8;
    if (c->arena.avail() < bytes + (uint64_t)nsets * 8 + 1024 && !grow_arena(c, bytes + (uint64_t)nsets * 8 + 1024))
        throw StatusError{GOSS_ERR_OOM, "pool_begin: the rows do not fit the HBM budget"};
    c->held = {Held::Pool, c->arena.lo};
    c->pool_rows = (unsigned long long*)c->arena.perm(bytes);
    c->pool_sizes = (unsigned long long*)c->arena.perm((uint64_t)nsets * 8);
    c->pool_top = c->arena.lo;
    c->pool_sets = nsets; c->pool_z = z;
    c->pool_added.assign(nsets, false);
    HIP_TRY(hipMemsetAsync(c->pool_rows, 0, bytes, c->stream));
    HIP_TRY(hipMemsetAsync(c->pool_sizes, 0, (uint64_t)nsets * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
}

void pool_add_masks(goss_gpu_ctx* c, uint32_t first, uint32_t nbits, const uint32_t* d_masks)
{
    const uint64_t z = c->pool_z, W = pool_words(z);
    PhaseTimer t(c, GOSS_T_REDUCE, z);
    hipLaunchKernelGGL(pool_rows_kernel, dim3(grid_for(W, kWaves * kPoolRowsWords * kPoolRowsTurns)), dim3(kTB), 0, c->stream, d_masks, z, W, first, nbits,
                       c->pool_rows, c->pool_sizes);
    t.stop();
    sync_checked(c);                       // the masks are the caller's again (a merging context may be reset now)
    for (uint32_t i = 0; i < nbits; ++i) c->pool_added[first + i] = true;
}

void pool_sizes(goss_gpu_ctx* c, uint64_t* sizes)
{
    HIP_TRY(hipMemcpyAsync(sizes, c->pool_sizes, (uint64_t)c->pool_sets * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
}

void pool_intersections(goss_gpu_ctx* c, uint64_t* inter)
{
    const uint32_t S = c->pool_sets;
    const uint64_t W = pool_words(c->pool_z);
    ArenaScope scope(c->arena);
    unsigned long long* d = (unsigned long long*)c->arena.temp((uint64_t)S * S * 8);
    HIP_TRY(hipMemsetAsync(d, 0, (uint64_t)S * S * 8, c->stream));
    const uint32_t ntiles = (S + kPoolTile - 1) / kPoolTile;
    const uint64_t npairs = (uint64_t)ntiles * (ntiles + 1) / 2;
    if (npairs > 0x7FFFFFFFULL) throw StatusError{GOSS_ERR_INVALID_ARG, "pool_intersections: too many samples for one launch"};
    const uint64_t nblocks = (W + kPoolPairWords - 1) / kPoolPairWords;
    // enough workgroups to fill the device a few times over, few enough that the atomics at their ends do not count
    const uint64_t want = std::max<uint64_t>(1, 8192 / npairs);
    const uint32_t gy = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nblocks, want), 65535);
    // a workgroup's 32-bit counts: the bits of the words it visits
    if ((nblocks + gy - 1) / gy * kPoolPairWords >= (1ULL << 26))
        throw StatusError{GOSS_ERR_INVALID_ARG, "pool_intersections: rows too long for one launch"};
    PhaseTimer t(c, GOSS_T_REDUCE, npairs * W);
    hipLaunchKernelGGL(pool_pairs_kernel, dim3((uint32_t)npairs, gy), dim3(kTB), 0, c->stream, (const unsigned long long*)c->pool_rows, S, W,
                       ntiles, d);
    t.stop();
    HIP_TRY(hipMemcpyAsync(inter, d, (uint64_t)S * S * 8, hipMemcpyDeviceToHost, c->stream));
    sync_checked(c);
    for (uint32_t i = 0; i < S; ++i)
        for (uint32_t j = 0; j < i; ++j) inter[(uint64_t)i * S + j] = inter[(uint64_t)j * S + i];
}

void pool_emit_index(goss_gpu_ctx* c)
{
    const uint32_t S = c->pool_sets;
    const uint64_t z = c->pool_z, W = pool_words(z);
    c->build.files.clear();
    c->arena.lo = c->pool_top;             // an earlier index goes
    const uint64_t nblk = (W + kPoolPosWords - 1) / kPoolPosWords, nunits = nblk * S;
    if (nunits >= (1ULL << 36)) throw StatusError{GOSS_ERR_INVALID_ARG, "pool_emit_index: rows too long for one launch"};
    uint64_t m = 0;
    unsigned long long* pos = nullptr;
    {
        ArenaScope scope(c->arena);
        uint64_t* begin = (uint64_t*)c->arena.temp((nunits + 1) * 8);
        // (timed as GOSS_T_REDUCE, the SparseArray's images below as GOSS_T_EMIT: tools/pool_probe.py tells them apart)
        PhaseTimer t(c, GOSS_T_REDUCE, nunits * kPoolPosWords);
        hipLaunchKernelGGL(pool_ones_kernel, unit_grid(nunits), dim3(kPoolPosWords), 0, c->stream, (const unsigned long long*)c->pool_rows, W, nblk,
                           nunits, (unsigned long long*)begin);
        scan_with_total(c, begin, nunits, pinned_words(c));
        sync_checked(c);
        m = pinned_words(c)[0];
        pos = (unsigned long long*)c->arena.perm(std::max<uint64_t>(m * 8, 16));
        hipLaunchKernelGGL(pool_positions_kernel, unit_grid(nunits), dim3(kPoolPosWords), 0, c->stream, (const unsigned long long*)c->pool_rows, z, W,
                           nblk, nunits, (const unsigned long long*)begin, pos);
        t.stop();
        sync_checked(c);
    }
    // SparseArray::Builder(name, fac, N = z * S, M = m) ... end(N)  (GossCmdPoolSamples.cc)
    const uint64_t N = z * S;
    PhaseTimer t(c, GOSS_T_EMIT, m);
    emit_sparse_array<Key1>(c, (const Key1*)pos, m, N, 0, m, N, 0, "");
    t.stop();
    HIP_TRY(hipStreamSynchronize(c->stream));
}
