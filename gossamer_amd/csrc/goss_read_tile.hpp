// goss_read_tile.hpp -- one tile of read bytes staged in LDS, and the window that starts at a position of it.  Shared by
// match_reads_kernel (kernels_match.hpp), components_mark_kernel (kernels_components.hpp) and links_windows_kernel
// (kernels_links.hpp).
//
// A tile is kMatchTile byte positions, one workgroup each.  Every lane turns 8 bytes into 16 bits of 2-bit codes, 8
// non-base flags and, where asked for, 8 newline flags (base_codes: the extraction kernels' decoder) and stores them
// into LDS bit arrays that the kernel declares: the tile's positions plus a halo of 64 (>= L - 1).  The window that
// starts at a position is then a funnel shift of two or three LDS words, valid when L flag bits are clear (a '\n' is a
// non-base, so a valid window lies inside one read).  Stored with the first base in the LOW bits, the shifted words are
// the window's reverse complement once inverted (GossReadBaseString.hh:133-188 wants the first base on top).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "goss_key.hpp"
#include "kernels_common.hpp"

namespace goss {

constexpr uint32_t kMatchTile = 2048;                    // positions per workgroup: 256 lanes x 8 bytes
constexpr uint32_t kMatchRuns = kMatchTile / 64;         // runs of 64 positions, 8 per wave
constexpr uint32_t kMatchGroups = kMatchTile / 8 + 8;    // 8-byte groups staged: the tile and a halo of 64 positions

// 0x80 in every byte of w that is '\n'
__device__ __forceinline__ uint32_t newline_flags(uint32_t w)
{
    const uint32_t v = w ^ 0x0A0A0A0Au;
    return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
}

// bytes [pos, pos + 8) of the input, 0 (no base, no newline) at and beyond nbytes
__device__ __forceinline__ uint64_t match_load8(const uint8_t* __restrict__ bases, uint64_t nbytes, uint64_t pos, bool aligned)
{
    if (aligned && pos + 8 <= nbytes) return *reinterpret_cast<const uint64_t*>(bases + pos);
    uint64_t w = 0;
    for (uint32_t j = 0; j < 8; ++j)
        if (pos + j < nbytes) w |= (uint64_t)bases[pos + j] << (8 * j);
    return w;
}

// the window of L bases whose first base is `v` bit 0..1 (2-bit codes, first base lowest): its key and, for
// normalising, the key of its reverse complement
template <class K> __device__ __forceinline__ void match_keys(uint64_t v0, uint64_t v1, uint32_t L, K* fwd, K* rc);
template <> __device__ __forceinline__ void match_keys<Key1>(uint64_t v0, uint64_t, uint32_t L, Key1* fwd, Key1* rc)
{
    *rc = Key1{~v0 & ((1ULL << (2 * L)) - 1)};
    *fwd = Key1{rev64(v0) >> (64 - 2 * L)};
}
template <> __device__ __forceinline__ void match_keys<Key2>(uint64_t v0, uint64_t v1, uint32_t L, Key2* fwd, Key2* rc)
{
    *rc = Key2{~v0, ~v1 & ((1ULL << (2 * L - 64)) - 1)};               // (32 <= L <= 63)
    *fwd = revcomp(*rc, L);
}

// The tile at byte t0 staged by the whole workgroup: group g = 8 bytes -> 16 bits of codes in s_codes[kMatchGroups / 4]
// (32 bases per word, first base lowest), 8 flags in s_inv[kMatchGroups / 8] (bit = not one of ACGTacgt, or beyond the
// input) and, with NL, 8 flags in s_nl[kMatchRuns] (bit = '\n'; the tile only, no halo).  The caller synchronises.
template <bool NL>
__device__ __forceinline__ void tile_stage(const uint8_t* __restrict__ bases, uint64_t nbytes, uint64_t t0, uint32_t aligned,
                                           uint64_t* s_codes, uint64_t* s_inv, uint64_t* s_nl)
{
    for (uint32_t g = threadIdx.x; g < kMatchGroups; g += kTB)
    {
        const uint64_t w = match_load8(bases, nbytes, t0 + 8ULL * g, aligned);
        uint32_t bad0, bad1;
        const uint32_t x0 = base_codes((uint32_t)w, bad0), x1 = base_codes((uint32_t)(w >> 32), bad1);
        reinterpret_cast<uint16_t*>(s_codes)[g] = (uint16_t)(pack_codes(x0) | (pack_codes(x1) << 8));
        reinterpret_cast<uint8_t*>(s_inv)[g] = (uint8_t)(pack_flags(bad0) | (pack_flags(bad1) << 4));
        if (NL && g < kMatchTile / 8)
            reinterpret_cast<uint8_t*>(s_nl)[g] = (uint8_t)(pack_flags(newline_flags((uint32_t)w)) | (pack_flags(newline_flags((uint32_t)(w >> 32))) << 4));
    }
}

// whether the window of L bases that starts at position run * 64 + lane of the tile holds bases only; lmask: L low bits
// set (L <= 63), which the kernel computes once
__device__ __forceinline__ bool tile_window_valid(const uint64_t* s_inv, uint32_t run, uint32_t lane, uint64_t lmask)
{
    const uint64_t iv = (s_inv[run] >> lane) | (lane ? s_inv[run + 1] << (64 - lane) : 0);
    return (iv & lmask) == 0;
}

// the key of the window of L bases that starts at position q of the tile, and of its reverse complement
template <class K>
__device__ __forceinline__ void tile_window_keys(const uint64_t* s_codes, uint32_t q, uint32_t L, K* fwd, K* rc)
{
    const uint32_t cw = q >> 5, co = 2 * (q & 31);
    const uint64_t c0 = s_codes[cw], c1 = s_codes[cw + 1];
    const uint64_t v0 = co ? (c0 >> co) | (c1 << (64 - co)) : c0;
    uint64_t v1 = 0;
    if (K::kWords == 2)
    {
        const uint64_t c2 = s_codes[cw + 2];
        v1 = co ? (c1 >> co) | (c2 << (64 - co)) : c1;
    }
    match_keys<K>(v0, v1, L, fwd, rc);
}

}  // namespace goss
