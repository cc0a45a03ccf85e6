/* goss_gpu_near.h -- compute-near-kmers against a KmerSet resident in HBM; part of the C ABI of libgossgpu.so,
 * included by goss_gpu.h (which declares goss_gpu_object and the status codes) and not meant to be included alone. */
#ifndef GOSS_GPU_NEAR_H
#define GOSS_GPU_NEAR_H

/*
 * compute-near-kmers (GossCmdComputeNearKmers.cc:58-121): the gray set of a KmerSet that carries a left and a right
 * membership bit per k-mer (the .lhs-bits / .rhs-bits of merge-and-annotate-kmer-sets, goss_gpu_emit_count_bits).
 * Per rank i with lhs[i] != rhs[i]: x = select(i); for j = 0 .. K-1 and b = 1 .. 3, y = x ^ mask(b, j); i is gray when
 * some y is in the set at a rank r with lhs[r] != rhs[r] and lhs[r] != lhs[i] -- a neighbour that belongs to the other
 * side only.  A gray rank gets both new bits 0; every other rank keeps its bits (ranks with both bits or neither
 * included).  Only OLD bits are read: in a chain left - right - left all three are gray.
 *
 * With flags = 0 the result is the reference's, bit for bit, which means two things that read like defects there:
 *   - its mask is b << j, a shift by j BITS: the masks touch bits 0 .. K only (the last (K + 1) / 2 bases, rounded
 *     up), and for odd j the two bits straddle two bases (:79-80);
 *   - it calls mKmerSet.normalize(y), which returns the canonical form by value (GraphEssentials.hh:152-157), throws
 *     the result away and looks y up as it is (:93-95): a neighbour counts only if x ^ mask is itself the stored form.
 * The two files are what `xenome classify` reads, so an index finished here must equal one finished there.  The two
 * flags give what was probably meant and are the two departures from the reference; `goss compute-near-kmers` sets
 * neither:
 *   GOSS_NEAR_WHOLE_BASES  masks b << 2j: every substitution of one base (all below bit 2K, so y is always a valid key)
 *   GOSS_NEAR_NORMALIZE    y is mapped to its canonical form (position_type::normalize, RankSelect.hh:126-140)
 *                          before the lookup
 *
 * Only a GOSS_OBJECT_KMER_SET is accepted (any other kind: GOSS_ERR_INVALID_ARG).  d_lhs, d_rhs, d_lhs_out and
 * d_rhs_out are (count + 63) / 64 words each on the object's device, in WordyBitVector layout (bit i of the array is
 * bit i % 64 of word i / 64); the bits at and past count of the last output word are 0 whatever the input holds there.
 * An output that overlaps an input or the other output is GOSS_ERR_INVALID_ARG and nothing is written.  *gray (host)
 * receives the number of gray ranks.  The call is synchronous on the object's stream; an empty set does nothing and
 * reports 0.  An index walk that cannot answer (a damaged image) fails the call with GOSS_ERR_INVALID_ARG, and
 * goss_gpu_object_last_error names the lowest such rank; the outputs are then undefined.
 * goss_gpu_object_near_kmers_host: the same with the four bitmaps in host memory, staged through the device; there an
 * output may be the input it replaces.
 */
enum { GOSS_NEAR_WHOLE_BASES = 1, GOSS_NEAR_NORMALIZE = 2 };
int goss_gpu_object_near_kmers(goss_gpu_object* obj, const uint64_t* d_lhs, const uint64_t* d_rhs, uint32_t flags,
                               uint64_t* d_lhs_out, uint64_t* d_rhs_out, uint64_t* gray /* host */);
int goss_gpu_object_near_kmers_host(goss_gpu_object* obj, const uint64_t* lhs, const uint64_t* rhs, uint32_t flags,
                                    uint64_t* lhs_out, uint64_t* rhs_out, uint64_t* gray);

#endif /* GOSS_GPU_NEAR_H */
