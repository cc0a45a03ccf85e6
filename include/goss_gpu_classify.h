/* goss_gpu_classify.h -- reads classified against an annotated KmerSet resident in HBM; part of the C ABI of
 * libgossgpu.so, included by goss_gpu.h (which declares goss_gpu_object and the status codes) and not meant to be
 * included alone. */
#ifndef GOSS_GPU_CLASSIFY_H
#define GOSS_GPU_CLASSIFY_H

/*
 * group-reads (GossCmdGroupReads.cc:381-485), the loop behind `xenome classify`: a KmerSet of count k-mers carries a
 * left and a right membership bit per k-mer (the .lhs-bits / .rhs-bits that merge-and-annotate-kmer-sets writes and
 * compute-near-kmers finishes; WordyBitVector layout, bit i of a bitmap is bit i % 64 of word i / 64, (count + 63) / 64
 * words each).  Every valid K-window of a read is normalised and looked up; a window present at rank r has the class
 * c = 2 * lhs[r] + rhs[r], and the read's mask is the OR of 1 << c over its windows:
 *   bit 0 "M"  a k-mer with neither bit (what compute-near-kmers leaves of a gray one)
 *   bit 1 "H"  right side only
 *   bit 2 "G"  left side only
 *   bit 3 "B"  both sides
 * A read none of whose windows is in the set has mask 0.  There is no early out: every valid window walks, the mask is
 * exact.
 *
 * goss_gpu_object_classify_reads takes the batch as goss_gpu_object_match_reads does and follows it in everything it
 * does not say otherwise: what a read and a window are, max_reads and GOSS_ERR_BUFFER (info->reads holds the need),
 * nbytes = 0, an input pointer of any alignment, the 2^32 - 1 window limit, a walk that cannot answer (the lowest byte
 * position is named and the call fails), synchronous on the object's stream, working memory that only grows, the same
 * input giving the same arrays.  d_classes[r] = the mask of read r (0 .. 15), d_windows[r] = its number of windows,
 * d_read_starts as there; each of the three may be NULL, and so may info.  info->counts[m] = the reads whose mask is
 * m, so their sum is info->reads; info->windows = the sum of the windows.
 *
 * d_lhs, d_rhs: the two bitmaps on the object's device.  Both NULL means the pair kept by
 * goss_gpu_object_classify_bits_host; with no pair kept that is GOSS_ERR_INVALID_ARG (goss_gpu_object_last_error says
 * so), except for an empty set, which has no bits to read.  One NULL and the other not is GOSS_ERR_INVALID_ARG.  Only a
 * GOSS_OBJECT_KMER_SET is accepted, and only the flag below (it must be given to get the reference's result; without
 * it the windows are looked up as they stand); anything else is GOSS_ERR_INVALID_ARG.  A NULL object returns -1.
 *
 * goss_gpu_object_classify_bits_host copies the two host bitmaps into device memory that the object keeps until it is
 * closed; a second call replaces the pair; an empty set accepts NULL.
 * goss_gpu_object_classify_reads_host: the same for a caller without device memory of its own (goss group-reads): the
 * kept pair, host pointers for the batch and the three arrays, staged as goss_gpu_object_match_reads_host stages them.
 */
enum { GOSS_CLASSIFY_NORMALIZE = 1 /* = GOSS_QUERY_NORMALIZE */ };
typedef struct {
    uint64_t reads;          /* reads in the input (what max_reads must hold) */
    uint64_t windows;        /* sum over the reads */
    uint64_t counts[16];     /* reads per mask */
    float ms;                /* HIP-event time of the kernels */
} goss_gpu_classify_info;
int goss_gpu_object_classify_reads(goss_gpu_object* obj, const void* d_bases, uint64_t nbytes, const uint64_t* d_lhs,
                                   const uint64_t* d_rhs, uint32_t flags, uint64_t max_reads, uint32_t* d_classes,
                                   uint32_t* d_windows, uint64_t* d_read_starts, goss_gpu_classify_info* info);
int goss_gpu_object_classify_bits_host(goss_gpu_object* obj, const uint64_t* lhs, const uint64_t* rhs);
int goss_gpu_object_classify_reads_host(goss_gpu_object* obj, const void* bases, uint64_t nbytes, uint32_t flags,
                                        uint64_t max_reads, uint32_t* classes, uint32_t* windows, uint64_t* read_starts,
                                        goss_gpu_classify_info* info);

#endif /* GOSS_GPU_CLASSIFY_H */
