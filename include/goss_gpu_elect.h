/* goss_gpu_elect.h -- reads against up to 64 references in one pass, over a KmerSet resident in HBM that carries one
 * colour word per k-mer; part of the C ABI of libgossgpu.so, included by goss_gpu.h (which declares goss_gpu_object and
 * the status codes) and not meant to be included alone. */
#ifndef GOSS_GPU_ELECT_H
#define GOSS_GPU_ELECT_H

/*
 * electus classify (ElectApp.cc:150-701), the loop of KmerFilter: every valid K-window of a read is normalised and
 * looked up in up to 64 k-mer sets, and the read's word is the OR of the membership masks of its windows.  Here the
 * sets are one KmerSet, their union, of count k-mers, which carries `colours`: one uint64_t per rank, bit i set when
 * reference i holds the k-mer at that rank.  The array lives in device memory that the object keeps until it is
 * closed, as it keeps the bitmaps of goss_gpu_object_classify_bits_host.
 *
 * goss_gpu_object_colours_host copies count words from the host; a second call replaces them; an empty set accepts
 * NULL.  ncolours must be 1 .. 64, and a word with a bit at or above ncolours is GOSS_ERR_INVALID_ARG
 * (goss_gpu_object_last_error names the lowest such rank); a refused call leaves what was kept as it was.
 *
 * goss_gpu_object_colours_from_index makes the words on the device from what pool-samples wrote: `index` is a
 * GOSS_OBJECT_SPARSE_ARRAY opened from a pool's <out>-index on the same device, `obj` the KmerSet opened from its
 * <out>-union.  The index holds the position i * z + r for every k-mer of sample i at rank r of the union, z = the
 * count of obj, so its universe N must be S * z with 1 <= S <= 64; anything else is GOSS_ERR_INVALID_ARG saying which
 * of the two failed, as is an index of another kind or on another device, and what was kept stays.  Every stored
 * position p ORs 1 << (p / z) into colours[p % z]: the result does not depend on the order, the array is the same
 * bytes on every run.  A stored position the index cannot give, or one at or past S * z, is a damaged image: the call
 * fails naming the lowest such stored position, and what was kept stays.  The words cost 8 bytes a k-mer; new ones are
 * filled in an allocation of their own that replaces the kept one when complete.  *ncolours_out = S (it may be NULL).  An index over an empty union cannot say S: it is refused.
 *
 * goss_gpu_object_colour_reads takes the batch as goss_gpu_object_classify_reads does and follows it in everything it
 * does not say otherwise: what a read and a window are, max_reads and GOSS_ERR_BUFFER (info->reads holds the need),
 * nbytes = 0, an input pointer of any alignment, the 2^32 - 1 window limit, a walk that cannot answer (the lowest byte
 * position is named and the call fails), synchronous on the object's stream, working memory that only grows, the same
 * input giving the same arrays.  d_colours[r] = the OR of colours[rank] over the windows of read r that are in the set
 * (a window at a rank whose word is 0 counts as a window and brings nothing), d_windows[r] = its number of windows,
 * d_read_starts as there; each of the three may be NULL, and so may info.  There is no early out: every valid window
 * walks, the word is exact.  info->by_count[j] = the reads whose word has j bits set, so their sum is info->reads;
 * info->windows = the sum of the windows.
 *
 * With no colours kept the call is GOSS_ERR_INVALID_ARG (goss_gpu_object_last_error says so), except for an empty
 * set, which has no word to read.  Only a GOSS_OBJECT_KMER_SET is accepted, and only the flag below (it must be given
 * to get the reference's result; without it the windows are looked up as they stand); anything else is
 * GOSS_ERR_INVALID_ARG.  A NULL object returns -1.
 *
 * goss_gpu_object_colour_reads_host: the same for a caller without device memory of its own (goss elect-reads): host
 * pointers for the batch and the three arrays, staged as goss_gpu_object_match_reads_host stages them.
 */
enum { GOSS_ELECT_NORMALIZE = 1 /* = GOSS_QUERY_NORMALIZE */ };
enum { GOSS_ELECT_MAX_COLOURS = 64 };
typedef struct {
    uint64_t reads;          /* reads in the input (what max_reads must hold) */
    uint64_t windows;        /* sum over the reads */
    uint64_t by_count[65];   /* reads per number of bits in their word */
    float ms;                /* HIP-event time of the kernels */
} goss_gpu_elect_info;
int goss_gpu_object_colours_host(goss_gpu_object* obj, const uint64_t* colours, uint32_t ncolours);
int goss_gpu_object_colours_from_index(goss_gpu_object* obj, goss_gpu_object* index, uint32_t* ncolours_out);
int goss_gpu_object_colour_reads(goss_gpu_object* obj, const void* d_bases, uint64_t nbytes, uint32_t flags,
                                 uint64_t max_reads, uint64_t* d_colours, uint32_t* d_windows, uint64_t* d_read_starts,
                                 goss_gpu_elect_info* info);
int goss_gpu_object_colour_reads_host(goss_gpu_object* obj, const void* bases, uint64_t nbytes, uint32_t flags,
                                      uint64_t max_reads, uint64_t* colours, uint32_t* windows, uint64_t* read_starts,
                                      goss_gpu_elect_info* info);

#endif /* GOSS_GPU_ELECT_H */
