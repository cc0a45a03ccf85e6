/* goss_gpu_match.h -- reads against an object resident in HBM; part of the C ABI of libgossgpu.so, included by
 * goss_gpu.h (which declares goss_gpu_object and the status codes) and not meant to be included alone. */
#ifndef GOSS_GPU_MATCH_H
#define GOSS_GPU_MATCH_H

/* Reads against an object: which reads share a k-mer / an edge with a KmerSet or a Graph.
 *
 * The role of the per-read loops of extract-reads (GossCmdExtractReads.cc:94-108: a read is kept when one of its
 * (K + 1)-mers is an edge of the graph) and of filter-reads (GossCmdFilterReads.cc:46-79, 136-153: a read, or a
 * pair, goes to the match file when one of its k-mers is in the set): GossRead::Iterator over the read, one
 * access() per window.  Here one call takes a batch of reads as bytes on the device and answers per read; the
 * window keys are made and looked up in registers and never stored.
 *
 * d_bases / nbytes: the byte form goss_gpu_push_bases_device takes.  A read is a maximal stretch of bytes between
 * '\n' (0x0A) bytes: a last stretch without its '\n' is a read, two adjacent '\n' enclose an empty read, so the
 * number of reads is the number of '\n' plus one if the last byte is none; no other byte ends a read.  A window is
 * L consecutive bytes of one read, all of ACGTacgt, L being the object's key length (K for a KmerSet, K + 1 for a
 * Graph's edges); its key has the first base in the most significant used bits -- exactly what
 * GossRead::Iterator(read, L) yields (GossRead.hh:57-114, GossReadBaseString.hh:133-188).
 *
 * Per read r: d_windows[r] = its number of windows, always exact; d_hits[r] = how many of them are in the object
 * (every window counts, repeats included) or, with GOSS_MATCH_ANY, 1 if at least one is and else 0 -- a read that has
 * matched then stops costing lookups.  GOSS_MATCH_NORMALIZE looks up each window's canonical form (as
 * GOSS_QUERY_NORMALIZE does), so either strand matches a KmerSet.  d_read_starts[r] = the byte offset of read r,
 * d_read_starts[reads] = the offset past the last read's last base (nbytes, or nbytes - 1 when the input ends in
 * '\n').  d_windows and d_hits hold max_reads entries, d_read_starts max_reads + 1; any of the three may be NULL,
 * and so may info.  With all three NULL max_reads is not looked at (info->reads is then the way to size them).
 *
 * Synchronous on the object's stream, like the queries; nbytes = 0 answers 0 reads.  Working memory beyond the
 * outputs: 8 bytes per 2,048 input bytes, kept by the object.  The same input gives the same arrays.
 * GOSS_ERR_BUFFER: more reads than max_reads (info->reads holds the need, the arrays are unspecified).
 * GOSS_ERR_INVALID_ARG: a bare SparseArray (no key length); an unknown flag bit; a read with 2^32 - 1 windows or
 * more (named); an index walk that cannot answer (a damaged image: the lowest such byte position is named) -- no
 * call returns a silent wrong answer.
 *
 * The packed 2-bit form (goss_gpu_push_packed_*) is not taken: its non-base flag cannot tell a read separator
 * from an N, and reads are what this call answers for.
 */
enum { GOSS_MATCH_NORMALIZE = 1 /* = GOSS_QUERY_NORMALIZE */, GOSS_MATCH_ANY = 4 };
typedef struct {
    uint64_t reads;          /* reads in the input (what max_reads must hold) */
    uint64_t windows, hits;  /* sums over the reads (hits: as the mode defines it) */
    uint64_t matched_reads;  /* reads with hits > 0 */
    float ms;                /* HIP-event time of the kernels */
} goss_gpu_match_info;
int goss_gpu_object_match_reads(goss_gpu_object* obj, const void* d_bases, uint64_t nbytes, uint32_t flags,
                                uint64_t max_reads, uint32_t* d_windows, uint32_t* d_hits,
                                uint64_t* d_read_starts, goss_gpu_match_info* info);
/* The same for a caller without device memory of its own (the goss commands): bases and the three arrays are host
 * pointers (page-locked ones, goss_gpu_host_alloc, copy fastest); the batch is copied to a buffer the object keeps,
 * matched there, and 4 bytes per read and array come back -- never the read text. */
int goss_gpu_object_match_reads_host(goss_gpu_object* obj, const void* bases, uint64_t nbytes, uint32_t flags,
                                     uint64_t max_reads, uint32_t* windows, uint32_t* hits, uint64_t* read_starts,
                                     goss_gpu_match_info* info);

#endif /* GOSS_GPU_MATCH_H */
