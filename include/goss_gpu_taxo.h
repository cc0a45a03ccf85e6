/* goss_gpu_taxo.h -- a taxonomy over the k-mers of a KmerSet resident in HBM: annotate-kmers and classify-reads; part
 * of the C ABI of libgossgpu.so, included by goss_gpu.h (which declares goss_gpu_object and the status codes) and not
 * meant to be included alone. */
#ifndef GOSS_GPU_TAXO_H
#define GOSS_GPU_TAXO_H

/*
 * The tree.  goss_gpu_object_taxo_tree_host takes n nodes in any order: ids[i] is a node's id, parent_index[i] the
 * index (not the id) of its parent, the root being its own parent.  It is refused (GOSS_ERR_INVALID_ARG,
 * goss_gpu_object_last_error says which node) unless there is exactly one root, every parent_index is below n, every
 * node hangs under the root, no id occurs twice and none is GOSS_TAXO_NONE or GOSS_TAXO_MANY.  The object keeps the
 * tree until it is closed; a second call replaces it and drops the annotation, whose classes were numbered by the
 * first.  Every array below that is "per node" is in the order of this call.
 *
 * The annotation: one node id per k-mer rank, GOSS_TAXO_NONE for a k-mer nothing has touched -- the bytes of the
 * <set>.annotation file.  goss_gpu_object_taxo_annotation_host(obj, NULL) starts an all-untouched one,
 * (obj, ann) loads count ids; an id the tree lacks is GOSS_ERR_INVALID_ARG naming the id and the rank, and the
 * annotation held before stays as it was.  goss_gpu_object_taxo_annotation_read copies it out (ann_out: count ids)
 * with counts_out[i] = the ranks whose class is exactly node i (n values); either may be NULL.
 *
 * goss_gpu_object_taxo_annotate: every valid K-window of every read of the batch is looked up, and at its rank r
 * class[r] = lca(class[r], the read's node), a first touch setting it.  d_read_nodes holds max_reads node ids, one per
 * read, all of them in the tree (else GOSS_ERR_INVALID_ARG naming the read and the id, before anything is touched);
 * a batch of more reads than max_reads is GOSS_ERR_BUFFER with info->reads the need, again before anything is touched.
 * lca is associative, commutative and idempotent: the annotation depends neither on the order of the calls nor on how
 * the reads are split over them.  d_windows[r] = the valid windows of read r (may be NULL).
 *
 * goss_gpu_object_taxo_classify_reads: result[r] = the deepest class among the windows of read r when those classes
 * lie on one root-to-leaf path, GOSS_TAXO_MANY when they do not, GOSS_TAXO_NONE when no window has a class.  A window
 * at a rank whose class is GOSS_TAXO_NONE is ignored as if absent and counted in info->unannotated.
 *
 * Both follow goss_gpu_object_classify_reads in what a read and a window are, max_reads, nbytes = 0, an input of any
 * alignment, the 2^32 - 1 window limit, a walk that cannot answer, the _host forms that stage the batch.  Only a
 * GOSS_OBJECT_KMER_SET is accepted and only the flag below.  Without a tree, or without an annotation, they return
 * GOSS_ERR_STATE -- except on an empty set, which accepts everything (no tree, no annotation, any node ids), touches
 * nothing and answers GOSS_TAXO_NONE.
 *
 * goss_gpu_object_taxo_pair: d_out[i] = the join of d_a[i] and d_b[i], each a node id or one of the two sentinels as
 * classify_reads returns them (the mates of a pair): the deeper when one is an ancestor-or-equal of the other, MANY
 * when not or when either is MANY, the other when one is NONE.  goss_gpu_object_taxo_tally: counts[i] = how many of the
 * n values are node i, counts[n_nodes] the NONEs, counts[n_nodes + 1] the MANYs (counts: n_nodes + 2 values on the
 * host).  In both an id the tree lacks is GOSS_ERR_INVALID_ARG naming the index.  The _host forms take host arrays.
 */
#define GOSS_TAXO_NONE 0xFFFFFFFFu
#define GOSS_TAXO_MANY 0xFFFFFFFEu
enum { GOSS_TAXO_NORMALIZE = 1 /* = GOSS_QUERY_NORMALIZE */ };
typedef struct {
    uint64_t reads;          /* reads in the input (what max_reads must hold) */
    uint64_t windows;        /* sum over the reads */
    uint64_t hits;           /* annotate: windows found in the set */
    uint64_t none;           /* classify: reads without a class */
    uint64_t many;           /* classify: reads whose classes lie on more than one path */
    uint64_t unannotated;    /* classify: windows found at a rank without a class */
    float ms;                /* HIP-event time of the kernels */
} goss_gpu_taxo_info;
int goss_gpu_object_taxo_tree_host(goss_gpu_object* obj, uint32_t n, const uint32_t* ids, const uint32_t* parent_index);
int goss_gpu_object_taxo_annotation_host(goss_gpu_object* obj, const uint32_t* ann);
int goss_gpu_object_taxo_annotation_read(goss_gpu_object* obj, uint32_t* ann_out, uint64_t* counts_out);
int goss_gpu_object_taxo_annotate(goss_gpu_object* obj, const void* d_bases, uint64_t nbytes, const uint32_t* d_read_nodes,
                                  uint32_t flags, uint64_t max_reads, uint32_t* d_windows, goss_gpu_taxo_info* info);
int goss_gpu_object_taxo_annotate_host(goss_gpu_object* obj, const void* bases, uint64_t nbytes, const uint32_t* read_nodes,
                                       uint32_t flags, uint64_t max_reads, uint32_t* windows, goss_gpu_taxo_info* info);
int goss_gpu_object_taxo_classify_reads(goss_gpu_object* obj, const void* d_bases, uint64_t nbytes, uint32_t flags,
                                        uint64_t max_reads, uint32_t* d_result, uint32_t* d_windows, uint64_t* d_read_starts,
                                        goss_gpu_taxo_info* info);
int goss_gpu_object_taxo_classify_reads_host(goss_gpu_object* obj, const void* bases, uint64_t nbytes, uint32_t flags,
                                             uint64_t max_reads, uint32_t* result, uint32_t* windows, uint64_t* read_starts,
                                             goss_gpu_taxo_info* info);
int goss_gpu_object_taxo_pair(goss_gpu_object* obj, const uint32_t* d_a, const uint32_t* d_b, uint64_t n, uint32_t* d_out);
int goss_gpu_object_taxo_pair_host(goss_gpu_object* obj, const uint32_t* a, const uint32_t* b, uint64_t n, uint32_t* out);
int goss_gpu_object_taxo_tally(goss_gpu_object* obj, const uint32_t* d_values, uint64_t n, uint64_t* counts);
int goss_gpu_object_taxo_tally_host(goss_gpu_object* obj, const uint32_t* values, uint64_t n, uint64_t* counts);

#endif /* GOSS_GPU_TAXO_H */
