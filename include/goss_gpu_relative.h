/* goss_gpu_relative.h -- the two graph passes of the reference's `translucent` executable that need no traversal:
 * trim-relative and merge-graph-with-reference; part of the C ABI of libgossgpu.so, included by goss_gpu.h (which declares
 * goss_gpu_ctx, goss_gpu_object and the status codes) and not meant to be included alone. */
#ifndef GOSS_GPU_RELATIVE_H
#define GOSS_GPU_RELATIVE_H

/*
 * Both entry points run between finish and emit, in graph mode, over the edge list the context holds, and follow
 * goss_gpu_prune_tips in everything they do not say otherwise: GOSS_ERR_STATE for a k-mer-set context, before finish
 * and after emit; GOSS_ERR_INVALID_ARG for a graph with multiplicities of 2^32 - 1 or more (goss_gpu_big_counts);
 * GOSS_ERR_OOM when the working arrays do not fit the context's arena; in each case, and after every other failure
 * named below, the result is what it was before the call and the report is zero.  Afterwards the context's result is
 * the new graph: goss_gpu_result, goss_gpu_emit, goss_gpu_emit_estimate, goss_gpu_emit_dump, goss_gpu_lint and the
 * other passes work on it unchanged.  Whatever the context held (segments, an entry edge set, components) is given back.
 *
 * goss_gpu_trim_relative (TransCmdTrimRelative.cc:81-191).  The edges that leave one node are adjacent in rank order, at
 * most four.  A node with two or more of them is judged (a fork); a node with one never is.  With `total` the sum of
 * their multiplicities as uint64_t, an edge of multiplicity c is below its node's threshold iff
 * (double)c < (double)total * rel -- one IEEE multiplication and one strict comparison, as the reference's
 * `pCounts[i] < totalCount * mRelCoverage`.  Every edge below its threshold goes, and so does its reverse complement;
 * edges that enter a node are judged only as the edges that leave the complementary node, so an edge can go as a
 * mirror image alone.  The reference splits the ranks among its threads at the first edge of a node, so its result
 * does not depend on their number; it is the one computed here.  rel <= 0 removes nothing; rel > 1 removes every edge
 * of every fork whose multiplicities are not all zero.  rel must be finite, else GOSS_ERR_INVALID_ARG.
 * The reference builds the survivors with their exact number as the estimate (zapped.count() counts distinct bits, an
 * edge that is its own reverse complement once): a following goss_gpu_emit writes its files.
 * An edge below its threshold whose reverse complement the graph lacks is GOSS_ERR_INVALID_ARG (last_error names the
 * lowest such index); other edges' mirror images are not looked up.  More than 2^32 - 2 edges: GOSS_ERR_INVALID_ARG.
 * Working room: two bits per edge for the two bitmaps, and only where an edge is below its threshold about four
 * bytes per edge for the bucket table of the mirror search and the survivors once more while they are compacted.
 * None of the link arrays of goss_gpu_prune_tips (9 bytes per edge) is built.
 * An empty graph stays empty (the reference calls select(0) on it).
 *
 * goss_gpu_recount_from (TransCmdMergeGraphWithReference.cc:47-114).  The result becomes its edges that `ref` holds
 * too, each with the multiplicity `ref` gives it; presence is what the reference's index says, not "multiplicity
 * != 0".  ref must be a GOSS_OBJECT_GRAPH of the same K (last_error names both Ks otherwise), not asymmetric, open
 * on the context's device: anything else is GOSS_ERR_INVALID_ARG, as is a walk of ref's index that cannot answer
 * (a damaged object; last_error names the lowest such edge).  ref is only read, and must stay open during the call.
 * The reference builds its output with the edge count of graph-in as the size estimate, not the survivors':
 * goss_gpu_emit_estimate(ctx, rep.edges_before) writes its files.
 * Working room: a bit and four bytes per edge, and the survivors once more while they are compacted.
 */
typedef struct {
    uint64_t edges_before, edges_after;   /* before - after = distinct edges removed (the reference's "number of edges removed") */
    uint64_t forks;                       /* from-nodes with >= 2 out-edges: the nodes judged */
    uint64_t below;                       /* edges below their own node's threshold */
    uint64_t mirror_only;                 /* edges removed only because their reverse complement was below */
} goss_gpu_relative_report;
int goss_gpu_trim_relative(goss_gpu_ctx* ctx, double rel, goss_gpu_relative_report* rep);

typedef struct { uint64_t edges_before, edges_after; } goss_gpu_recount_report;
int goss_gpu_recount_from(goss_gpu_ctx* ctx, goss_gpu_object* ref, goss_gpu_recount_report* rep);

/* ms[3]: device time of the phases of the last of the two calls above that got past its checks, in milliseconds --
 * trim-relative: judge, mirror (the bucket table and the search), compaction; recount: lookup, 0, compaction; 0 for a
 * phase it did not reach. */
int goss_gpu_relative_timing(goss_gpu_ctx* ctx, float* ms);

#endif /* GOSS_GPU_RELATIVE_H */
