/* goss_gpu_links.h -- read links: the reads threaded over the linear segments of a finished graph, the "mapping reads"
 * stage of the reference's thread-reads; part of the C ABI of libgossgpu.so, included by goss_gpu.h (which declares
 * goss_gpu_ctx and the status codes) and not meant to be included alone. */
#ifndef GOSS_GPU_LINKS_H
#define GOSS_GPU_LINKS_H

/*
 * What is computed (GossCmdThreadReads.cc:321-402 over KmerAligner.hh:169-229, straight after build-supergraph, when
 * every superpath is one entry edge's linear path and a superpath id is an entry-edge rank):
 *
 * A segment is a linear path as goss_gpu_entries_build defines them, named by the rank of its first edge among the
 * entry edges.  seg(e) of an edge e is the segment that holds it, GOSS_LINK_NONE for an edge on a cycle of
 * one-in-one-out nodes, which has no entry edge.
 *
 * Per read (a line of the batch; '\n' ends it, any other byte that is not one of ACGTacgt ends the windows that hold
 * it) the valid forward (K+1)-windows e_0, e_1, ... are taken in order, not normalised, their reverse complements
 * not looked up.  Every window gets an answer:
 *   exact mode (flags 0)    seg(e_i) when e_i is an edge of the graph and has a segment, else a miss;
 *   GOSS_LINKS_CARRY        the reference's aligner.  With A_i = e_i is in the graph, and from(e_i) = to(e_{i-1}), and
 *                           e_i is the only edge that leaves that node: a window whose predecessor in the read was
 *                           aligned and for which A_i holds takes the predecessor's segment without a lookup -- even
 *                           where the node has two incoming edges and e_i starts a new segment, and across an 'N' where
 *                           the two edges happen to be adjacent.  Every other window is looked up as in exact mode.
 *                           The state is reset at every read; the reference never resets it, so that a read's first
 *                           window can carry from whatever read the same thread saw before: that dependence on the
 *                           schedule is not reproduced.
 * A window is a hit when it is aligned and its segment is unique.  Per read: gap counts the windows that are no hit;
 * the first hit primes (b = its segment, gap = 0); a hit on b changes nothing; a hit on another segment s adds the
 * record (a = b, b = s, gap) and sets b = s, gap = 0.  Over all reads of all batches count[a, b] is the number of
 * records and gap_sum[a, b] the sum of their gaps, both 64-bit (the reference's are uint32_t and wrap).  The table
 * does not depend on how the reads are cut into batches or ordered, as long as no read is cut.
 *
 * All entry points run between finish and emit, in graph mode, and leave the context's result untouched.  What
 * goss_gpu_read_links_begin builds is the context's held result: goss_gpu_read_links_release, or any call that gives
 * back a held result, gives it back, and the other entry points then answer GOSS_ERR_STATE.
 *
 * goss_gpu_read_links_begin: GOSS_ERR_STATE for a k-mer-set context, before finish and after emit;
 * GOSS_ERR_INVALID_ARG for an asymmetric graph (an edge without its reverse complement; last_error names the lowest),
 * for 2^32 - 1 edges or more, for flags other than GOSS_LINKS_CARRY, and for a bitmap whose unique_bits is not the
 * number of entry edges.  `unique`: one bit per entry rank, bit (i & 7) of byte i / 8, on the host; NULL (with
 * unique_bits 0): every segment is unique.  Working room: the link arrays and the list ranking of
 * goss_gpu_entries_build (about 40 bytes per edge); held afterwards: 5 bytes per edge, the bucket table of the window
 * lookup and the bitmap.
 */
#define GOSS_LINKS_CARRY 1u
#define GOSS_LINK_NONE 0xFFFFFFFFu        /* an edge without a segment */
#define GOSS_LINK_MISS 0xFFFFFFFFu        /* a window that was not aligned (an edge without a segment is a miss) */
#define GOSS_LINK_NON_UNIQUE 0x80000000u  /* set on a window's segment when the segment is not unique */

typedef struct {
    uint64_t edges, entries;
    uint64_t edges_without_segment;
    float ms_link, ms_rank, ms_segments;  /* device time: the link pass, the list ranking, the segment table */
    uint32_t reserved;
} goss_gpu_read_links_info;
int goss_gpu_read_links_begin(goss_gpu_ctx* ctx, uint32_t flags, const uint8_t* unique, uint64_t unique_bits, goss_gpu_read_links_info* info);

/* seg(e) of the edges of rank [first, first + count), to the host. */
int goss_gpu_read_links_segments(goss_gpu_ctx* ctx, uint64_t first, uint64_t count, uint32_t* out);

typedef struct {
    uint64_t reads;                       /* lines of the batch, empty ones included: its '\n's, and one more
                                           * when it does not end in one */
    uint64_t windows, misses, carried;    /* misses: windows that are no edge of the graph */
    uint64_t hits;                        /* 0 from goss_gpu_read_links_windows_host, which runs no linker */
    uint64_t records;                     /* records this batch added (0 from goss_gpu_read_links_windows_host) */
    float ms_windows, ms_scans, ms_compact;   /* device time: staging and lookup; the recurrences; hits, links and compaction */
    uint32_t reserved;
} goss_gpu_read_links_batch;

/* The answer per window of one batch of whole reads (`bases` on the host, n < 2^32 - 2 bytes), in read order: the
 * segment, with GOSS_LINK_NON_UNIQUE where it is not unique, or GOSS_LINK_MISS.  info->windows says how many there are;
 * at most `capacity` are written.  Nothing is accumulated. */
int goss_gpu_read_links_windows_host(goss_gpu_ctx* ctx, const void* bases, uint64_t n, uint32_t* out, uint64_t capacity,
                                     goss_gpu_read_links_batch* info);

/* The records of one batch of whole reads are added to those the context holds (12 bytes per record). */
int goss_gpu_read_links_add_host(goss_gpu_ctx* ctx, const void* bases, uint64_t n, goss_gpu_read_links_batch* info);

typedef struct { uint32_t a, b; uint64_t count, gap_sum; } goss_gpu_link_row;
typedef struct {
    uint64_t records, rows;
    float ms_sort, ms_reduce;
} goss_gpu_read_links_table_info;
/* The records held so far are sorted and reduced to the table, rows ascending by (a, b).  The records stay: batches
 * may follow, and a second call reduces again. */
int goss_gpu_read_links_finish(goss_gpu_ctx* ctx, goss_gpu_read_links_table_info* info);
int goss_gpu_read_links_table(goss_gpu_ctx* ctx, uint64_t first, uint64_t count, goss_gpu_link_row* out);
int goss_gpu_read_links_release(goss_gpu_ctx* ctx);

#endif /* GOSS_GPU_LINKS_H */
