"""gossamer_amd -- MI355X-native k-mer counting / de Bruijn edge-set construction.

The product is the C ABI in include/goss_gpu.h (libgossgpu.so, HIP kernels for gfx950) and
the C++ host command `goss` (build-kmer-set / build-graph).  This Python package only binds
the C ABI for tests and bench.py.
"""
from .binding import (Context, GossGpuError, MODE_GRAPH, MODE_KMER_SET, SYMBOLS,  # noqa: F401
                      OBJECT_ENTRY_EDGE_SET, OBJECT_GRAPH, OBJECT_KMER_SET, OBJECT_SPARSE_ARRAY, MATCH_ANY, MATCH_NORMALIZE, MATCH_SYMBOLS, CLASSIFY_NORMALIZE, CLASSIFY_SYMBOLS, NEAR_NORMALIZE, NEAR_SYMBOLS, NEAR_WHOLE_BASES, Object, encode_kmers,
                      group_emit, group_exchange, group_route_exchange, load, synth_reads_host,
                      POOL_PAIR_WORDS, POOL_POS_WORDS, POOL_TILE, format_double, pool_similarity_text,
                      TAXO_MANY, TAXO_NONE, TAXO_NORMALIZE, TAXO_SYMBOLS, format_phylogeny, parse_phylogeny, phylogeny_nodes,
                      ELECT_MAX_COLOURS, ELECT_NORMALIZE, ELECT_SYMBOLS, elect,
                      RECOUNT_REPORT_FIELDS, RELATIVE_REPORT_FIELDS, RELATIVE_SYMBOLS,
                      LINK_DTYPE, LINK_MISS, LINK_NONE, LINK_NON_UNIQUE, READ_LINKS_SYMBOLS, estimate_coverage, filter_links,
                      unique_segments)
