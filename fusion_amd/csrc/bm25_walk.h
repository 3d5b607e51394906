// bm25_walk.h -- what the lexical posting walk of bm25.hip (the whole corpus) and its restatement in bm25_stream.hip (a range of documents)
// must agree on: the modes, the table grain, the terms per batch and the workgroup shapes.  The walk itself is not shared: as one device
// function called from both kernels it cost bm25_kernel registers and an occupancy step (profiles/r14_slices_refactor.json).
// The same held within the range family: moving lexical_range_kernel's walk into a __forceinline__ function, to share it with a counting
// kernel in bm25_count.hip, took its TF-IDF instantiations from 32 / 33 to 58 VGPRs (plane / filter; cross-compiled).  An epilogue
// parameter of the one kernel does not: with plane, filter and count as LEX_* values of lexical_range_kernel's own template parameter the
// walk stays in the __global__ body, and all six instantiations keep the registers, LDS and occupancy that the two restated kernels had
// (pinned in tests/test_bm25_stream_cpu.py and tests/test_bm25_count_cpu.py; timed in profiles/r27_lexical_walk_ab.json).
#pragma once
#include "slices.h"

namespace fz {

constexpr int BM25_GRAIN = 3584;    // granularity of the per-index posting-offset table (fz_bm25_slice_offsets): a workgroup's slice is 1 or 2 of these
constexpr int BM25_TERMS = 256;     // query terms whose posting ranges are resolved per batch

// MODE: 0 = BM25's expression per posting; 1 = TFIDF: score += tf * idf (bm25.py:114); 2 = the posting's term comes from a table (pval):
// every posting of the index has ONE value for a given (k1, b) -- idf, tf and the document's length norm are all the index's -- so the
// float64 division (a dozen instructions at half rate: most of this kernel's time) is done once per index, like the idf table, not once
// per (query, posting); the walk adds the same bits in the same order.
enum { BM25_EXPR = 0, BM25_TFIDF = 1, BM25_PVAL = 2 };

// EPI: what the range walk (lexical_range_kernel) does with a slice's accumulators -- slices.h's store_plane, filter_candidates, count_beaters
enum { LEX_PLANE = 0, LEX_FILTER = 1, LEX_COUNT = 2 };

// One workgroup's slice, for the kernels' walks and the launchers' grids and LDS alike: table grains per slice x BM25_GRAIN documents, and
// its threads -- PVAL 3,584 documents x 512 threads, the others 7,168 x 1,024 (measured: see bm25_kernel).
constexpr int BM25_PV_GRAINS = 1, BM25_PV_THREADS = 512;
template <int MODE> constexpr int slice_grains() { return MODE == BM25_PVAL ? BM25_PV_GRAINS : 2; }
template <int MODE> constexpr int slice_docs() { return BM25_GRAIN * slice_grains<MODE>(); }
template <int MODE> constexpr int slice_threads() { return MODE == BM25_PVAL ? BM25_PV_THREADS : 1024; }
static_assert(slice_docs<BM25_EXPR>() == 7168 && slice_docs<BM25_TFIDF>() == 7168 && slice_docs<BM25_PVAL>() == 3584,
              "the measured slice sizes (see bm25_kernel)");

}  // namespace fz
