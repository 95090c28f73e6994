// record_layout.hpp -- where the pieces of a block's result record sit: the ONE statement of the byte layout.
//
//   [BlockScalars, head bytes][bands 2 x band_capacity complex64][sym int32][cen int32][mag float32]      <- core
//   [bits u8][centres u8][trust u8][post][end][hits int32: idx | score per template][would-be stash edges]  <- stream stages only
//
// Every piece starts on a 16-byte boundary; the record is contiguous so that ONE copy brings it to the host.  Host only and free of
// HIP, so a plain C++ compiler builds it (tests/csrc/record_layout_print.cpp).  The sizes it depends on keep their definitions where
// the kernels use them (bank_ctx.hpp, stream_kernels.hpp) and arrive here as a RecordConsts.
#pragma once
#include <stddef.h>
#include <stdint.h>

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct RecordConsts {
    size_t head;                   // BLK_HEAD: bytes set aside for the BlockScalars
    size_t post_max, end_max;      // STREAM_POST_MAX, STREAM_END_MAX
    size_t max_tmpl, max_hits;     // STREAM_MAX_TMPL, STREAM_MAX_HITS
    size_t edge_cands, edge_bytes; // STREAM_EDGE_CANDS, sizeof(StreamEdge)
};

struct RecordLayout {              // byte offsets inside one record
    size_t scalars, bands, sym, cen, mag;
    size_t core;                   // bytes without the stream stages' outputs (= where they start)
    size_t bits, cenw, trust, post, end, hits, edges;      // 0 without stages
    size_t bytes;                  // the whole record: the stride between the blocks of a batch
    bool stages;
};

static inline RecordLayout record_layout(const RecordConsts &k, int band_capacity, int symbols, bool stages) {
    RecordLayout l = {};
    const size_t arr = align16((size_t)symbols * sizeof(int32_t));
    l.scalars = 0;
    l.bands = k.head;
    l.sym = l.bands + align16((size_t)2 * band_capacity * 2 * sizeof(float));
    l.cen = l.sym + arr;
    l.mag = l.cen + arr;
    l.core = l.bytes = l.mag + arr;
    l.stages = stages;
    if (stages) {
        const size_t a1 = align16((size_t)symbols);
        l.bits = l.core;
        l.cenw = l.bits + a1;
        l.trust = l.cenw + a1;
        l.post = l.trust + a1;
        l.end = l.post + k.post_max;
        l.hits = l.end + k.end_max;
        l.edges = l.hits + k.max_tmpl * 2 * k.max_hits * sizeof(int32_t);
        l.bytes = l.edges + align16(k.edge_cands * k.edge_bytes);
    }
    return l;
}
