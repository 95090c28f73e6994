// Stand-alone print-out of pycusdr_amd/csrc/channelize_plan.hpp (tests/test_channelize_plan_host.py): the header is host-only, so a
// plain C++ compiler builds this.  usage: channelize_plan_print kind:U:D:T:M:out_base:out_count:cell_frames ...
// (kind 0 integer, 1 rational, 2 uniform, 3 survey; cell_frames is read for a survey).  One line per tuple: the tuple, every field
// of ChzGeom, the grid and the input span of the call, and for a survey its chunk and the tables of a handle whose max_out is
// out_count (0 for the other kinds).
#include <stdio.h>
#include <stdlib.h>

#include "../../pycusdr_amd/csrc/channelize_plan.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s kind:U:D:T:M:out_base:out_count:cell_frames ...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        int kind = 0, U = 0, D = 0, T = 0, M = 0, out_count = 0, cell = 0;
        long long out_base = 0;
        if (sscanf(argv[i], "%d:%d:%d:%d:%d:%lld:%d:%d", &kind, &U, &D, &T, &M, &out_base, &out_count, &cell) != 8 || kind < 0 || kind > 3) {
            fprintf(stderr, "bad tuple %s\n", argv[i]);
            return 2;
        }
        const ChzGeom g = chz_geom(kind, U, D, T, M);
        int64_t first = 0, last = 0;
        chz_input_span(g, out_base, out_count, &first, &last);
        int C = 0;
        ChusTables t = {};
        if (kind == CHZ_SURVEY) {
            C = chus_chunk(g, cell);
            t = chus_tables(g, cell, out_count);
        }
        printf("kind=%d U=%d D=%d T=%d M=%d out_base=%lld out_count=%d cell_frames=%d Tb=%d threads=%d tile=%d L=%d S=%d lds_bytes=%zu grid=%u "
               "first=%lld last=%lld C=%d cells=%lld chunks=%lld words=%d\n",
               g.kind, g.U, g.D, g.T, g.M, out_base, out_count, cell, g.Tb, g.threads, g.tile, g.L, g.S, g.lds_bytes, chz_grid(g, out_count),
               (long long)first, (long long)last, C, (long long)t.cells, (long long)t.chunks, t.words);
    }
    return 0;
}
