// Stand-alone print-out of the uniform rational plan of pycusdr_amd/csrc/channelize_plan.hpp
// (tests/test_channelizer_uniform_rational_host.py): the header is host-only, so a plain C++ compiler builds this.
// usage: channelize_uniform_rational_plan_print M:U:D:T:out_base:out_count ...
// One line per tuple: the tuple, the helpers chur_frames / chur_span / chur_lds_bytes on their own, the fields of the
// CHZ_UNIFORM_RATIONAL ChzGeom, the grid and the input span of the call, and the budget.
#include <stdio.h>
#include <stdlib.h>

#include "../../pycusdr_amd/csrc/channelize_plan.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s M:U:D:T:out_base:out_count ...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        int M = 0, U = 0, D = 0, T = 0, out_count = 0;
        long long out_base = 0;
        if (sscanf(argv[i], "%d:%d:%d:%d:%lld:%d", &M, &U, &D, &T, &out_base, &out_count) != 6) {
            fprintf(stderr, "bad tuple %s\n", argv[i]);
            return 2;
        }
        const int F = chur_frames(M, U, D, T);
        const ChzGeom g = chz_geom(CHZ_UNIFORM_RATIONAL, U, D, T, M);
        int64_t first = 0, last = 0;
        chz_input_span(g, out_base, out_count, &first, &last);
        printf("M=%d U=%d D=%d T=%d out_base=%lld out_count=%d F=%d span=%d lds=%zu kind=%d gU=%d gD=%d gT=%d gM=%d Tb=%d threads=%d tile=%d "
               "L=%d S=%d lds_bytes=%zu grid=%u first=%lld last=%lld budget=%d\n",
               M, U, D, T, out_base, out_count, F, chur_span(U, D, T, F), chur_lds_bytes(M, U, D, T, F), g.kind, g.U, g.D, g.T, g.M, g.Tb,
               g.threads, g.tile, g.L, g.S, g.lds_bytes, chz_grid(g, out_count), (long long)first, (long long)last, (int)CHU_LDS_BUDGET);
    }
    return 0;
}
