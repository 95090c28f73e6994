// Stand-alone print-out of the synthesiser's plan arithmetic in pycusdr_amd/csrc/channelize_plan.hpp
// (tests/test_synthesizer_host.py): the header is host-only, so a plain C++ compiler builds this.
// usage: synthesize_plan_print M:I:T:out_base:out_count ...   One line per tuple: the tuple, the CHZ_SYNTHESIS geometry -- F, the rows
// of the image, the LDS bytes (0 where the plan does not fit) -- and the grid of the call.
#include <stdio.h>
#include <stdlib.h>

#include "../../pycusdr_amd/csrc/channelize_plan.hpp"

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s M:I:T:out_base:out_count ...\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        int M = 0, I = 0, T = 0, out_count = 0;
        long long out_base = 0;
        if (sscanf(argv[i], "%d:%d:%d:%lld:%d", &M, &I, &T, &out_base, &out_count) != 5 || M < 1 || I < 1 || T < 1 || out_count < 1) {
            fprintf(stderr, "bad tuple %s\n", argv[i]);
            return 2;
        }
        const ChzGeom g = chz_geom(CHZ_SYNTHESIS, I, 1, T, M);
        const int F = chsy_frames(M, I, T);
        printf("M=%d I=%d T=%d out_base=%lld out_count=%d kind=%d U=%d D=%d Tb=%d threads=%d tile=%d F=%d rows=%d lds_bytes=%zu grid=%u\n", g.M,
               g.U, g.T, out_base, out_count, g.kind, g.U, g.D, g.Tb, g.threads, g.tile, F, F ? chsy_rows(I, T, F) : 0, g.lds_bytes,
               F ? chsy_grid(g, out_base, out_count) : 0u);
    }
    return 0;
}
