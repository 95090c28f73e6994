// Stand-alone print-out of pycusdr_amd/csrc/record_layout.hpp (tests/test_record_layout.py): the header is host-only, so a plain C++
// compiler builds this.  usage: record_layout_print head post_max end_max max_tmpl max_hits edge_cands edge_bytes  bcap:symbols:stages ...
// One line per triple: every offset of RecordLayout by name, then bytes and stages.
#include <stdio.h>
#include <stdlib.h>

#include "../../pycusdr_amd/csrc/record_layout.hpp"

int main(int argc, char **argv) {
    if (argc < 9) {
        fprintf(stderr, "usage: %s head post_max end_max max_tmpl max_hits edge_cands edge_bytes bcap:symbols:stages ...\n", argv[0]);
        return 2;
    }
    RecordConsts k;
    size_t *fields[7] = {&k.head, &k.post_max, &k.end_max, &k.max_tmpl, &k.max_hits, &k.edge_cands, &k.edge_bytes};
    for (int i = 0; i < 7; ++i) *fields[i] = (size_t)strtoull(argv[1 + i], nullptr, 10);
    for (int i = 8; i < argc; ++i) {
        int bcap = 0, symbols = 0, stages = 0;
        if (sscanf(argv[i], "%d:%d:%d", &bcap, &symbols, &stages) != 3) {
            fprintf(stderr, "bad triple %s\n", argv[i]);
            return 2;
        }
        const RecordLayout l = record_layout(k, bcap, symbols, stages != 0);
        printf("bcap=%d symbols=%d scalars=%zu bands=%zu sym=%zu cen=%zu mag=%zu core=%zu bits=%zu cenw=%zu trust=%zu post=%zu end=%zu hits=%zu "
               "edges=%zu bytes=%zu stages=%d\n",
               bcap, symbols, l.scalars, l.bands, l.sym, l.cen, l.mag, l.core, l.bits, l.cenw, l.trust, l.post, l.end, l.hits, l.edges, l.bytes,
               (int)l.stages);
    }
    return 0;
}
