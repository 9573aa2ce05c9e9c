// tests/host/plonk_desc_check.cpp -- sipp_amd/csrc/plonk_desc.hpp on its own (CPU only; built with the sanitizers by the Makefile's
// plonk_desc_check_asan, fed by tests/test_plonk_desc_host.py).  One description per line on stdin, the reason per line on stdout:
//   lookup <num_wires> <num_constants> <num_selectors> <w0> .. <w7>     the lookup validator
//   params <R> <D> <C> <log_n>                                          the parameters, as the permutation argument needs them
//                                                                        (routed wires, the chunk cap); "ok <log_d> <m>" when served
#include <stdio.h>
#include <string.h>

#include "plonk_desc.hpp"

int main() {
    static const char* const lookup_names[] = {"ok", "too_many_slots", "empty_with_tag", "one_sided", "circuit_sizes", "column_outside",
                                               "marker_is_selector", "tag_columns"};
    static const char* const params_names[] = {"ok", "bad_argument", "chunk_size", "counts"};
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        unsigned v[11];
        if (sscanf(line, "lookup %u %u %u %u %u %u %u %u %u %u %u", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9, v + 10) == 11) {
            const uint32_t w[8] = {v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]};
            const plonk_desc::Lookup l = plonk_desc::lookup_of(w);
            for (int q = 0; q < 8; q++)
                if (plonk_desc::lookup_word(l, q) != w[q]) return 3;
            puts(lookup_names[(int)plonk_desc::lookup_check(l, v[0], v[1], v[2])]);
        } else if (sscanf(line, "params %u %u %u %u", v, v + 1, v + 2, v + 3) == 4) {
            const sipp_plonk_params p{v[0], v[1], v[2]};
            uint32_t log_d = 0, m = 0;
            const plonk_desc::Params r = plonk_desc::params_check(&p, v[3], plonk_desc::ROUTED | plonk_desc::CHUNK_CAP, &log_d, &m);
            if (r == plonk_desc::Params::ok) printf("ok %u %u\n", log_d, m);
            else puts(params_names[(int)r]);
        } else {
            fprintf(stderr, "plonk_desc_check: cannot read: %s", line);
            return 2;
        }
    }
    return 0;
}
