// plan_step's rerun grid (csrc/step_plan.hpp) from the command line, for
// tests/test_rerun_plan.py: StepIn rows as whitespace-separated integers on
// stdin (the fields in step_plan_main.cpp's order), one line per row on
// stdout: spec, segs, rerun_grid, and the bound the header was built with.
#include <cstdio>
#include <iostream>

#include "step_plan.hpp"

int main() {
    lc::StepIn in;
    long long K, n_events, max_configs, ws_words, fin_words, ws_max_bytes;
    int b[11];
    while (std::cin >> K >> n_events >> in.cu_count) {
        for (int i = 0; i < 6; ++i) std::cin >> b[i];
        std::cin >> in.algorithm >> in.flags >> in.path_flags >> in.spec_segs >> max_configs;
        for (int i = 6; i < 11; ++i) std::cin >> b[i];
        std::cin >> in.spec8_waves >> ws_words >> fin_words >> ws_max_bytes;
        if (!std::cin) return 1;
        in.K = K; in.n_events = (uint64_t)n_events; in.max_configs = (uint64_t)max_configs;
        in.t0_only = b[0]; in.table = b[1]; in.taggable = b[2]; in.seg_pays = b[3]; in.validated = b[4];
        in.has_events16 = b[5];
        in.want_peak = b[6]; in.want_final = b[7]; in.want_n_final = b[8]; in.res_host = b[9]; in.allow_async = b[10];
        in.ws_words = (uint64_t)ws_words; in.fin_words = (uint64_t)fin_words; in.ws_max_bytes = (uint64_t)ws_max_bytes;
        const lc::StepPlan p = lc::plan_step(in);
        std::printf("%d %d %d %d\n", p.spec, p.segs, p.rerun_grid, lc::SPEC_RERUN_GRID);
    }
    return 0;
}
