// plan_lane (csrc/lane_plan.hpp) from the command line, for tests/test_lane_plan.py:
// LaneIn rows as whitespace-separated integers on stdin (the fields in the
// order read below, then n_flight triples seq lo hi), one line of LanePlan
// fields per row on stdout.
#include <cstdio>
#include <iostream>

#include "lane_plan.hpp"

int main() {
    unsigned long long seq, run_n, lo, hi;
    long long waves, resident_waves;
    int b[5], path_flags, n_flight;
    std::printf("%d %d %d\n", lc::LANES, lc::LANE_SLOTS, lc::LANE_FLIGHT);
    while (std::cin >> seq >> run_n) {
        for (int &v : b) std::cin >> v;
        std::cin >> path_flags >> waves >> resident_waves >> lo >> hi >> n_flight;
        if (!std::cin || n_flight < 0 || n_flight > lc::LANE_FLIGHT) return 1;
        lc::LaneIn in;
        in.seq = seq; in.run_n = run_n;
        in.async = b[0]; in.spec = b[1]; in.split = b[2]; in.comm = b[3]; in.mapped = b[4];
        in.path_flags = path_flags;
        in.waves = waves; in.resident_waves = resident_waves;
        in.lo = lo; in.hi = hi;
        in.n_flight = n_flight;
        for (int i = 0; i < n_flight; ++i) {
            unsigned long long fs, fl, fh;
            std::cin >> fs >> fl >> fh;
            in.flight[i].seq = fs; in.flight[i].lo = fl; in.flight[i].hi = fh;
        }
        if (!std::cin) return 1;
        const lc::LanePlan p = lc::plan_lane(in);
        std::printf("%d %d %d %lld %d %lld\n", p.lane, p.overlap, p.direct, (long long)p.after, p.slot,
                    (long long)p.slot_waits);
    }
    return 0;
}
