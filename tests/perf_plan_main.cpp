// Stand-alone driver of csrc/perf_plan.hpp for tests/test_perf_plan.py: reads
// commands on stdin, prints one line of integers per command.
//   bucket T DT          -> floor(T / DT), its midpoint
//   qindex N Q           -> min(N - 1, (long) floor((double) N * Q))   (Q as a decimal)
//   qrange N0 N1 Q       -> the index for every N in [N0, N1], one line
//   tier N FORCE         -> 0 none, 1 LDS, 2 HBM
//   tile B B0            -> the tile slot of bucket B in a workgroup that starts at B0, or -1
//   index F TYPE REL NR NQ -> rate index, group index
//   bias MAXMAG          -> magnitude bits, live latency digits
//   dtbits DT            -> bits of x - bucket start, live time digits
//   shape N NM TMIN TMAX XMIN XMAX NF RDT QDT -> rc rate_first rate_n q_first q_n
//   consts               -> records per workgroup, tile buckets, LDS limit, digit bits, LDS share
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "perf_plan.hpp"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "bucket") {
            long long t, dt;
            std::cin >> t >> dt;
            const int64_t b = lcp::perf_bucket(t, dt);
            std::printf("%lld %lld\n", (long long)b, (long long)lcp::perf_bucket_mid(b, dt));
        } else if (cmd == "qindex") {
            unsigned long long n;
            double q;
            std::cin >> n >> q;
            std::printf("%llu\n", (unsigned long long)lcp::perf_quantile_index(n, q));
        } else if (cmd == "qrange") {
            unsigned long long n0, n1;
            double q;
            std::cin >> n0 >> n1 >> q;
            for (unsigned long long n = n0; n <= n1; ++n) std::printf("%llu ", (unsigned long long)lcp::perf_quantile_index(n, q));
            std::printf("\n");
        } else if (cmd == "tier") {
            unsigned long long n;
            int force;
            std::cin >> n >> force;
            std::printf("%d\n", lcp::perf_tier(n, force != 0));
        } else if (cmd == "tile") {
            long long b, b0;
            std::cin >> b >> b0;
            std::printf("%d\n", lcp::perf_tile_slot(b, b0));
        } else if (cmd == "index") {
            unsigned f, type;
            unsigned long long rel, nr, nq;
            std::cin >> f >> type >> rel >> nr >> nq;
            std::printf("%llu %llu\n", (unsigned long long)lcp::perf_rate_index(f, type, rel, nr),
                        (unsigned long long)lcp::perf_group_index(f, rel, nq));
        } else if (cmd == "bias") {
            unsigned long long m;
            std::cin >> m;
            const uint32_t k = lcp::perf_mag_bits(m);
            std::printf("%u %u\n", k, lcp::perf_live_digits(k + 1));
        } else if (cmd == "dtbits") {
            long long dt;
            std::cin >> dt;
            const uint32_t k = lcp::perf_dt_bits(dt);
            std::printf("%u %u\n", k, lcp::perf_live_digits(k));
        } else if (cmd == "shape") {
            lc_perf_batch b{};
            long long v[6];
            int nf;
            long long rdt, qdt;
            for (long long &x : v) std::cin >> x;
            std::cin >> nf >> rdt >> qdt;
            b.n = v[0]; b.n_matched = v[1]; b.t_min = v[2]; b.t_max = v[3]; b.x_min = v[4]; b.x_max = v[5]; b.n_f = nf;
            const lcp::PerfShape s = lcp::perf_shape(&b, rdt, qdt);
            std::printf("%d %lld %lld %lld %lld\n", s.rc, (long long)s.rate_first, (long long)s.rate_n, (long long)s.q_first,
                        (long long)s.q_n);
        } else if (cmd == "consts") {
            std::printf("%u %u %u %u %u\n", lcp::PERF_WG_RECORDS, lcp::PERF_TILE_BUCKETS, lcp::PERF_LDS_MAX, lcp::PERF_DIGIT_BITS,
                        lcp::PERF_LDS_SHARE);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
