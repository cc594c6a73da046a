# Round-1 evidence run: GPU parity tests, the C2 bench line, a rocprofv3
# kernel-trace summary of the same bench command, and FETCH/WRITE_SIZE passes.
# Logs and profiles go under $O (default bench_out/, git-ignored).
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
O=${O:-bench_out}
mkdir -p $O/prof
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $O/gpu_tests.log 2>&1 || { echo TESTS_FAILED; tail -30 $O/gpu_tests.log; exit 1; }
tail -1 $O/gpu_tests.log
timeout -k 10 300 python bench.py --full --steps 50 --warmup 5 > $O/bench_c2.log 2>&1 || { echo BENCH_FAILED; tail -20 $O/bench_c2.log; exit 1; }
tail -1 $O/bench_c2.log | cut -c1-300
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof/kt -o kt --output-format csv -- python3 bench.py --full --steps 50 --warmup 5 --no-cpu > $O/prof/kt.log 2>&1 || { echo PROF_FAILED; tail -20 $O/prof/kt.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $O/prof/fetch -o f --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu > $O/prof/f.log 2>&1 || { echo PMC1_FAILED; tail -5 $O/prof/f.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $O/prof/write -o w --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu > $O/prof/w.log 2>&1 || { echo PMC2_FAILED; tail -5 $O/prof/w.log; exit 1; }
find $O/prof -name "*.csv" | head -20
timeout -k 10 300 python bench.py --full --config C5 --steps 20 --warmup 3 > $O/bench_c5.log 2>&1 || { echo C5_FAILED; tail -5 $O/bench_c5.log; exit 1; }
timeout -k 10 300 python bench.py --full --config C4 --budget 65536 --steps 3 --warmup 1 > $O/bench_c4.log 2>&1 || { echo C4_FAILED; tail -5 $O/bench_c4.log; exit 1; }
timeout -k 10 300 python bench.py --full --config C3 --keys 20000 --steps 5 --warmup 1 --no-cpu > $O/bench_c3s.log 2>&1 || { echo C3_FAILED; tail -5 $O/bench_c3s.log; exit 1; }
timeout -k 10 300 python bench.py --full --config C1 --steps 20 --warmup 3 > $O/bench_c1.log 2>&1 || { echo C1_FAILED; tail -5 $O/bench_c1.log; exit 1; }
tail -1 $O/bench_c1.log | cut -c1-300
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof/kt4 -o kt4 --output-format csv -- python3 bench.py --full --config C4 --budget 65536 --steps 3 --warmup 1 --no-cpu > $O/prof/kt4.log 2>&1 || { echo PROF4_FAILED; tail -20 $O/prof/kt4.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc FETCH_SIZE -d $O/prof/fetch4 -o f4 --output-format csv -- python3 bench.py --full --config C4 --budget 65536 --steps 2 --warmup 1 --no-cpu > $O/prof/f4.log 2>&1 || { echo PMC41_FAILED; tail -5 $O/prof/f4.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc WRITE_SIZE -d $O/prof/write4 -o w4 --output-format csv -- python3 bench.py --full --config C4 --budget 65536 --steps 2 --warmup 1 --no-cpu > $O/prof/w4.log 2>&1 || { echo PMC42_FAILED; tail -5 $O/prof/w4.log; exit 1; }
timeout -s KILL 120 rocprofv3 --pmc TCC_EA0_ATOMIC_sum -d $O/prof/atom4 -o a4 --output-format csv -- python3 bench.py --full --config C4 --budget 65536 --steps 2 --warmup 1 --no-cpu > $O/prof/a4.log 2>&1 || { echo PMC43_FAILED; tail -5 $O/prof/a4.log; exit 1; }
echo ALL_OK
