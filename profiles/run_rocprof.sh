# rocprofv3 kernel-trace stats + separate FETCH_SIZE / WRITE_SIZE passes of bench.py
# (PMC passes carry no trace domains: MI355X_MICROARCH.md §HBM / gpurun rules).
# usage on the GPU box:  bash profiles/run_rocprof.sh <tag>
# (--streams 1: per-dispatch durations match bench.py's 1-stream roofline pass; --no-pmc:
#  bench.py's own live PMC child passes are not started under the profiler)
# The first pass runs bench.py --full: its JSON carries the per-kernel HIP-event figures the
# rocprofv3 averages are compared with.  Output goes to $OUT_DIR (default profiles/out).
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
T=${1:-cur}
O=${OUT_DIR:-$R/profiles/out}
mkdir -p $O
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$T -o run --output-format csv -- python $R/bench.py --full --steps 5 --warmup 2 --also --no-cpu-baseline --no-extra --no-pmc --streams 1 > $O/prof_${T}_bench.json 2> $O/prof_${T}_bench.err && \
timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE -d $O/pmc_fetch_$T -o run --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --streams 1 > $O/pmc_fetch_$T.log 2>&1 && \
timeout -k 10 300 rocprofv3 --pmc WRITE_SIZE -d $O/pmc_write_$T -o run --output-format csv -- python $R/bench.py --steps 2 --warmup 1 --streams 1 > $O/pmc_write_$T.log 2>&1
