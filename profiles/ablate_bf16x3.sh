# bf16x3 kernel ablations (the DEBUG_FLAGS bits of csrc/diag.h): per-kernel ms for each flag set.
# Needs a library built with HFG_EXTRA_FLAGS=-DHFG_ABLATE=1: the shipped build holds no
# ablation, and a flag set on it times the default schedule.  Each JSON's "config" records the
# override it ran under (schedule_overrides).
# usage: bash profiles/ablate_bf16x3.sh TAG "0 1 4 8 128 4096"
T=${1:-abl}
O=${OUT_DIR:-profiles/out}
mkdir -p $O
for f in ${2:-0 1 4 8 128 4096 16384 32768 65536}; do
  timeout -k 10 120 python bench.py --full --steps 5 --warmup 2 --precision bf16x3 --no-cpu-baseline --no-extra --also --sched DEBUG_FLAGS=$f > $O/${T}_$f.json 2>/dev/null || exit 1
done
