# whole-ResBlock kernel ablations (the DEBUG_FLAGS bits of csrc/diag.h: 16 no MRF epilogue,
# 32 x zeroed, 64 no operand writes, 2048 no lo-plane reads; 112 = 16 + 32 + 64).
# Needs a library built with HFG_EXTRA_FLAGS=-DHFG_ABLATE=1: the shipped build holds no
# ablation, and a flag set on it times the default schedule.
O=${OUT_DIR:-profiles/out}
mkdir -p $O
for f in 0 16 32 64 2048 112; do
  timeout -k 10 120 python bench.py --full --no-cpu-baseline --also --no-extra --steps 5 --sched DEBUG_FLAGS=$f > $O/abl_$f.json 2> $O/abl_$f.err || exit 1
done
