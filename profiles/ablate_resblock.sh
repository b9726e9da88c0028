O=${OUT_DIR:-profiles/out}
mkdir -p $O
for f in 0 16 32 64 128 240; do
  HFG_DEBUG_FLAGS=$f timeout -k 10 120 python bench.py --full --no-cpu-baseline --also --no-extra --steps 5 > $O/abl_$f.json 2> $O/abl_$f.err || exit 1
done
