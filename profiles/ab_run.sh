# Same-box A/B on the GPU box: bench with the working tree's library (new) and the
# HEAD build (libhifigan_hip.so.old), alternated ROUNDS times (default 2).
# usage: [ROUNDS=3] [DUMP=1] bash profiles/ab_run.sh TAG [bench args]
# (bench.py --full: profiles/ab_show.py prints the per-kernel figures and, with DUMP=1, compares
#  the dumped wav.npy of every run; output in $OUT_DIR, default profiles/out)
T=${1:-ab}; shift
L=tts-sambert_hifigan_amd/libhifigan_hip.so
O=${OUT_DIR:-profiles/out}
mkdir -p $O
cp $L /tmp/ab_new.so
for i in $(seq ${ROUNDS:-2}); do
  for v in old new; do
    if [ $v = old ]; then cp $L.old $L; else cp /tmp/ab_new.so $L; fi
    D=""; [ -n "$DUMP" ] && D="--dump-outputs $O/${T}_$v$i"
    timeout -k 10 150 python bench.py --full --also --no-extra --no-cpu-baseline --steps 20 "$@" $D > $O/${T}_$v$i.json 2>/dev/null || { cp /tmp/ab_new.so $L; exit 1; }
  done
done
cp /tmp/ab_new.so $L
