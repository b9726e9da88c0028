# Same-box A/B on the GPU box: bench with the working tree's library (new) and the
# HEAD build (libhifigan_hip.so.old), alternated twice.  usage: bash profiles/ab_run.sh TAG [bench args]
# (bench.py --full: profiles/ab_show.py prints the per-kernel figures; output in $OUT_DIR,
#  default profiles/out)
T=${1:-ab}; shift
L=tts-sambert_hifigan_amd/libhifigan_hip.so
O=${OUT_DIR:-profiles/out}
mkdir -p $O
cp $L /tmp/ab_new.so
for i in 1 2; do
  cp /tmp/ab_new.so $L && timeout -k 10 150 python bench.py --full --also --no-extra --no-cpu-baseline --steps 20 "$@" > $O/${T}_new$i.json 2>/dev/null || exit 1
  cp $L.old $L && timeout -k 10 150 python bench.py --full --also --no-extra --no-cpu-baseline --steps 20 "$@" > $O/${T}_old$i.json 2>/dev/null || exit 1
done
cp /tmp/ab_new.so $L
