# A/B of stereo extraction (--mode extract) and config 5 (--mode batch) under environment settings:
# bash tools/exab.sh "VAR=VAL ..." ...   ("X=1" = the defaults); results in $AB_OUT/exab.txt (default ab/exab)
# (--full: the summary reads the batch mode's stage times)
set -o pipefail
OUT=${AB_OUT:-ab/exab}
mkdir -p $OUT
for i in 1 2; do
for v in "$@"; do
  for m in extract batch; do
    env $v timeout -k 10 200 python bench.py --full --mode $m --steps 100 --warmup 20 --no-cpu-baseline > $OUT/run.log 2>&1 || exit 1
    echo "$m $v: $(tail -1 $OUT/run.log | python -c 'import json,sys; d=json.load(sys.stdin); print(d["value"], d["ms_per_step"], d.get("stage_ms_per_launch"))')" | tee -a $OUT/exab.txt
  done
done; done
