# native closed loop (bench --mode system) on two library builds, alternating: bash tools/sys_ab.sh LIB_A LIB_B
# (logs and summary.txt in $AB_OUT, default ab/sysab; --full: the summary reads the synchronous loop's rate)
OUT=${AB_OUT:-ab/sysab}
mkdir -p $OUT
for i in 1 2; do
  for L in "$@"; do
    n=$(basename $L .so)
    ORBMI_LIB=$L timeout -k 10 400 python bench.py --full --mode system --no-cpu-baseline > $OUT/${n}_$i.log 2>&1 || exit $?
    tail -1 $OUT/${n}_$i.log | python -c 'import json,sys; d=json.load(sys.stdin); print("'$n'", d["value"], d["ate_rmse_m"], d["phase_ms_per_frame"], d["synchronous_local_mapping"]["frames_per_s"])' | tee -a $OUT/summary.txt
  done
done
