#!/bin/bash
# rocprofv3 summaries of the bench workload (run on an MI355X; the summaries go to $PROF_OUT, default build/prof):
#   1. kernel trace + stats of the driver's command (python bench.py --steps 20 --warmup 5), 2. the two HBM counters of the kernels
#   of the direct solve in their own passes on a shorter run (FETCH_SIZE and WRITE_SIZE do not fit one pass; counters are never
#   combined with tracing), 3. the bench lines with roofline and cpu_baseline (bench.py --full: default command and the driver's command).
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${1:-r05}
WL=${WORKLOAD:-cfg4}
ARGS=${BENCH_ARGS:---steps 20 --warmup 5 --no-cpu-baseline}
PMC_ARGS=${PMC_ARGS:---steps 3 --warmup 1 --no-cpu-baseline}
OUT=${PROF_OUT:-build/prof}   # the summaries; scripts/install_profiles.py reads them from the same folder
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -o ${TAG}_bench -- python bench.py --workload $WL $ARGS > $OUT/${TAG}_bench_stdout.log 2>&1
tail -1 $OUT/${TAG}_bench_stdout.log | cut -c1-300
rm -f $OUT/*kernel_trace.csv
for PAIR in "k_ds_gemm1=k_ds_gemm(_x)?<1" "k_ds_extend_panels=k_ds_extend_panels" "k_ds_gemm0=k_ds_gemm(_x)?<0" "k_ds_gj_flow=k_ds_gj_flow" "k_ds_gemv=k_ds_gemv"; do   # name=regex: the Schur / G GEMMs run as k_ds_gemm<mode, 4> and k_ds_gemm_x<mode, 4>
  KN=${PAIR%%=*}; KRN=${PAIR#*=}
  for CNT in FETCH_SIZE WRITE_SIZE; do
    rocprofv3 --pmc $CNT --kernel-include-regex "$KRN" --output-format csv -d $OUT -o ${TAG}_pmc_${KN}_$CNT -- python bench.py --workload $WL $PMC_ARGS > $OUT/${TAG}_pmc_stdout.log 2>&1
    python - <<PY
import csv, glob
for f in glob.glob("$OUT/**/${TAG}_pmc_${KN}_${CNT}_counter_collection.csv", recursive=True):
    rows = list(csv.DictReader(open(f)))
    vals = [float(r["Counter_Value"]) for r in rows if r.get("Counter_Name") == "$CNT"]
    if vals:
        line = f"$CNT kernel=$KRN dispatches={len(vals)} mean={sum(vals)/len(vals)} min={min(vals)} max={max(vals)} sum={sum(vals)}"
        print(line)
        open("$OUT/${TAG}_pmc_${KN}_${CNT}_summary.txt", "w").write(line + "\n")
    break
PY
    find $OUT -name "*counter_collection.csv" -delete
  done
done
python bench.py --full --workload $WL > $OUT/${TAG}_full_default.json 2> $OUT/${TAG}_full_default.err
python bench.py --full --workload $WL --steps 20 --warmup 5 > $OUT/${TAG}_full_driver.json 2> $OUT/${TAG}_full_driver.err
# scene groups next to the headline (S scenes of this GPU in lock step, merged factorisations): the multi_scene object of the same line
for S in 2 4; do
  python bench.py --workload $WL --steps 10 --warmup 3 --no-cpu-baseline --scenes-per-gpu $S > $OUT/${TAG}_multi_$S.json 2> $OUT/${TAG}_multi_$S.err
done
ls $OUT
