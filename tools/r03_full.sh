# round-3 closing run on one MI355X: the whole GPU suite, the default bench line, the multi-rank legs rehearsed, the three rocprofv3 passes, the rows
# usage: tools/r03_full.sh OUTDIR   (logs and lines go there; the profile scripts keep their own output folder and print their summaries into the logs)
OUT=${1:?usage: tools/r03_full.sh OUTDIR}
mkdir -p "$OUT"
TMLQCD_HIP_FLAG_TIMEOUT_S=20 timeout -k 10 900 python -m pytest tests -x -q -m gpu --timeout 400 --timeout-method=thread > "$OUT/r03_gpu_all.log" 2>&1
tail -4 "$OUT/r03_gpu_all.log"
timeout -k 10 400 python bench.py --full > "$OUT/r03_bench_n1.json" 2> "$OUT/r03_bench_n1.err" || { echo "bench failed"; tail -20 "$OUT/r03_bench_n1.err"; }
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print({k: d[k] for k in ('value','ms_per_step','cg_16')}, d['roofline']['frac'], d['cg']['iters_per_s'], d['cpu_baseline']['value'], d.get('parity_max_rel_err_vs_cpu'), d['next_rows'])" "$OUT/r03_bench_n1.json"
TMLQCD_HIP_FLAG_TIMEOUT_S=20 timeout -k 10 500 python bench.py --full --loopback 2 --rehearse-split --no-cpu --no-rows --steps 100 --warmup 10 --cg-iters 25 > "$OUT/r03_bench_rehearse.json" 2> "$OUT/r03_bench_rehearse.err" || { echo "rehearse failed"; tail -20 "$OUT/r03_bench_rehearse.err"; }
python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['rank_check']['ok'], d['strong']['value'], d['strong_32']['value'], d['strong_32']['rank_check']['ok'])" "$OUT/r03_bench_rehearse.json"
bash tools/profile.sh r03 > "$OUT/r03_profile.log" 2>&1; grep -A12 "^# rocprofv3 summary" "$OUT/r03_profile.log"
bash tools/profile_rows.sh r03 > "$OUT/r03_profile_rows.log" 2>&1; tail -16 "$OUT/r03_profile_rows.log"
