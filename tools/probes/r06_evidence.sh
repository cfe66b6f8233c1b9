# round 6 evidence set: bench lines of all four workloads, kernel tables, per-kernel counters  ->  <out>/<tag>_*
# usage: r06_evidence.sh <tag> <out>  (the kernel tables go where tools/prof_stats.sh puts them)
tag=${1:?usage: r06_evidence.sh <tag> <out>}
out=${2:?usage: r06_evidence.sh <tag> <out>}
mkdir -p $out
set -x
python bench.py --steps 20 --warmup 5 --full > $out/${tag}_bench.json 2> $out/${tag}_bench.err
python bench.py --workload beta --steps 20 --warmup 5 --full > $out/${tag}_bench_beta.json 2>/dev/null
python bench.py --workload n12 --steps 20 --warmup 5 --full > $out/${tag}_bench_n12.json 2>/dev/null
python bench.py --workload c5 --steps 5 --warmup 2 --full > $out/${tag}_bench_c5.json 2>/dev/null
bash tools/prof_stats.sh ${tag} > /dev/null 2>&1
bash tools/prof_stats.sh ${tag}_beta --workload beta > /dev/null 2>&1
bash tools/prof_stats.sh ${tag}_n12 --workload n12 > /dev/null 2>&1
bash tools/prof_stats.sh ${tag}_c5 --workload c5 --steps 3 --warmup 1 > /dev/null 2>&1
python tools/pmc_kernels.py $out/${tag}_kernels_pmc.json > $out/${tag}_pmc.log 2>&1
# the long window (the flow trains: three steps per walker where two did), the learned first-step table and the adjoint over it, kernel timeline of its last iterations
python bench.py --steps 200 --warmup 20 --full --no-extras > $out/${tag}_bench_200steps.json 2>/dev/null
python tools/probes/h_table_drift.py 2e-5 300 20 2>&1 | grep -v amdgpu.ids > $out/${tag}_h_table_drift.txt
( R=$PWD; O=$(cd $out && pwd); cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --output-format csv -d $O/${tag}_trace -- python3 $R/tools/probes/long_run.py 2e-5 260 > /dev/null 2>&1; f=$(ls $O/${tag}_trace/*/*kernel_trace.csv | head -1); python3 $R/tools/probes/pass_timeline.py $f 30 > $O/${tag}_iteration_timeline_late.txt; rm -rf $O/${tag}_trace )
python - <<PY
import json
for f in ("${tag}_bench","${tag}_bench_beta","${tag}_bench_n12","${tag}_bench_c5","${tag}_bench_200steps"):
    try:
        d=json.loads([l for l in open(f"$out/{f}.json") if l.startswith("{")][-1]); print(f, round(d["ms_per_step"],4), d["value"], d["stages_ms"], "frac", round(d["roofline"]["frac"],4), "traffic", d["roofline"].get("traffic"))
    except Exception as e: print(f, "failed", e)
PY
