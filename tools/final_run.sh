# The closing checks in one go: GPU tests, smoke(), the full bench line, the Burgers lines, the parity report, the profiles.
#   bash tools/final_run.sh [OUT_DIR]        (default OUT_DIR: final_out/ in the repository root)
cd "$(dirname "$0")/.."
O=${1:-final_out}
mkdir -p $O
( timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -8 ) > $O/gpu_tests.log 2>&1
( timeout 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -3 ) > $O/smoke.log 2>&1
( timeout 900 python bench.py --full 2>&1 | tail -1 ) > $O/bench.json 2>$O/bench.err
( timeout 300 python bench.py --workload burgers --no-cpu-baseline --no-extras 2>&1 | tail -1 ) > $O/bench_burgers.json
( timeout 300 python bench.py --workload burgers-bf16 --no-cpu-baseline --no-extras 2>&1 | tail -1 ) > $O/bench_burgers_bf16.json
( timeout 900 python tools/parity_report.py --out $O/parity_report.json 2>&1 | tail -15 ) > $O/parity.log 2>&1
bash tools/run_profile_r02.sh > $O/profile.log 2>&1
tail -3 $O/gpu_tests.log; cat $O/smoke.log; cut -c1-400 $O/bench.json
