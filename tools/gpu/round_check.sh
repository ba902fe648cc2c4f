# Full GPU check of the tree: GPU tests, default bench, config sweep, window kernel profile
#   O=<output directory> bash tools/gpu/round_check.sh
set -o pipefail
O=${O:?set O to the output directory}
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gputest.log 2>&1 || { tail -40 $O/gputest.log; exit 1; }
tail -1 $O/gputest.log
timeout -k 10 180 python bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
python3 -c "import json; j=json.load(open('$O/bench.json')); print('bench', j['ms_per_step'], j['value'], j['verified'], j['roofline']['kernel_ms'])"
timeout -k 10 300 python tools/config_sweep.py $O/configs_1gpu.json > $O/configs.log 2>&1 || { tail -20 $O/configs.log; exit 1; }
tail -12 $O/configs.log
bash tools/gpu/window_prof.sh
