# Window probe variants (host read of the loss after each window; no events)
# beside one bench line, same box.
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
for v in "1 0" "0 0" "1 1" "0 1"; do
  set -- $v
  WP_ITEM=$1 WP_EVENTS=$2 WP_WINDOWS=5 timeout -k 10 240 python3 -u scripts/window_probe.py 2>/dev/null | sed 's/ | steps.*//' >> $OUT/dip2.txt || exit 1
done
timeout -k 10 240 python3 bench.py --full --no-roofline --no-alt --no-cpu-baseline --no-sweep --steps 20 --warmup 5 > $OUT/dip2.json 2>/dev/null || exit 1
python3 -c "import json,sys; d=json.load(open(sys.argv[1])); print('bench', d['value'], d['runs_clips_s'])" $OUT/dip2.json >> $OUT/dip2.txt
