# schedules against each other on one box, alternating: the shipped one, a candidate file ($1, e.g. scripts/vote_schedule.py's output copied
# into the tree, such as scratch/) and a fresh autotune (img/s two in flight, ms/step, single-stream img/s, conv-family frac)
CAND=${1:-}
O=${OUT:-scratch/sched}; mkdir -p $O
for r in 1 2 3; do
python bench.py --full --no-cpu-baseline > $O/h_ship$r.json 2>/dev/null
if [ -n "$CAND" ]; then python bench.py --full --no-cpu-baseline --load-tiles $CAND > $O/h_cand$r.json 2>/dev/null; fi
python bench.py --full --retune --no-cpu-baseline --save-tiles $O/retuned_$r.json > $O/h_tune$r.json 2>/dev/null
done
for f in h_ship1 h_cand1 h_tune1 h_ship2 h_cand2 h_tune2 h_ship3 h_cand3 h_tune3; do [ -f $O/$f.json ] && python - $O $f <<'PY'
import json,sys
d=json.loads(open(f'{sys.argv[1]}/{sys.argv[2]}.json').read().strip().splitlines()[-1])
print(sys.argv[2], d['value'], d['ms_per_step'], d.get('single_stream_value'), d['roofline']['frac'], d['schedule'][:40])
PY
done
