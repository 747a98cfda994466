set -x
O=${OUT:-scratch/alias}; mkdir -p $O
python -m pytest tests/test_gpu_api.py -x -q -k "aliasing or in_flight or autotune_pair" 2>&1 | tail -5
python bench.py --full --no-alias-workspace --save-tiles $O/tiles.json > $O/plain2.json 2> $O/plain2.err
python bench.py --full --load-tiles $O/tiles.json --alias-workspace > $O/alias2.json 2> $O/alias2.err
python bench.py --full --load-tiles $O/tiles.json --in-flight 1 --no-alias-workspace > $O/plain1.json 2>/dev/null
python bench.py --full --load-tiles $O/tiles.json --in-flight 1 --alias-workspace > $O/alias1.json 2>/dev/null
python bench.py --full --load-tiles $O/tiles.json --alias-workspace --in-flight 3 > $O/alias3.json 2>/dev/null
python bench.py --full --no-alias-workspace --load-tiles $O/tiles.json > $O/plain2b.json 2>/dev/null
python bench.py --full --load-tiles $O/tiles.json --alias-workspace > $O/alias2b.json 2>/dev/null
python bench.py --full --alias-workspace > $O/alias2_owntune.json 2>/dev/null
for f in plain2 alias2 plain1 alias1 alias3 plain2b alias2b alias2_owntune; do python - $O $f <<'PY'
import json,sys
d=json.loads(open(f'{sys.argv[1]}/{sys.argv[2]}.json').read().strip().splitlines()[-1])
print(sys.argv[2], d['value'], d['ms_per_step'], d.get('single_stream_value'), d['roofline']['frac'], d.get('activation_workspace_bytes'), d['outputs_sha256'][:12])
PY
done
