set -o pipefail
# six fresh processes back to back: headline, unramped and causal TF/s of each (results in $OUT, default out/ramp)
OUT=${OUT:-out/ramp}
mkdir -p "$OUT"
for i in 1 2 3 4 5 6; do
  timeout -k 10 150 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/b$i.json" 2> "$OUT/b$i.err" || exit $?
  python3 -c "import json;d=json.loads(open('$OUT/b$i.json').read().strip().splitlines()[-1]);print($i, round(d['value'],1), round(d['unramped']['TFLOP/s'],1), round(d['flash_causal']['TFLOP/s'],1), flush=True)"
done
