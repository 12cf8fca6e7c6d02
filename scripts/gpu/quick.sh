# quick loop: MLP kernel parity tests + the per-kernel timings of the bench workload, the render and
# north-star legs (bench.py --full, the other legs off):   bash scripts/gpu/quick.sh OUTDIR
OUT=${1:?usage: bash scripts/gpu/quick.sh OUTDIR}
mkdir -p $OUT
python -m pytest tests/test_kernels_gpu.py tests/test_pipeline_gpu.py -m gpu -q -x -k "mlp or nerf or fit or step or wide" > $OUT/pytest.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest.log
tail -3 $OUT/pytest.log
python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-config3 --no-config5 --no-skip-leg --no-bf16-leg ${BENCH_EXTRA} > $OUT/bench.json 2> $OUT/bench.err
python - $OUT/bench.json <<'PY'
import json, sys
b = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
print("ms/step", round(b["ms_per_step"], 3), "rays/s", round(b["value"]))
for k, v in b["kernels"].items(): print(" ", k, v["avg_ms"], v["frac"])
if b.get("render"): print("  render fps", b["render"]["kernels_only_fps"], b["render"]["value"])
if b.get("north_star_shape"):
    n = b["north_star_shape"]; print("  north star", n["mlp_ms"], n["frac"], {k: (v["avg_ms"], v["frac"]) for k, v in n["kernels"].items()})
PY
