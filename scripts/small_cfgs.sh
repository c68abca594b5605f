set -e
OUT=${OUT:-runs}; mkdir -p $OUT
for w in "complex csr" "complex auto" "banded auto" "poisson2d auto"; do
  set -- $w
  python bench.py --workload $1 --stream $2 --full --no-cpu-baseline --no-also --steps 500 --warmup 50 > $OUT/small_$1_$2.json 2> $OUT/small_$1_$2.err || { tail -5 $OUT/small_$1_$2.err; exit 1; }
  python - $1 $2 $OUT/small_$1_$2.json <<'PY'
import json, sys
j = json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
r = j["roofline"]
print(sys.argv[1], sys.argv[2], "%.0f it/s  %.2f us/iteration" % (j["value"], j["ms_per_step"] * 1e3), "spmv %.2f us" % r["avg_launch_us"], "frac %.3f" % r["frac"], j["timing"].get("profiled_pass", {}).get("ms_per_step_with_events"))
PY
done
