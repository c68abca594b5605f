# same box: cfg 3 / cfg 4 with M3 inside M1 (default) and without (spmv_fuse=0)
OUT=${OUT:-runs}; mkdir -p $OUT
for w in "complex" "banded"; do
  for f in 0 -1 1 0 -1 1; do
    python bench.py --workload $w --full --no-cpu-baseline --no-also --steps 500 --warmup 50 --set spmv_fuse=$f > $OUT/mf_${w}_$f.json 2> $OUT/mf_${w}_$f.err || { tail -5 $OUT/mf_${w}_$f.err; exit 1; }
    python - $w $f $OUT/mf_${w}_$f.json <<'PY'
import json, sys
j = json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
r = j["roofline"]
print(sys.argv[1], "spmv_fuse", sys.argv[2], "%.0f it/s  %.2f us/iteration" % (j["value"], j["ms_per_step"] * 1e3), "| SpMV launch %.2f us" % r["avg_launch_us"], "frac %.3f" % r["frac"])
PY
  done
done
