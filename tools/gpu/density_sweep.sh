# Fixed-density sweep of the bench (roofline, dense-SDPA speedup and quality per density: --full).
# Usage (from the repo root): bash tools/gpu/density_sweep.sh OUTDIR
set -o pipefail
OUT=${1:?usage: density_sweep.sh OUTDIR}
mkdir -p $OUT
for d in 0.7 0.5 0.3; do
  timeout -k 10 300 python bench.py --full --density $d --no-cpu-baseline --no-pmc > $OUT/cog_d$d.json 2> $OUT/cog_d$d.err || exit 1
  echo "cog $d: $(cut -c1-200 $OUT/cog_d$d.json)"
done
for d in 0.5 0.3; do
  timeout -k 10 300 python bench.py --full --variant wan --density $d --no-cpu-baseline --no-pmc > $OUT/wan_d$d.json 2> $OUT/wan_d$d.err || exit 1
  echo "wan $d done"
done
