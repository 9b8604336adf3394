export OUT=${OUT:-probe_out}; mkdir -p "$OUT/exp1"
for v in 0 1; do
  HIP_FORCE_DEV_KERNARG=$v python bench.py --full --steps 200 --warmup 20 --no-secondary --no-cpu-baseline > $OUT/exp1/kernarg$v.json 2> $OUT/exp1/kernarg$v.err
  python - <<P
import json
d=json.loads(open('$OUT/exp1/kernarg$v.json').read().strip().splitlines()[-1])
print('KERNARG=$v', d['ms_per_step'], d['no_prefetch']['ms_per_step'], d['eager_ms_per_step'], d['kernel_us'])
P
done
