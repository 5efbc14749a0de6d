#!/bin/bash
# run bench.py (short) once per library variant in build/variants; prints key timings per variant (results under $OUT)
OUT=${OUT:-tool_out}
mkdir -p $OUT
for so in build/variants/*.so; do
  name=$(basename $so .so)
  OCTREELIB_AMD_LIB=$PWD/$so python bench.py --full --steps 6 --warmup 2 --no-cpu-baseline > $OUT/ab_$name.json 2> $OUT/ab_$name.err || echo "FAILED $name"
done
OUT=$OUT python - <<'PY'
import json, glob, os
for f in sorted(glob.glob(os.environ['OUT'] + '/ab_*.json')):
    try:
        d = json.load(open(f)); k = d['kernels']
        print(os.path.basename(f)[3:-5], 'step %.2f ms' % d['ms_per_step'], 'ransac %.3f' % k['ransac']['ms_per_step'],
              'keygen %.3f' % k['keygen']['ms_per_step'], 'build-only %.3f' % d.get('secondary', {}).get('insert_subdivide_only', {}).get('ms', 0),
              'kept', d['config']['points_after_ransac'])
    except Exception as e:
        print(f, 'ERR', e)
PY
