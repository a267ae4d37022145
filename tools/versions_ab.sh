#!/bin/bash
# the moving-model leg of bench.py (a model moved before every frame) for several ArtTuning settings, e.g. the depth of the ring of structure versions:
#   bash tools/versions_ab.sh <steps> "as_versions=3" "as_versions=4" "" ...
S=$1; shift
OUT=$(mktemp -d)
for i in 1 2; do for t in "$@"; do
  python bench.py --full --steps $S --warmup 5 --no-cpu-baseline ${t:+--tuning $t} > $OUT/vab.json 2> $OUT/vab.err || { tail -5 $OUT/vab.err; exit 1; }
  python -c "
import json; d=json.load(open('$OUT/vab.json')); m=d['moving_model']; print('${t:-default}', 'static', round(d['value']), 'moving', round(m['value']), 'Mray/s', round(m['ms_per_step'], 4), 'ms  refit_ms', m.get('refit_ms'), flush=True)"
done; done
