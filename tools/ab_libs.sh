#!/bin/bash
# A/B of two builds of libart on one box, alternating: [PAIRS=n] [NEW_TUNING=k=v,...] bash tools/ab_libs.sh <base.so> <new.so> [bench.py arguments ...]   (default: 2 pairs, config 2, 1000 steps)
# NEW_TUNING adds a third arm to every round: the new build under that ArtTuning setting (shadow_hints=1: the new build with its hints off, which has to sit inside the base's range).
# The summary says whether the ranges overlap: a gain counts only if every run of the new build beats every run of the base in this one call (machines differ by up to 8 %).
A=$1; B=$2; shift 2
ARGS=${@:---steps 1000 --warmup 50}
OUT=${AB_OUT:-$(mktemp -d)}   # AB_OUT: where the runs' lines are kept (default: a temporary directory)
mkdir -p $OUT; export OUT
: > $OUT/ab_runs.txt
for i in $(seq ${PAIRS:-2}); do for arm in base new ${NEW_TUNING:+new_tuned}; do
  L=$B; T=""; [ $arm = base ] && L=$A; [ $arm = new_tuned ] && T="--tuning $NEW_TUNING"
  ART_LIB_PATH=$PWD/$L timeout -k 10 300 python bench.py --plain $ARGS $T > $OUT/ab.json 2> $OUT/ab.err || { tail -5 $OUT/ab.err; exit 1; }
  python -c "
import json; d=json.load(open('$OUT/ab.json')); print('$arm', '$L', '$T', round(d['value'], 1), 'Mray/s', round(d['ms_per_step'], 4), 'ms', flush=True); open('$OUT/ab_runs.txt', 'a').write('$arm %r\n' % d['value'])"
done; done
python - <<'EOF'
import os
import statistics as st
runs = {}
for l in open(os.environ['OUT'] + '/ab_runs.txt'):
    k, v = l.split(); runs.setdefault(k, []).append(float(v))
for k, v in runs.items():
    print(f"{k:9s} min {min(v):9.1f} median {st.median(v):9.1f} max {max(v):9.1f} Mray/s  spread {100 * (max(v) / min(v) - 1):.2f} %")
b, n = runs['base'], runs['new']
print(f"new / base: median ratio {st.median(n) / st.median(b):.4f}; every new run beats every base run: {min(n) > max(b)}; every base run beats every new run: {min(b) > max(n)}")
if 'new_tuned' in runs:
    t = runs['new_tuned']
    print(f"new_tuned / base: median ratio {st.median(t) / st.median(b):.4f}; inside the base's range: {min(b) <= st.median(t) <= max(b)}")
EOF
