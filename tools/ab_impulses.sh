#!/bin/bash
# Velocity impulses, timing. No table: interleaved A/B of bench.py between this tree and a built checkout of the parent commit
# on one box (devices differ by several per cent, so only runs of one call compare). With a table: tools/time_impulses.py on
# this tree (K = 20 in one launch against 20 launches with adds). Everything goes to <outdir>/impulses_ab.txt, headed by the
# two commit ids: that file is profiles/impulses_ab.txt. usage (GPU box, from the repository root):
#   tools/ab_impulses.sh <outdir> <reps> <parent_tree> <parent_commit> <this_commit> [bench.py arguments, default: --full]
set -o pipefail
OUT=$1; REPS=$2; PARENT=$3; PARENT_ID=$4; THIS_ID=$5; shift 5
ARGS=${*:---full}
mkdir -p "$OUT" || exit 1
OUT=$(cd "$OUT" && pwd)
HERE=$PWD
TXT="$OUT/impulses_ab.txt"
{
  echo "# velocity impulses: A/B without a table against the parent, timing with a table (tools/ab_impulses.sh)"
  echo "# parent $PARENT_ID"
  echo "# this   $THIS_ID"
  echo "# one MI355X, one session; bench.py --gpus 1 --steps 500 --warmup 500 $ARGS, $REPS interleaved repetitions"
} > "$TXT"
for rep in $(seq "$REPS"); do
  for v in parent this; do
    if [ $v = parent ]; then cd "$PARENT" || exit 1; else cd "$HERE" || exit 1; fi
    timeout -k 10 900 python3 bench.py --gpus 1 --steps 500 --warmup 500 $ARGS > "$OUT/bench_${v}_$rep.json" 2>"$OUT/err_${v}_$rep.log"
    rc=$?
    if [ $rc -ne 0 ]; then tail -5 "$OUT/err_${v}_$rep.log"; echo "bench.py ($v, rep $rep) rc=$rc"; exit $rc; fi
    tail -1 "$OUT/bench_${v}_$rep.json" | python3 -c "
import json, sys
r = json.loads(sys.stdin.read())
def flat(d, pre=''):
    for k in sorted(d):
        if isinstance(d[k], dict):
            yield from flat(d[k], pre + k + '.')
        elif isinstance(d[k], (int, float)) and not isinstance(d[k], bool) and 'ms' in k:
            yield '%s%s=%.5f' % (pre, k, d[k])
print('%-6s rep%s ' % ('$v', '$rep') + ' '.join(flat(r)))" | tee -a "$TXT"
    rc=$?
    if [ $rc -ne 0 ]; then echo "summary of bench.py ($v, rep $rep) rc=$rc"; exit $rc; fi
  done
done
cd "$HERE" || exit 1
echo "# with a table, fp32, K = 20 (tools/time_impulses.py): ms per step" >> "$TXT"
timeout -k 10 600 python3 tools/time_impulses.py --steps 20 --batches 65536 4096 --reps 5 2>"$OUT/err_impulses_on.log" | tee -a "$TXT"
rc=$?
if [ $rc -ne 0 ]; then tail -5 "$OUT/err_impulses_on.log"; echo "time_impulses.py rc=$rc"; exit $rc; fi
