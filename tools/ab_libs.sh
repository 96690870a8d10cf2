#!/bin/bash
export NAGP_DEVELOPER=1      # developer tool: libnagp.so reads its switches only with this set
# same-box A/B of several builds of libnagp.so: tools/ab_libs.sh "bench args" rounds lib1.so lib2.so ...
# The candidates are selected through NAGP_LIB (nagp/_lib.py); the in-tree library is never touched.
# Prints ms_per_step and kernel_ms_per_step.filter of every run.  Every bench.py call runs under its own time limit
# (AB_TIMEOUT seconds, default 300), and the script ends at the first call that does not return 0: nothing is started
# on a GPU that has just faulted or hung.
cd "$(dirname "$0")/.." || exit 1
args="$1"; rounds=$2; shift 2
for r in $(seq 1 $rounds); do for which in "$@"; do
  out=$(NAGP_LIB="$(realpath "$which")" timeout -k 10 "${AB_TIMEOUT:-300}" python bench.py $args --no-cpu-baseline --extras none 2>/dev/null)
  st=$?
  if [ $st -ne 0 ]; then echo "$(basename $which) [$args]: bench.py exit status $st -- stopping" >&2; exit $st; fi
  echo "$(basename $which) [$args]: $(echo "$out" | python -c 'import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d.get("kernel_ms_per_step") or {}; print(round(d["ms_per_step"],1), "filter", round(k.get("filter", float("nan")),1))')" || exit 1
done; done
