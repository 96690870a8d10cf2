#!/bin/bash
export NAGP_DEVELOPER=1      # developer tool: libnagp.so reads its switches only with this set
# A/B of the forms of stage 1b in the IHGP ADF kernel on one box: NAGP_IH_TABLES = 0 (default: per-point moments straight from Q, v and the
# link tables, four barriers per step), 1 (tables e / t1 / ve on wave 1, q0 / s0 on workers 3, 4, five barriers).  Every GPU call under its
# own time limit; the script ends at the first one that does not return 0.
cd "$(dirname "$0")/.." || exit 1
for v in ${FORMS:-0 1 0 1 0 1}; do
  out=$(NAGP_IH_TABLES=$v timeout -k 10 300 python bench.py --workload cfg3 --steps 3 --warmup 1 --no-cpu-baseline --extras none 2>/dev/null) || { echo "NAGP_IH_TABLES=$v: bench.py failed -- stopping" >&2; exit 1; }
  echo "tables $v: $(echo "$out" | python -c 'import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print(d["ms_per_step"], d["value"])')"
done
for v in ${FORMS_STAMPS:-0 1}; do
  echo "== NAGP_IH_TABLES=$v"
  out=$(NAGP_STAMPS=1 NAGP_IH_TABLES=$v timeout -k 10 120 python tools/gpu_perf_probe.py cfg3 20000 2>&1) || { echo "probe failed -- stopping" >&2; exit 1; }
  echo "$out" | grep -a "worker wave" | head -2 | cut -c1-330
done
