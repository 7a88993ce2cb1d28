#!/bin/bash
set -eo pipefail  # every GPU step has a time limit; the first failure or time limit ends the script
for lib in libcgrt.so libcgrt_oldloop.so; do
  echo "== $lib exact walk, bench frame"
  CGRT_LIB_NAME=$lib timeout -k 10 300 python bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --walk exact 2>/dev/null | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(j['value'], j['roofline']['kernel_ms'])"
  echo "== $lib config 3 + dragon shaded"
  CGRT_LIB_NAME=$lib timeout -k 10 300 python tools/measure_config3.py
done
