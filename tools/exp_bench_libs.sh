#!/bin/bash
set -eo pipefail  # every GPU step has a time limit; the first failure or time limit ends the script
# bench the default library and experiment builds (cg-raytracer_amd/lib/libcgrt_<name>.so)
for lib in "$@"; do
  echo "== $lib"
  CGRT_LIB_NAME=$lib timeout -k 10 300 python bench.py --full --steps 30 --warmup 3 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(j['value'], j['roofline']['kernel_ms'], j['roofline']['per_ray'])"
done
