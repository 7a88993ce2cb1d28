#!/bin/bash
set -eo pipefail  # every GPU step has a time limit; the first failure or time limit ends the script
for o in 2 4 5; do echo "== CGRT_FAST_OPEN=$o"; CGRT_FAST_OPEN=$o timeout -k 10 300 python tools/measure_config3.py dragon800k; CGRT_FAST_OPEN=$o timeout -k 10 300 python bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --no-extras 2>/dev/null | python -c "import sys,json; j=json.loads(sys.stdin.read()); print(j['value'], j['roofline']['kernel_ms'], j['roofline']['per_ray_entering_tree'], j['config']['bvh_build_and_upload_s'])"; done
