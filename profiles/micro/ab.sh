#!/bin/bash
# A/B of two builds of the library ON THE SAME BOX (boxes differ by +-1.5 %, so numbers from different runs do
# not compare):  bash profiles/micro/ab.sh liblsf_hip_base.so liblsf_hip.so   (files under levelsetfortran_amd/)
D=${AB_OUT:-${TMPDIR:-/tmp}}
for rep in 1 2; do
for lib in "$@"; do
  LSF_LIB_PATH=$PWD/levelsetfortran_amd/$lib timeout -k 10 300 python bench.py --full --no-cpu-baseline > "$D/ab.json" 2> "$D/ab.err"
  python -c "import json;d=json.load(open('$D/ab.json'));print('$lib', 'gs ms/step', round(d['ms_per_step'],4), 'jacobi ms/step', round(d['jacobi']['ms_per_step'],4), 'jacobi kernel us', round(d['jacobi']['roofline']['avg_launch_us'],1))"
done; done
