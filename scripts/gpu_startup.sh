# the driver's command with its steady-state leg and HIP-event pass (--full, twice) + the start-up probe
OUT=${OUT:-/tmp/startup}
mkdir -p $OUT
for i in 1 2; do python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --no-secondary --no-cpu-baseline 2>&1 | grep -v amdgpu.ids | tail -1 > $OUT/driver_cmd_$i.json; done
python3 bench.py --full --no-secondary --no-cpu-baseline 2>&1 | grep -v amdgpu.ids | tail -1 > $OUT/default_200.json
python3 scripts/startup_probe.py inbatch 2>&1 | grep -v amdgpu.ids > $OUT/probe_inbatch.jsonl
for f in $OUT/driver_cmd_1.json $OUT/driver_cmd_2.json $OUT/default_200.json; do python3 -c "
import json,sys; d=json.load(open('$f')); print('$f', d['value'], d['ms_per_step'], d['roofline']['steady_ms_per_step'])"; done
cut -c1-1500 $OUT/probe_inbatch.jsonl
