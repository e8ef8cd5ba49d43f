# the full benchmark (the driver's command with --full); every JSON line's leg name and size, then the final line
OUT=${OUT:-/tmp/bench_lines}
mkdir -p $OUT
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_full_cmd.out 2> $OUT/bench_full_cmd.err
echo "rc=$?"
grep -v amdgpu.ids $OUT/bench_full_cmd.err | tail -5
OUT=$OUT python - <<'P'
import json, os
for line in open(os.path.join(os.environ["OUT"], "bench_full_cmd.out")):
    if not line.startswith("{"):
        continue
    d = json.loads(line)
    print(len(line), d.get("leg", "FINAL"), d.get("error", ""))
print(line[:6000])
P
