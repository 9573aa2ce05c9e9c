# one variant's figures for A/B runs of the STARK openings kernel (scripts/ab_prebuilt.sh): serial event time of the openings per instance at n = 128 / 1024 / 4096
for n in 128 1024 4096; do
SIPP_BENCH_IO_SHARD_N= SIPP_BENCH_MAP_G2=0 SIPP_BENCH_OTHER_AIR=0 SIPP_BENCH_OUTER_PLONK=0 python3 bench.py --full --n $n --no-cpu-baseline --steps 2 --warmup 1 --inflight 1 2>/dev/null | python3 -c "
import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d['kernel_ms_serial']
print('n=$n', 'ms_per_step %.2f'%d['ms_per_step'], 'openings serial', k.get('openings'), 'verified', d['verified'])"
done
