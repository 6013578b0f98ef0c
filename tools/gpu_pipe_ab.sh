cd /tmp && export TMPDIR=/tmp && cd $REPO_ROOT && mkdir -p bench_out
for p in 3 4 2 3; do
  timeout -k 10 400 python bench.py --full --no-e2e --no-side-configs --no-cpu-baseline --no-pcie --no-fastq --steps 100 --warmup 10 --pipeline $p > bench_out/pipe_$p.json 2> bench_out/pipe_$p.err || exit $?
  python3 -c "import json; d=json.loads(open('bench_out/pipe_$p.json').read().strip().splitlines()[-1]); print($p, d['ms_per_step'], d['one_stream_ms_per_step'], d['sync_plan_ms_per_step'])"
done
