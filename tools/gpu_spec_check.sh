#!/bin/bash
# GPU check of a build: every GPU test, then the configs[1] bench without its child lines.
# Each step has its own time limit; the chain stops at the first failure.
cd /tmp && export TMPDIR=/tmp && cd "${REPO_ROOT:-$(dirname "$0")/..}" && mkdir -p bench_out
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > bench_out/pytest_gpu.log 2>&1
rc=$?; tail -3 bench_out/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --no-e2e --no-side-configs --no-cpu-baseline --no-pcie --no-fastq --steps 100 --warmup 10 > bench_out/bench_spec.json 2> bench_out/bench_spec.err
rc=$?; tail -c 400 bench_out/bench_spec.err; head -c 1500 bench_out/bench_spec.json; exit $rc
