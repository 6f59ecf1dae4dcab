#!/bin/bash
# GPU box: the default bench line and the 20-step line of the sources in the tree
out=${OUT:-bench_out}; mkdir -p $out                # results folder (OUT=<dir> to choose another)
python bench.py --full > $out/r06_bench_default.json 2> $out/r06_bench_default.err
python bench.py --full --steps 20 --warmup 5 > $out/r06_bench_head.json 2> $out/r06_bench_head.err
tail -c 600 $out/r06_bench_head.json
