set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-build/out}
mkdir -p "$out"
python3 bench.py --full --steps 20 --warmup 5 > $out/r04_bench_default.json 2> $out/r04_bench_default.err
echo "bench done"
for pol in bf16 fp8 fp4; do
  rm -rf $out/prof_r04f_$pol
  rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_r04f_$pol -- python3 bench.py --full --steps 16 --warmup 4 --policies $pol --no-cpu --no-gpt2 > $out/r04_bench_${pol}_under_rocprof.json 2> $out/prof_r04f_$pol.err
  python3 tools/summarize_rocprof.py $out/prof_r04f_$pol $out/r04_bench_${pol}_kernels.md "round 4: python bench.py --full --steps 16 --warmup 4 --policies $pol --no-cpu --no-gpt2 under rocprofv3 --kernel-trace --stats"
  rm -rf $out/prof_r04f_$pol
  echo "trace $pol done"
done
