set -e
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
out=${OUT_DIR:-build/out}
mkdir -p "$out"
export MILA_CDNA4_TUNING=1
rm -rf $out/prof_2k_mfma
rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof_2k_mfma -- python3 bench.py --full --steps 16 --warmup 4 --policies bf16 --no-cpu --no-gpt2 --no-prefill --attn-split -7 > $out/prof_2k_mfma.log 2>&1
python3 tools/summarize_rocprof.py $out/prof_2k_mfma $out/ctx2k_mfma_kernels.md "experiment: MFMA decode from a band of 1024 keys on"
