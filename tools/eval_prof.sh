set -e
# rocprofv3 kernel trace of the eval loop (300 images). Usage, from the repo root: tools/eval_prof.sh <outdir>
R=$(pwd)
OUT=$R/${1:?output directory}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/evprof -o p -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-prof --eval-images 300 > $OUT/evprof.log 2>&1
