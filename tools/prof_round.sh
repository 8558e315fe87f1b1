# Profile evidence of one round: whole SC and SCL bench lines (--full), rocprofv3 kernel statistics and the
# FETCH_SIZE / WRITE_SIZE passes.  usage: bash tools/prof_round.sh TAG   (e.g. r01i)
# Traces go to /tmp on the box; only the *_stats.csv summaries are copied to $O (default prof_out/).
set -e
TAG=${1:?usage: prof_round.sh TAG}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
T=/tmp/${TAG}_prof
O=${O:-prof_out}
mkdir -p $O
timeout -k 10 300 python bench.py --full > $O/${TAG}_bench_sc.json 2> $O/${TAG}_bench_sc.err
timeout -k 10 300 python bench.py --full --decoder scl > $O/${TAG}_bench_scl.json 2> $O/${TAG}_bench_scl.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/sc -o sc -- python3 bench.py --full --steps 300 --no-cpu-baseline > $O/${TAG}_prof_sc.json 2> $O/${TAG}_prof_sc.err
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $T/scl -o scl -- python3 bench.py --full --decoder scl --steps 10 --no-cpu-baseline > $O/${TAG}_prof_scl.json 2> $O/${TAG}_prof_scl.err
for f in $(find $T -name "*_stats.csv"); do cp "$f" $O/${TAG}_$(basename $(dirname $f))_$(basename $f); done
ls -la $O
# HBM traffic: FETCH_SIZE and WRITE_SIZE in separate passes (MI355X_MICROARCH HBM section)
for dec in sc scl; do
  for c in FETCH_SIZE WRITE_SIZE; do
    timeout -s KILL 120 rocprofv3 --pmc $c --output-format csv -d $T/pmc_${dec}_$c -o run -- python3 bench.py --decoder $dec --steps 3 --warmup 1 > /dev/null 2> $O/${TAG}_pmc_${dec}_$c.err
    cp $(find $T/pmc_${dec}_$c -name "*counter_collection.csv") $O/${TAG}_pmc_${dec}_$c.csv
  done
done
ls -la $O
