# end-of-round verification: GPU test tier, smoke(), the bench line, the round's profiles.  usage: r6_final.sh TAG
TAG=${1:-round6_c}
export OUT=${OUT:-$PWD/profile_out}    # tools/profile_round.sh writes there too
mkdir -p $OUT
( time timeout 1500 python -m pytest tests -m gpu -x -q ) > $OUT/${TAG}_pytest_gpu.log 2>&1; tail -4 $OUT/${TAG}_pytest_gpu.log
timeout 600 python __graft_entry__.py smoke > $OUT/${TAG}_smoke.log 2>&1; tail -2 $OUT/${TAG}_smoke.log
timeout 900 python bench.py --full > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench.err; tail -c 600 $OUT/${TAG}_bench_line.json
bash tools/profile_round.sh $TAG stats_default stats sq traffic dominant > $OUT/${TAG}_profile.log 2>&1
timeout 600 python tools/low_occupancy.py $(find $OUT/profd_$TAG -name '*results.db' | head -1) > $OUT/${TAG}_low_occupancy.md 2>&1
ls -la $OUT/${TAG}_*
