# HBM traffic (FETCH_SIZE / WRITE_SIZE per kernel, tools/pmc_traffic.py) of library builds:
#   tools/traffic_ab.sh <lib|default> ...        (lib: the path of a libttup build, absolute or from the repository root)
# Output: tab_<tag>.json (per-kernel bytes read / written) per build, beside the profiles.
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT; cd $R
for spec in "$@"; do
  if [ "$spec" = default ]; then tag=default; unset TTUP_LIB
  else tag=$(basename "$spec" .so); tag=${tag#libttup_}; export TTUP_LIB=$(realpath "$spec"); fi
  rocprofv3 --output-format csv --kernel-trace --pmc FETCH_SIZE -d gpurun_out/tab_$tag/f -- python3 tools/prof_cnn.py > /dev/null 2>&1
  rocprofv3 --output-format csv --kernel-trace --pmc WRITE_SIZE -d gpurun_out/tab_$tag/w -- python3 tools/prof_cnn.py > /dev/null 2>&1
  python3 tools/pmc_traffic.py gpurun_out/tab_$tag/f gpurun_out/tab_$tag/w > gpurun_out/tab_$tag.json
done
