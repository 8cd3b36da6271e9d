#!/bin/bash
# Builds diagnostic variants of the stem kernel, four at a time: build_stem.sh <name>:<extra -D flags> ...
#   e.g. build_stem.sh 0:-DTT_STEM_SKIP=0 60:-DTT_STEM_SKIP=60 0ns:-DTT_STEM_SKIP=0,-DTT_STEM_REALTIME
# (stamps in shader cycles; with -DTT_STEM_REALTIME in ns: the two together give the clock the kernel held;
#  STAMP=0 build_stem.sh ... builds without the stamps: the launch time of such a build is the one to compare)
cd "$(dirname "$0")"
F="-O3 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -fno-slp-vectorize"
[ "${STAMP:-1}" = 1 ] && F="$F -DTT_STEM_STAMP"
n=0
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  ( hipcc $F ${flags//,/ } -o stem_parts_$name stem_parts.hip 2>&1 | grep -E "error" -A3 ) &
  n=$((n + 1)); if [ $((n % 4)) -eq 0 ]; then wait; fi
done
wait
