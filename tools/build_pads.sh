#!/bin/bash
# Placement-sweep builds of the working tree: one library per variant
# (NAME:-D flags of the compress half ...) into
# lightweight-snappy_amd/variants/libsnappy_amd_<NAME>.so for tools/variant_bench.py,
# each by the Makefile's own recipe (`make lib`) in an object directory of its own.
#   tools/build_pads.sh 'a2:-DSNAPPY_K1R_PAD32=2' 'e2:-DSNAPPY_K1R_RMIN=3 -DSNAPPY_K1R_PAD32=2' ...
# (env BASE: -D flags every variant gets, in both halves and the shim)
set -e
cd "$(dirname "$0")/.."
P=lightweight-snappy_amd; mkdir -p $P/variants
build_one() {
    local name=${1%%:*} defs=${1#*:}
    make -s -j4 -C $P lib OBJDIR="$PWD/$P/build/pad_$name" LIBOUT="$PWD/$P/variants/libsnappy_amd_$name.so" \
        DEFS_COMPRESS="$BASE $defs" DEFS_DECODE="$BASE" DEFS_SHIM="$BASE"
    echo "built $name ($defs)"
}
# four variants at a time (16 jobs)
n=0
for spec in "$@"; do
    build_one "$spec" &
    n=$((n + 1))
    if [ $((n % 4)) -eq 0 ]; then wait; fi
done
wait
