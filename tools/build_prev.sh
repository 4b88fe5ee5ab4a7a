#!/bin/bash
# Build the library of a git revision (default HEAD), of the working tree (WORK)
# or of a directory holding csrc/ and include/ (DIR:path) into
# lightweight-snappy_amd/variants/libsnappy_amd_<name>.so (default name: prev)
# for A/B against the working tree with tools/variant_bench.py.  The recipe is
# the working tree's Makefile (`make lib`) over the revision's whole csrc/ and
# include/; the extra -D flags go to both kernel halves and the shim.
#   tools/build_prev.sh [REV|WORK|DIR:path] [NAME] [extra -D flags...]
# (env VARCH: the target; SCHED_C / SCHED_D: the halves' scheduler flags, A/B)
set -e
cd "$(dirname "$0")/.."
REV=${1:-HEAD}
NAME=${2:-prev}
shift 2 2>/dev/null || shift $#
P=lightweight-snappy_amd
B=$PWD/$P/build/var_$NAME
case $REV in WORK | DIR:*) ;; *)
    if ! git cat-file -e "$REV:$P/csrc/snappy_frame_host.cpp" 2>/dev/null; then
        echo "build_prev.sh: $REV is older than the framing format, whose objects the Makefile links: not built" >&2
        exit 1
    fi ;;
esac
rm -rf "$B" && mkdir -p "$B" $P/variants
case $REV in
WORK) SRCDIR=$PWD/$P/csrc INCDIR=$PWD/include ;;
DIR:*) D=$(cd "${REV#DIR:}" && pwd) SRCDIR=$D/csrc INCDIR=$D/include ;;
*)
    git archive "$REV" $P/csrc include | tar -x -C "$B"
    SRCDIR=$B/$P/csrc INCDIR=$B/include ;;
esac
make -s -j16 -C $P lib SRCDIR="$SRCDIR" INCDIR="$INCDIR" OBJDIR="$B" LIBOUT="$PWD/$P/variants/libsnappy_amd_$NAME.so" \
    DEFS_COMPRESS="$*" DEFS_DECODE="$*" DEFS_SHIM="$*" ${VARCH:+ARCH=$VARCH} \
    ${SCHED_C+SCHED_COMPRESS="$SCHED_C"} ${SCHED_D+SCHED_DECODE="$SCHED_D"}
rm -rf "$B"
echo "built $NAME ($REV $*)"
