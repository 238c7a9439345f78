#!/bin/bash
# Builds the UNPATCHED reference (GATB-Core, /root/reference/gatb-core) with ITS OWN cmake into a scratch directory — nothing is written to the reference
# tree, no reference source enters this repository — and copies the tools the measurement and integration legs use into oracle/_ref/ref/
# (git-ignored; oracle/build_ref.sh, run by __graft_entry__.build(), drives this script):
#   dbgh5, dbginfo      bench.py --full's cpu_baseline leg, kind "reference": the reference's own multithreaded SortingCountAlgorithm timed on the GPU box's host cores
#   gatb-h5dump         tools/make_reference_run_vectors.py, integration/check_graphunitigs.sh
# and leaves lib/Release/libgatbcore.a + libhdf5.a in the build directory for integration/check_integration.sh --link.
#   integration/build_reference.sh [build dir, default /tmp/gatb_build]
# A build directory that already holds the artefacts is reused (the cmake build takes ~10 minutes on 8 cores).
set -e
HERE=$(cd "$(dirname "$0")" && pwd); REPO=$(dirname "$HERE")
REF=${GATB_REFERENCE:-/root/reference/gatb-core}
BUILD=${1:-/tmp/gatb_build}
test -d "$REF/src/gatb" || { echo "reference not found at $REF"; exit 3; }
if [ ! -f "$BUILD/lib/Release/libgatbcore.a" ] || [ ! -x "$BUILD/bin/Release/dbgh5" ] || [ ! -x "$BUILD/bin/Release/dbginfo" ] || [ ! -x "$BUILD/bin/Release/gatb-h5dump" ]; then
  # the configure step writes generated HDF5 headers into the source tree: it runs on a writable copy (integration/reference_copy.sh), never on the reference
  SRC=$(bash "$HERE/reference_copy.sh" "$REF") || { echo "no writable copy of $REF"; exit 4; }
  if [ -f "$BUILD/CMakeCache.txt" ] && ! grep -qsx "CMAKE_HOME_DIRECTORY:INTERNAL=$SRC" "$BUILD/CMakeCache.txt"; then rm -rf "$BUILD"; fi    # configured from another tree
  mkdir -p "$BUILD"
  echo "[build_reference] configuring the reference (copy: $SRC) in $BUILD"
  (cd "$BUILD" && cmake -DCMAKE_BUILD_TYPE=Release -DGATB_CORE_EXCLUDE_EXAMPLES=1 -DGATB_CORE_EXCLUDE_TESTS=1 "$SRC" > cmake.log 2>&1) || { tail -20 "$BUILD/cmake.log"; exit 4; }
  echo "[build_reference] building (make -j${GKC_INTEGRATION_JOBS:-$(nproc)} dbgh5 dbginfo gatb-h5dump)"
  (cd "$BUILD" && make -j"${GKC_INTEGRATION_JOBS:-$(nproc)}" dbgh5 dbginfo gatb-h5dump > make.log 2>&1) || { tail -30 "$BUILD/make.log"; exit 5; }
fi
mkdir -p "$REPO/oracle/_ref/ref"
for t in dbgh5 dbginfo gatb-h5dump; do cp -f "$BUILD/bin/Release/$t" "$REPO/oracle/_ref/ref/$t" && strip -s "$REPO/oracle/_ref/ref/$t"; done     # (stripped: oracle/_ref/ travels)
echo "[build_reference] ok: $REPO/oracle/_ref/ref/{dbgh5,dbginfo,gatb-h5dump} (from $BUILD)"
