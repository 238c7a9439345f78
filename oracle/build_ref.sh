#!/bin/bash
# Builds the reference-side binaries the drop-in tests, tools/make_reference_run_vectors.py and bench.py --full run, into oracle/_ref/ (git-ignored):
#   oracle/_ref/ref/{dbgh5,dbginfo,gatb-h5dump}   the UNPATCHED reference, built with its own cmake (integration/build_reference.sh)
#   oracle/_ref/ref/unitigs_check                 integration/unitigs_check.cpp against the unpatched library
#   oracle/_ref/{dbgh5_device,unitigs_check}      the reference's dbgh5 patched with integration/gatb-core.device.patch, linked against libgkc_hip.so
#                                                 (integration/check_integration.sh --link; found at run time through an rpath relative to oracle/_ref/)
# oracle/_ref/ holds these six (stripped) executables and nothing else, so it can travel to another machine as it is. The intermediate trees live outside the
# repository under GKC_REFERENCE_WORK (default $TMPDIR/gkc-reference-<uid>): gatb-core/ (a writable copy of the reference sources), gatb_build/ (the
# reference's cmake build), integration/ (the patched units' objects); a second run only relinks. Needs the reference sources (GATB_REFERENCE); without
# them it changes nothing and exits 3.
#   oracle/build_ref.sh            (libgkc_hip.so must be built first)
set -e
HERE=$(cd "$(dirname "$0")" && pwd); REPO=$(dirname "$HERE")
OUT="$HERE/_ref"
export GKC_REFERENCE_WORK=${GKC_REFERENCE_WORK:-${TMPDIR:-/tmp}/gkc-reference-$(id -u)}
J=$(nproc); [ "$J" -gt 16 ] && J=16
export GKC_INTEGRATION_JOBS=${GKC_INTEGRATION_JOBS:-$J}
rc=0; bash "$REPO/integration/build_reference.sh" "$GKC_REFERENCE_WORK/gatb_build" || rc=$?
[ $rc -eq 0 ] || exit $rc
bash "$REPO/integration/check_integration.sh" "$GKC_REFERENCE_WORK/integration" --link "$GKC_REFERENCE_WORK/gatb_build"
for art in dbgh5_device unitigs_check ref/dbgh5 ref/gatb-h5dump ref/dbginfo ref/unitigs_check; do
  test -x "$OUT/$art" || { echo "[build_ref] $OUT/$art was not produced"; exit 1; }
done
echo "[build_ref] ok: $OUT"
