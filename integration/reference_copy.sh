#!/bin/bash
# Prints the path of a writable copy of the reference sources, made on first use outside the repository.
# The reference's cmake configure step writes generated HDF5 headers (H5Epubgen.h, H5Einit.h, ...) into its own source tree, so it cannot run on
# a read-only reference; build_reference.sh and check_integration.sh configure and compile against this copy instead. The reference itself is only read.
#   integration/reference_copy.sh <reference dir>      (the copy goes to GKC_REFERENCE_COPY, else GKC_REFERENCE_WORK/gatb-core)
set -e
REF=$(cd "$1" && pwd)
DST=${GKC_REFERENCE_COPY:-${GKC_REFERENCE_WORK:-${TMPDIR:-/tmp}/gkc-reference-$(id -u)}/gatb-core}
if [ ! -f "$DST/.copied_from" ] || [ "$(cat "$DST/.copied_from")" != "$REF" ]; then
  rm -rf "$DST" "$DST.part"
  mkdir -p "$(dirname "$DST")"
  cp -R "$REF" "$DST.part"
  chmod -R u+w "$DST.part"
  echo "$REF" > "$DST.part/.copied_from"
  mv "$DST.part" "$DST"
fi
echo "$DST"
