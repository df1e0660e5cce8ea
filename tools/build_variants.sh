#!/bin/bash
# Dev tool: build libgemini_hip.so with the flags of $EXTRA into tools/_build/var<name>/ for A/B runs through
# GM_LIB_PATH (tools/ab_variants.sh).  Usage: EXTRA=... tools/build_variants.sh <name>...
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
for k in "$@"; do
  d=$ROOT/tools/_build/var$k
  rm -rf "$d" && mkdir -p "$d/gemini_amd" "$d/include"
  cp -r "$ROOT/gemini_amd/csrc" "$d/gemini_amd/" && cp "$ROOT"/include/* "$d/include/"
  rm -f "$d"/gemini_amd/csrc/*.o
  make -s -C "$d/gemini_amd/csrc" -j4 EXTRA="$EXTRA" >/dev/null
  echo "built $d/gemini_amd/libgemini_hip.so (EXTRA=$EXTRA)"
done
