#!/usr/bin/env bash
# Compare the gfx950 device code of two source trees, file by file, without a GPU.
#
#   scripts/diff_device_isa.sh <tree-a> <tree-b> [jobs]
#
# For every deadtrees_amd/csrc/*.hip of either tree the device assembly is emitted with the Makefile's flags
# (hipcc --cuda-device-only -S) and compared after replacing the __hip_cuid_<hash> symbol — the one thing that moves when
# only host code or source text changes — with a fixed token.  Prints one line per file and exits 1 if any listing
# differs: a refactor of the host plumbing must leave all of them identical.  Compiler messages are shown only when a
# compile fails.
set -euo pipefail
[ $# -ge 2 ] || { echo "usage: $0 <tree-a> <tree-b> [jobs]" >&2; exit 2; }
A=$(cd "$1" && pwd); B=$(cd "$2" && pwd); JOBS=${3:-8}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CXXFLAGS=$(sed -n 's/^CXXFLAGS *= *//p' "$B/deadtrees_amd/csrc/Makefile" | sed 's/\$(ARCH)/'"${ARCH:-gfx950}"'/')
OUT=$(mktemp -d)
trap 'rm -rf "$OUT"' EXIT
mkdir -p "$OUT/a" "$OUT/b"
FILES=$( (cd "$A/deadtrees_amd/csrc" && ls *.hip; cd "$B/deadtrees_amd/csrc" && ls *.hip) | sort -u)
for f in $FILES; do
  for side in a b; do
    tree=$A; [ $side = b ] && tree=$B
    if [ -f "$tree/deadtrees_amd/csrc/$f" ]; then echo "$tree/deadtrees_amd/csrc $f $OUT/$side/${f%.hip}.s"; fi
  done
done | xargs -P "$JOBS" -L 1 sh -c 'cd "$0" && '"$HIPCC $CXXFLAGS"' --cuda-device-only -S "$1" -o "$2" 2>> "$2.log"' ||
  { echo "a compile failed:" >&2; cat "$OUT"/*/*.log >&2; exit 2; }
rc=0
for f in $FILES; do
  s=${f%.hip}.s
  if [ ! -f "$OUT/a/$s" ] || [ ! -f "$OUT/b/$s" ]; then echo "MISSING    $f"; rc=1; continue; fi
  sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$OUT/a/$s" > "$OUT/a/$s.n"
  sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$OUT/b/$s" > "$OUT/b/$s.n"
  if cmp -s "$OUT/a/$s.n" "$OUT/b/$s.n"; then
    echo "identical  $f ($(wc -l < "$OUT/a/$s.n") lines)"
  else
    echo "DIFFERENT  $f ($(diff "$OUT/a/$s.n" "$OUT/b/$s.n" | grep -c '^[<>]' || true) lines differ)"; rc=1
  fi
done
exit $rc
