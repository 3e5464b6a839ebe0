#!/bin/bash
# Is the working tree's rucene_amd/csrc/rgpu_api.hip the same program as the one at <git-rev>? For changes that only move text between
# files (the parts under csrc/api/): nothing the compiler sees may differ. No GPU. Exits non-zero at the first difference.
#   scripts/same_translation_unit.sh <git-rev>
# (0) the expanded source text, comments included, which (a) cannot see: rgpu_api.hip in front of the banner of its tail, then each part
#     in include order without its head (everything through its "Not a stand-alone header" line and the blank line behind it), with
#     `#include "../host/` read as `#include "host/`. First, because it is instant: text moved verbatim and in order compares equal;
# (a) the preprocessed text (hipcc -E -P, blank lines deleted) of the host and of the device side, for the default build and for each
#     variant macro the file branches on;
# (b) the device-only object of the default build, under the build's own flags and one fixed compilation-unit id on both sides
#     (-cuid: by default a hash of the main file, which names some device symbols), byte for byte;
# (c) the host-only object of the default build, the same way.
# The old tree (rucene_amd/csrc and include) is exported from git into a temporary directory; at most two compiles run at a time.
# The whole .so is not comparable: two builds of one source already differ.
set -u
REV=${1:?usage: scripts/same_translation_unit.sh <git-rev>}
R=$(cd "$(dirname "$0")/.." && pwd)
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
mkdir -p "$T/old" "$T/out"
git -C "$R" archive "$REV" rucene_amd/csrc include | tar -x -C "$T/old" || { echo "cannot export $REV"; exit 2; }
OLD=$T/old/rucene_amd/csrc/rgpu_api.hip
NEW=$R/rucene_amd/csrc/rgpu_api.hip

# pair <name> <flags ...>: run hipcc with the flags on the old and on the new file at once, into $T/out/<name>.{old,new}
pair() {
  local name=$1; shift
  "$HIPCC" --offload-arch=gfx950 -std=c++17 "$@" -o "$T/out/$name.old" "$OLD" 2> "$T/out/$name.old.err" &
  local p_old=$!
  "$HIPCC" --offload-arch=gfx950 -std=c++17 "$@" -o "$T/out/$name.new" "$NEW" 2> "$T/out/$name.new.err"
  local rc_new=$?
  wait $p_old
  local rc_old=$?
  if [ $rc_old -ne 0 ] || [ $rc_new -ne 0 ]; then
    echo "FAILED TO COMPILE  $name (old: $rc_old, new: $rc_new)"; tail -n 20 "$T/out/$name.old.err" "$T/out/$name.new.err"; exit 2
  fi
}

echo "rgpu_api.hip: the working tree against $(git -C "$R" rev-parse --short "$REV")"
# (0) expanded <csrc dir>: rgpu_api.hip in front of the banner of its tail, then every part in include order, each from behind its head
expanded() {
  sed '/^\/\/ ---- the tail of this translation unit/,$d' "$1/rgpu_api.hip"
  sed -n 's|^#include "\(api/[a-z_]*\.hpp\)".*|\1|p' "$1/rgpu_api.hip" | while read -r part; do
    awk 'h == 2 { print } h == 1 { h = 2; if ($0 != "") print } h == 0 && /Not a stand-alone header/ { h = 1 }' "$1/$part"
  done
}
expanded "$T/old/rucene_amd/csrc" | sed 's|#include "\.\./host/|#include "host/|' > "$T/out/expanded.old"
expanded "$R/rucene_amd/csrc" | sed 's|#include "\.\./host/|#include "host/|' > "$T/out/expanded.new"
if ! cmp -s "$T/out/expanded.old" "$T/out/expanded.new"; then
  echo "DIFFERENT  expanded source text"
  diff "$T/out/expanded.old" "$T/out/expanded.new" | head -n 20
  exit 1
fi
printf 'same  expanded source text  %d lines\n' "$(wc -l < "$T/out/expanded.new")"
for variant in "" -DRGPU_LZ_TIME -DRGPU_ORX_TIME -DRGPU_AND_TIME -DRGPU_TERM_TRACE -DRGPU_AND_TRACE -DRGPU_EXP_COUNT -DRGPU_EXP_KEEP_TAU \
               -DRGPU_HOST_TIME -DRGPU_ORX_WAVES=16; do
  for side in host device; do
    name=pp_${side}_${variant:-default}
    pair "$name" -E -P --cuda-$side-only $variant
    sed -i '/^[[:space:]]*$/d' "$T/out/$name.old" "$T/out/$name.new"
    if ! cmp -s "$T/out/$name.old" "$T/out/$name.new"; then
      echo "DIFFERENT  preprocessed text, $side side, ${variant:-default build}"
      diff "$T/out/$name.old" "$T/out/$name.new" | head -n 20
      exit 1
    fi
    printf 'same  preprocessed text  %-6s  %-20s  %8d lines\n' $side "${variant:-default build}" "$(wc -l < "$T/out/$name.new")"
  done
done

pair device_object -O3 -ffp-contract=off -fPIC --cuda-device-only -c -cuid=rgpu_api
if ! cmp "$T/out/device_object.old" "$T/out/device_object.new"; then
  echo "DIFFERENT  device object of the default build"
  exit 1
fi
printf 'same  device object (default build, -cuid=rgpu_api)  %d bytes  sha256 %s\n' "$(stat -c %s "$T/out/device_object.new")" \
  "$(sha256sum "$T/out/device_object.new" | cut -c1-16)"

# (c) the host-only object likewise: the calling thread's code is what a step of the fused single-term call mostly costs
pair host_object -O3 -ffp-contract=off -fPIC --cuda-host-only -c -cuid=rgpu_api
if ! cmp "$T/out/host_object.old" "$T/out/host_object.new"; then
  echo "DIFFERENT  host object of the default build"
  exit 1
fi
printf 'same  host object   (default build, -cuid=rgpu_api)  %d bytes  sha256 %s\n' "$(stat -c %s "$T/out/host_object.new")" \
  "$(sha256sum "$T/out/host_object.new" | cut -c1-16)"
echo "the same program"
