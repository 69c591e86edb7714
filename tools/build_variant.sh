#!/bin/bash
# Dev box: build a named variant of libhfpf.so for same-box A/B runs (tools/ab_kernels.sh name=build/variants/name.so ...).
#   tools/build_variant.sh <name> [extra hipcc flags, e.g. -DHFPF_UPD2_CHUNK=12]      from the working tree
#   tools/build_variant.sh --rev <git rev> <name> [flags]                            from a committed revision
# build/ is git-ignored but travels to the GPU box with the snapshot.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
SRC=$R/high-fidelity-pointcloud-fusion_amd/csrc
if [ "$1" = "--rev" ]; then
  REV=$2; shift 2
  TMP=$(mktemp -d)
  # the revision's own csrc/ and include/, whole: whatever its hfpf.hip includes is there, and no list of files is kept here
  git -C $R archive $REV high-fidelity-pointcloud-fusion_amd/csrc include | tar -x -C $TMP
  SRC=$TMP/high-fidelity-pointcloud-fusion_amd/csrc
fi
NAME=$1; shift
mkdir -p $R/build/variants
# the engine's flag line lives in csrc/Makefile (the working tree's, also for --rev)
FLAGS=$(make -s --no-print-directory -C $R/high-fidelity-pointcloud-fusion_amd/csrc print-hipflags)
/opt/rocm/bin/hipcc $FLAGS "$@" -shared -o $R/build/variants/$NAME.so $SRC/hfpf.hip
echo "built build/variants/$NAME.so ($*)"
