#!/bin/bash
# A second build of this tree with extra compiler flags, next to the in-tree one:
#   bash tools/exp_build.sh NAME "FLAGS" -> exp/NAME/lib/{libr3dg_hip.so,_C.so}
# Its one standing use is the counting build, `bash tools/exp_build.sh COUNT -DR3DG_EXP_COUNT` (same
# results as the default build, plus the counters tools/exp_count.py prints). Run against a build with
# R3DG_LIB_DIR=exp/NAME/lib. The kernels have no other -D switches: a tuning A/B edits the constant.
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2
rm -rf "exp/$NAME"  # build.py rebuilds by source mtime only: a flag change needs a clean directory
R3DG_LIB_DIR=exp/$NAME/lib R3DG_OBJ_DIR=exp/$NAME/obj R3DG_EXTRA_HIPFLAGS="$FLAGS" python relightable3dgaussian_amd/build.py
