#!/bin/bash
# experiment helper: build libmcorr with extra -D flags for ONE source into variants/<tag>/libmcorr.so
# usage: scripts/build_variant.sh <tag> <source.hip> <extra hipcc flags...>   (run on the CPU box, after a build)
# The objects are torch_motion_correction_amd/_build.py's SOURCES: every object compiled from <source.hip> is
# rebuilt with its own flags plus the extra ones, the others are linked from the package's build directory.
set -e
tag=$1; src=$(basename "$2"); shift 2
cd "$(dirname "$0")/.."
pkg=torch_motion_correction_amd
mkdir -p variants/$tag
objs=""; hit=0
while read -r s stem flags; do
  if [ "$s" = "$src" ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -Iinclude -I$pkg/csrc $flags "$@" \
      -c $pkg/csrc/$s -o variants/$tag/$stem.o
    objs="$objs variants/$tag/$stem.o"; hit=1
  else
    objs="$objs $pkg/build/$stem.o"
  fi
done < <(python3 -c "import sys; sys.path.insert(0, '$pkg'); from _build import SOURCES
for s, stem, flags in SOURCES: print(s, stem, *flags)")
[ $hit = 1 ] || { echo "$src is not a source of $pkg/_build.py" >&2; exit 1; }
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o variants/$tag/libmcorr.so
echo built variants/$tag/libmcorr.so
