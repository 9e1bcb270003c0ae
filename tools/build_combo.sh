#!/bin/bash
# development helper: build tuning variants of librfx_hip.so that swap SEVERAL objects at once into realism-effects_amd/csrc/variants/
# (git-ignored).  Complements build_variants.sh (one file, several define sets).
#   tools/build_combo.sh obj  <objname> <source.hip> "<extra flags>"      compile one object into variants/<objname>.o
#   tools/build_combo.sh link <libname> <stem>=<objname> <stem>=<objname> ...   link variants/librfx_<libname>.so, the named objects swapped in
# contraction follows csrc/Makefile (sources.mk's contracted list; a source whose name starts with a contracted stem counts) unless the extra
# flags say otherwise; the object list is csrc/Makefile's too.
set -e
cd "$(dirname "$0")/../realism-effects_amd/csrc"
mkdir -p variants
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -I. -Wno-unused-function -Wno-unused-value -Wno-unused-result"
case $1 in
obj)
  name=$2; src=$3; extra=$4
  C="-ffp-contract=off"
  for s in $(make -s print-contracted); do case $(basename $src) in $s*) C="-ffp-contract=fast-honor-pragmas";; esac; done
  /opt/rocm/bin/hipcc $F $C $extra -c $src -o variants/$name.o 2>/dev/null
  ;;
link)
  lib=$2; shift 2
  objs=""
  for o in $(make -s print-stems); do
    r=$o.o
    for kv in "$@"; do [ "${kv%%=*}" = "$o" ] && r=variants/${kv#*=}.o; done
    objs="$objs $r"
  done
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o variants/librfx_$lib.so $objs 2>/dev/null
  ;;
*) echo "usage: see the header"; exit 2;;
esac
