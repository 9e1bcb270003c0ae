#!/bin/bash
# development helper: build tuning variants of librfx_hip.so into realism-effects_amd/csrc/variants/ (git-ignored).
#   tools/build_variants.sh <kernel-file-stem> <name>:"<defines>" ...     e.g.  tools/build_variants.sh k3_denoise a:"-DKNOB=4" b:"-DKNOB=8"
# time them on the GPU box with tools/time_variants.sh
# the object list and the contraction setting are csrc/Makefile's (sources.mk)
set -e
cd "$(dirname "$0")/../realism-effects_amd/csrc"
make -s
mkdir -p variants
stem=$1; shift
stems=$(make -s print-stems)
F="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -Wno-unused-function -Wno-unused-value -Wno-unused-result"
if make -s print-contracted | grep -qx "$stem"; then F="$F -ffp-contract=fast-honor-pragmas"; else F="$F -ffp-contract=off"; fi
for spec in "$@"; do
  name=${spec%%:*}; defs=${spec#*:}
  (
    /opt/rocm/bin/hipcc $F $defs -c $stem.hip -o variants/${stem}_$name.o 2>/dev/null
    objs=""
    for o in $stems; do
      if [ $o = $stem ]; then objs="$objs variants/${stem}_$name.o"; else objs="$objs $o.o"; fi
    done
    /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o variants/librfx_${stem}_$name.so $objs 2>/dev/null
  ) &
done
wait
ls variants/*.so
