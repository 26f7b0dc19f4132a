#!/bin/bash
# a second library with extra -D flags on EVERY device source (tools/build_variant.sh recompiles render.hip only): tools/build_variant_all.sh <name> <flags...>
# -> fredholm_amd/libfredholm_hip_<name>.so (git-ignored, travels to the GPU box; FH_LIB=... selects it)
set -e
name=$1; shift
cd "$(dirname "$0")/../fredholm_amd/csrc"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt -Wno-unused-function -Wno-unused-result"
mkdir -p /tmp/fhv_$name
[ -f gen/tables.inc ] || make gen/tables.inc
SRCS="capi scene render bvh_build kat post denoise motion group envmap"  # (fredholm_amd/csrc/Makefile: SRCS)
for f in $SRCS; do
  /opt/rocm/bin/hipcc $FLAGS "$@" -c $f.hip -o /tmp/fhv_$name/$f.o &
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o ../libfredholm_hip_$name.so $(for f in $SRCS; do echo /tmp/fhv_$name/$f.o; done)
ls -la ../libfredholm_hip_$name.so
