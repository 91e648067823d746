#!/bin/sh
# refresh_direct_asan.sh -- builds scripts/refresh_direct_asan.cpp with the host side of libmort_hip.so and the C scene layer under
# AddressSanitizer and UndefinedBehaviorSanitizer as ONE stand-alone executable, and runs it.  CPU only: the
# sanitizers instrument the host code alone (-Xarch_host; the kernels are compiled as they always are and never launched), and the
# program makes no HIP call.  Run from the repository root; build products go to build/asan.
set -e
ROCM=${ROCM:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
ARCH=${ARCH:-gfx950}
OUT=build/asan
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g"
CSAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g"
mkdir -p $OUT
objs=""
for f in mort_amd/csrc/hip/*.hip; do
    o=$OUT/$(basename $f .hip).o
    $HIPCC -O1 -std=c++17 -fPIC --offload-arch=$ARCH -ffp-contract=off -fno-fast-math -fno-slp-vectorize -fno-gpu-rdc $SAN -Wno-unused-value \
        -Wno-unused-result -Iinclude -c -o $o $f &
    objs="$objs $o"
done
for f in mort_amd/csrc/host/*.c; do
    o=$OUT/$(basename $f .c).o
    $HIPCC -O1 -x c -std=gnu11 -fPIC -ffp-contract=off -fno-fast-math $CSAN -Iinclude -c -o $o $f &
    objs="$objs $o"
done
$HIPCC -O1 -std=c++17 --offload-arch=$ARCH -fno-gpu-rdc -ffp-contract=off $SAN -Iinclude -c -o $OUT/refresh_direct_asan.o scripts/refresh_direct_asan.cpp &
wait
$HIPCC --offload-arch=$ARCH -fno-gpu-rdc $CSAN -o $OUT/refresh_direct_asan $OUT/refresh_direct_asan.o $objs -lpthread -ldl -lm
ASAN_OPTIONS=detect_leaks=1 $OUT/refresh_direct_asan
