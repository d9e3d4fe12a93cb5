#!/bin/bash
# Proves that a change of host code left the device code alone, without a GPU.
#
#   tools/device_code_diff.sh build <tree> <outdir>     compile the device side of every HIP unit and part of <tree>'s library
#   tools/device_code_diff.sh compare <dirA> <dirB>     compare two such directories, unit by unit
#
# `build` takes the compile lines from a dry run of <tree>'s own csrc/Makefile (so every unit gets exactly the flags its build rule
# gives it, -D part selectors included) and reruns each with --cuda-device-only (unbundled, and with a fixed compilation-unit id: the
# default one is a hash of the source path, which would make two checkouts differ), writing <outdir>/<object name>.co.
# `compare` expects byte-identical code objects; for a unit that differs it prints the kernel symbols only one side has and the
# kernels whose disassembly differs.  Two checkouts (e.g. `git worktree add ../parent HEAD~1`) give the before / after pair.
# JOBS: parallel compiles (default 8).
set -euo pipefail
ROCM=${ROCM_PATH:-/opt/rocm}
READELF=$ROCM/llvm/bin/llvm-readelf
OBJDUMP=$ROCM/llvm/bin/llvm-objdump

case "${1:-}" in
build)
    tree=$(cd "$2" && pwd); out=$3
    mkdir -p "$out"; out=$(cd "$out" && pwd)
    make -n -B -C "$tree/area_average_interpolation_amd/csrc" OBJ=/nonexistent/obj OUT=/nonexistent/lib.so |
        grep -E -- ' -c -o /nonexistent/obj/[^ ]+\.o [^ ]+\.hip$' |
        sed -E "s# -c -o /nonexistent/obj/([^ ]+)\.o # --cuda-device-only --no-gpu-bundle-output -cuid=aai -c -o $out/\1.co #" > "$out/commands.txt"
    echo "$(wc -l < "$out/commands.txt") HIP units and parts in $tree"
    xargs -P "${JOBS:-8}" -d '\n' -n 1 sh -c < "$out/commands.txt"
    ;;
compare)
    a=$2; b=$3; differ=0
    for f in "$a"/*.co; do
        n=$(basename "$f")
        if [ ! -f "$b/$n" ]; then echo "MISSING    $n"; differ=1; continue; fi
        if cmp -s "$f" "$b/$n"; then echo "identical  $n  $(stat -c %s "$f") bytes"; continue; fi
        differ=1
        echo "DIFFERENT  $n  $(stat -c %s "$f") / $(stat -c %s "$b/$n") bytes"
        diff <("$READELF" -sW "$f" | awk '$4 == "FUNC" {print $8}' | sort) <("$READELF" -sW "$b/$n" | awk '$4 == "FUNC" {print $8}' | sort) | sed 's/^/    symbols: /' || true
        diff <("$OBJDUMP" -d --no-show-raw-insn "$f" | sed -E 's/^ +[0-9a-f]+://; s#^/.*:##') \
             <("$OBJDUMP" -d --no-show-raw-insn "$b/$n" | sed -E 's/^ +[0-9a-f]+://; s#^/.*:##') | grep -c '^[<>]' | sed 's/^/    disassembly lines that differ: /' || true
    done
    for f in "$b"/*.co; do [ -f "$a/$(basename "$f")" ] || { echo "EXTRA      $(basename "$f")"; differ=1; }; done
    exit $differ
    ;;
*)
    sed -n '2,12p' "$0"; exit 2
    ;;
esac
