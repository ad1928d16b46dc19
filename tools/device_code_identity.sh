#!/usr/bin/env bash
# Same device code in two checkouts: for every translation unit of csrc/build.sh's SRCS, compile the gfx950 code object alone
# (the library's flags plus --cuda-device-only --no-gpu-bundle-output) in checkout A and in checkout B and compare
#   * the symbols and their sizes (llvm-readelf -sW; the __hip_cuid_* object hashes the source text and is left out),
#   * the hash of the disassembly (llvm-objdump -d, without the line that names the file).
# Prints one line per unit: unit, kernels (kernel descriptors), symbols, disassembly hash of B, same | DIFFERENT.  Exit status 1 when
# a unit differs.  A host-side refactor of the launchers must leave every unit "same": a difference is an instantiation added or lost.
# usage: tools/device_code_identity.sh CHECKOUT_A CHECKOUT_B [WORKDIR]      (HDB_BUILD_JOBS: parallel compiles, default 8)
set -euo pipefail
A="$(cd "$1" && pwd)"; B="$(cd "$2" && pwd)"; WORK="${3:-$(mktemp -d)}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
LLVM="${LLVM_BIN:-/opt/rocm/llvm/bin}"
JOBS="${HDB_BUILD_JOBS:-8}"
FLAGS="$(sed -n 's/^FLAGS="\(.*\)"$/\1/p' "${B}/local-hyperdb_amd/csrc/build.sh")"
SRCS="$(sed -n 's/^SRCS="\(.*\)"$/\1/p' "${B}/local-hyperdb_amd/csrc/build.sh")"
mkdir -p "${WORK}/a" "${WORK}/b"
for side in a b; do
  root="${A}"; [ "${side}" = b ] && root="${B}"
  for u in ${SRCS}; do echo "${root}/local-hyperdb_amd/csrc/${u}.hip ${WORK}/${side}/${u}.co"; done
done | xargs -P "${JOBS}" -n 2 sh -c "exec ${HIPCC} ${FLAGS} --cuda-device-only --no-gpu-bundle-output -c \"\$0\" -o \"\$1\""
symbols() { "${LLVM}/llvm-readelf" -sW "$1" | awk '$1 ~ /^[0-9]+:$/ && $8 != "" && $8 !~ /^__hip_cuid_/ { print $8, $3, $4 }' | sort; }
disasm_hash() { "${LLVM}/llvm-objdump" -d "$1" | grep -v 'file format' | sha256sum | cut -c1-16; }
bad=0
printf '%-24s %8s %8s  %-16s  %s\n' unit kernels symbols disasm_sha256 verdict
for u in ${SRCS}; do
  sa="$(symbols "${WORK}/a/${u}.co")"; sb="$(symbols "${WORK}/b/${u}.co")"
  ha="$(disasm_hash "${WORK}/a/${u}.co")"; hb="$(disasm_hash "${WORK}/b/${u}.co")"
  v=same; { [ "${sa}" = "${sb}" ] && [ "${ha}" = "${hb}" ]; } || { v=DIFFERENT; bad=1; }
  printf '%-24s %8d %8d  %-16s  %s\n' "${u}" "$(printf '%s\n' "${sb}" | grep -c '\.kd ' || true)" "$(printf '%s\n' "${sb}" | grep -c . || true)" "${hb}" "${v}"
done
exit "${bad}"
