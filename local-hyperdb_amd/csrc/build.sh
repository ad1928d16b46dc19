#!/usr/bin/env bash
# Build libhyperdb_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${HERE}/../lib"
mkdir -p "${OUT}" "${HERE}/obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-pass-failed"
# parallel compiles: every core up to 16 unless HDB_BUILD_JOBS says otherwise
CORES="$(nproc)"
JOBS="${HDB_BUILD_JOBS:-$(( CORES < 16 ? CORES : 16 ))}"
# the translation units: compiled in this order, linked in this order
SRCS="hdb_mfma_anyd_a hdb_mfma_anyd_b hdb_mfma_anyd_c hdb_mfma_anyd_d hdb_mfma_anyd_e hdb_mfma_anyd_f hdb_mfma_ksplit hdb_mfma_ksplit_s hdb_mfma_d384 hdb_mfma_f32 hdb_mfma_f32b hdb_mfma_f32s hdb_mfma_f32s_b hdb_mfma_bf16 hdb_mfma_bf16_b hdb_mfma_bf16_ks hdb_mfma_bf16_ks_b hdb_mfma_f8 hdb_mfma_f8_b hdb_mfma_f8_ks hdb_mfma_f8_ks_b hdb_mfma_f8_lds hdb_mfma_f8_lds_b hdb_mfma_f8_lds_ks hdb_mfma_f8_lds_ks_b hdb_mfma_i8 hdb_mfma_i8_b hdb_mfma_b1 hdb_mfma_b1_b hdb_mfma_b1_ks hdb_mfma_b1_ks_b hdb_mfma_qt2 hdb_mfma_wide hdb_mfma_mid hdb_mfma_narrow hdb_mfma_1k hdb_mfma_fused hdb_mfma_fused_wide hdb_bits_fused hdb_l1_tile hdb_scan hdb_bscan hdb_rerank hdb_group hdb_maxsim hdb_mmr hdb_select hdb_mfma hdb_sort hdb_rows hdb_quant hdb_quant_mfma hdb_api"
# an object is stale when its source, any header beside it or the public header is newer
stale() {
  local obj="${HERE}/obj/$1.o" dep
  [ -f "${obj}" ] || return 0
  for dep in "${HERE}/$1.hip" "${HERE}"/*.h "${HERE}/../../include/hyperdb_hip.h"; do
    [ "${dep}" -nt "${obj}" ] && return 0
  done
  return 1
}
pids=()
objs=()
for src in ${SRCS}; do
  objs+=("${HERE}/obj/${src}.o")
  if stale "${src}"; then
    while [ "$(jobs -rp | wc -l)" -ge "${JOBS}" ]; do sleep 0.2; done
    ${HIPCC} ${FLAGS} -c "${HERE}/${src}.hip" -o "${HERE}/obj/${src}.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
${HIPCC} --offload-arch=gfx950 -shared -fPIC -o "${OUT}/libhyperdb_hip.so" "${objs[@]}"
echo "built ${OUT}/libhyperdb_hip.so"
