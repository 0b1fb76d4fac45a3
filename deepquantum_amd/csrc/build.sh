#!/bin/bash
# Build libdqhip.so for gfx950 (cross-compiles without a GPU).  Output lands next to the package so it
# travels to the GPU box with the repo snapshot.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="${here}/../libdqhip.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
srcs=(dq_capi.hip dq_gate.hip dq_dense.hip dq_pass.hip dq_wave.hip dq_reduce.hip dq_dist.hip dq_plan.hip dq_entangle.hip dq_rdm.hip dq_sample.hip dq_diag.hip dq_pauli.hip dq_perm.hip dq_mux.hip dq_muxgrad.hip dq_excite.hip dq_psum.hip dq_select.hip dq_gram.hip dq_qft.hip dq_terms.hip dq_collapse.hip dq_hist.hip dq_jump.hip)
flags=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result -Wno-unused-value -mllvm -simplifycfg-sink-common=false -mllvm -structurizecfg-skip-uniform-regions)
# "object:what it holds" of the kernels that keep their working set in registers: nothing of it may land in scratch memory.
no_scratch=(
  "dq_select:a select_pauli_kernel"                    # a unit's entries and vectors
  "dq_gram:a gram_kernel / combine_kernel"             # the tiles' accumulators and a step's vectors
  "dq_qft:a qft_stage_kernel"                          # a window's 16 amplitudes and its twiddles
  "dq_terms:a terms_cross_kernel"                      # a unit's eight products through eleven butterfly stages
  "dq_collapse:a collapse_kernel / measure_draw_kernel"  # a unit's source vectors and the lane's part of the index map
)
# the objects compiled with resource-usage remarks, which go to build/<name>.usage: what a guard below reads
usage=(dq_wave "${no_scratch[@]%%:*}")
usage_files=("${usage[@]/#/${here}/build/}")
# compile $1 into $2 with the further flags $3..
compile() { "$HIPCC" "${flags[@]}" "${@:3}" ${DQ_HIPCC_EXTRA:-} -c "$1" -o "$2"; }
objs=()
mkdir -p "${here}/build"
# any header of this directory newer than object $1?
newer_hpp() { local h; for h in "${here}"/*.hpp; do [[ "$h" -nt "$1" ]] && return 0; done; return 1; }
pids=()
for s in "${srcs[@]}"; do
  name="${s%.hip}"
  o="${here}/build/${name}.o"
  objs+=("$o")
  if newer_hpp "$o" || [[ ! -f "$o" || "${here}/$s" -nt "$o" || "${here}/../../include/dq_hip.h" -nt "$o" || ( "$s" == dq_wave.hip && ( "${here}/dq_wave_asm.inc" -nt "$o" || "${here}/dq_wave_asm64.inc" -nt "$o" || "${here}/dq_wave_valu.inc" -nt "$o" || "${here}/dq_wave_valu64.inc" -nt "$o" ) ) ]]; then
    if [[ " ${usage[*]} " == *" ${name} "* ]]; then
      compile "${here}/$s" "$o" -Rpass-analysis=kernel-resource-usage 2> "${here}/build/${name}.usage" &
    else
      compile "${here}/$s" "$o" &
    fi
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do
  if [[ -n "$p" ]] && ! wait "$p"; then
    grep -h -B2 -A3 "error" "${usage_files[@]/%/.usage}" 2>/dev/null | head -40 >&2
    echo "build failed" >&2
    exit 1
  fi
done
# The wave-tile kernels are built for three waves per SIMD: 168 VGPRs, nothing spilled.  One SGPR too many held across
# the assembly spills into a 169th VGPR and silently costs a third of the occupancy (8 % of the headline, measured).
if [[ -f "${here}/build/dq_wave.usage" ]]; then
  if grep -A8 "wave_pass_kernel" "${here}/build/dq_wave.usage" | grep -E "VGPRs: (169|1[7-9][0-9]|[2-9][0-9][0-9])|Spill: [1-9]" > /dev/null; then
    echo "dq_wave.hip: a wave_pass_kernel instantiation exceeds 168 VGPRs or spills (see build/dq_wave.usage)" >&2
    grep -E "Function Name|VGPRs:|Spill" "${here}/build/dq_wave.usage" | sed 's/.*remark: //' >&2
    exit 1
  fi
fi
for g in "${no_scratch[@]}"; do
  name="${g%%:*}"
  if [[ -f "${here}/build/${name}.usage" ]]; then
    if grep -E "ScratchSize \[bytes/lane\]: [1-9]|Spill: [1-9]" "${here}/build/${name}.usage" > /dev/null; then
      echo "${name}.hip: ${g#*:} instantiation spills or uses scratch memory (see build/${name}.usage)" >&2
      exit 1
    fi
  fi
done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o "$out"
echo "built $out"
