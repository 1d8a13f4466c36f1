#!/bin/bash
# Builds libdss2_hip.so for gfx950 in-tree (next to the package's Python files).
# hipcc cross-compiles without a GPU.  Usage: build.sh [extra hipcc flags]
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="${DSS2_OUT:-$HERE/../libdss2_hip.so}"
OBJ="${DSS2_OBJ:-$HERE/obj}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
# NOPK (dss2_gemm_chain16.hip only): no v_pk_{fma,mul,add}_f32 -- see that file's header.  The host pass does not know
# the feature and says so; that line is filtered.
FLAGS="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -I$ROOT/include -I$HERE -Wall -Wno-unused-function"
NOPK="-Xclang -target-feature -Xclang -packed-fp32-ops"
NOPK_SRCS="${DSS2_NOPK_SRCS-dss2_gemm_chain16 dss2_gemm_chain_sp dss2_gemm_chain_sp6 dss2_wgrad16 dss2_wgrad16h dss2_wgrad16th dss2_stack dss2_edge16}"      # (DSS2_NOPK_SRCS="" builds the diagnostic library WITH packed ops everywhere)
mkdir -p "$OBJ"
SRCS="dss2_api dss2_lanegroup dss2_gat dss2_gine dss2_gnn dss2_cheb dss2_stack dss2_gemm_prop dss2_gemm_chain dss2_gemm_chain16 dss2_gemm_chain_sp dss2_gemm_chain_sp6 dss2_edge dss2_edge16 dss2_wgrad dss2_wgrad16 dss2_wgrad16h dss2_wgrad16th dss2_loss dss2_wls_solve dss2_wls_bad_data dss2_wls_large dss2_wls_robust dss2_optim dss2_dataset dss2_topology"
# An object is rebuilt when it or its depfile is missing, or when the depfile -- written by the compiler (-MMD): the source and every
# header it includes -- names a file that is newer than the object or no longer exists.
stale() {
  local o="$OBJ/$1.o" d="$OBJ/$1.d" f
  [ -f "$o" ] && [ -f "$d" ] || return 0
  for f in $(sed -e 's/^[^:]*: *//' -e 's/ *\\$//' "$d"); do
    [ -e "$f" ] && ! [ "$f" -nt "$o" ] || return 0
  done
  return 1
}
pids=()
for src in $SRCS; do
  if stale "$src"; then
    extra=""; case " $NOPK_SRCS " in *" $src "*) extra="$NOPK";; esac
    $HIPCC $FLAGS $extra "$@" -MMD -MF "$OBJ/$src.d" -c "$HERE/$src.hip" -o "$OBJ/$src.o" 2> >(grep -v "is not a recognized feature for this target" >&2) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
echo "compiled ${#pids[@]} of $(echo $SRCS | wc -w) translation units"
# The NOPK translation units must really be free of packed fp32 VALU ops: the flag is passed with -Xclang and the host
# pass's "not a recognized feature" line is filtered above, so a toolchain that silently ignored it on the DEVICE pass
# would give no other signal.  Disassemble the gfx950 code objects and fail the build if one v_pk_*_f32 is left.
OBJDUMP="${OBJDUMP:-/opt/rocm/lib/llvm/bin/llvm-objdump}"
for src in $NOPK_SRCS; do
  tmp="$(mktemp -d)"
  cp "$OBJ/$src.o" "$tmp/x.o"
  (cd "$tmp" && "$OBJDUMP" --offloading x.o >/dev/null)
  co="$(ls "$tmp"/x.o.*gfx950* 2>/dev/null | head -1)"
  if [ -z "$co" ]; then echo "build.sh: no gfx950 code object found in $src.o" >&2; rm -rf "$tmp"; exit 1; fi
  npk="$("$OBJDUMP" -d "$co" | grep -c -E 'v_pk_(fma|mul|add)_f32' || true)"
  rm -rf "$tmp"
  if [ "$npk" != "0" ]; then
    echo "build.sh: $src.hip was compiled with $npk packed fp32 VALU instructions: '-target-feature -packed-fp32-ops' did not take effect" >&2
    exit 1
  fi
done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" "$OBJ"/*.o
echo "built $OUT"
