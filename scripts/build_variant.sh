#!/bin/bash
# An A/B build of the engine (same ABI) under scripts/_bin/ (git-ignored, travels to the GPU box): never loaded by the product path.
# usage: scripts/build_variant.sh <name> [-DMACRO=VALUE | -mllvm <flag> ...]      the extra flags go to every unit of the library
#        UNIT=fe_particles|fe_particles_gather|fe_engine scripts/build_variant.sh <name> <flags>      ... to that object only (per-unit A/B)
#        SRC=<dir> scripts/build_variant.sh <name>      builds another checkout's sources: a single-file checkout (before the engine was two units) the old way
NAME=$1; shift
cd "$(dirname "$0")/.." && mkdir -p scripts/_bin || exit 1
if [ -n "$SRC" ] && [ ! -f "$SRC/fluidlab_amd/csrc/fe_particles.hip" ]; then
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC -munsafe-fp-atomics -fno-slp-vectorize -mllvm -amdgpu-kernarg-preload-count=16 "$@" \
        -o scripts/_bin/libfe_$NAME.so $SRC/fluidlab_amd/csrc/fe_engine.hip && echo built scripts/_bin/libfe_$NAME.so
    exit $?
fi
OUT=$PWD/scripts/_bin/libfe_$NAME.so
cd "${SRC:-.}" && python - "$OUT" "${UNIT:-}" "$@" <<'EOF' && echo built scripts/_bin/libfe_$NAME.so
import sys
sys.path.insert(0, '.')
import __graft_entry__ as g
out, unit, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
if unit:
    assert unit in [obj for obj, _, _ in g.UNITS], unit
    g.UNITS = tuple((obj, src, list(flags) + (extra if obj == unit else [])) for obj, src, flags in g.UNITS)
    extra = []
g._compile_engine(out, extra)
EOF
