#!/bin/bash
# profiling build of the engine with in-kernel phase stamps (scripts/timeline.py); never loaded by the product path
# (every unit of the library with -DFE_TIMELINE: SimP carries the stamp buffer, so the units have to agree on it)
cd "$(dirname "$0")/.." && python -c "
import sys
sys.path.insert(0, '.')
import __graft_entry__ as g
g._compile_engine('fluidlab_amd/csrc/libfluidengine_tl_hip.so', ['-DFE_TIMELINE'])"
