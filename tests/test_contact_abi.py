"""The contact wrench is a HIP-engine extension (include/fluidengine_ext.h): the HIP library exports its two names, the ctypes record and the
numpy dtype have the size and the offsets of the C record, and an oracle engine refuses the new Engine methods.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_contact_count', 'fe_contact_wrench']
FIELDS = ['impulse', 'ang_impulse', 'ref', 'n_particles', 'n_nodes', 'valid', 'kind']


def test_hip_library_exports_the_two_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_ctypes_record_has_the_size_and_offsets_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu", sizeof(FeContactRecord));\n'
                   + ''.join(f'  printf(" %zu", offsetof(FeContactRecord, {k}));\n' for k in FIELDS) + '  printf("\\n"); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    size, *offs = (int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(_capi.FeContactRecord) == size == _capi.CONTACT_DTYPE.itemsize == 8 * 12
    assert [k for k, _ in _capi.FeContactRecord._fields_] == FIELDS == list(_capi.CONTACT_DTYPE.names)
    assert [getattr(_capi.FeContactRecord, k).offset for k in FIELDS] == offs == [_capi.CONTACT_DTYPE.fields[k][1] for k in FIELDS]


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    for call in (lambda: eng.contact_count(), lambda: eng.contact_wrench(0), lambda: eng.contact_wrench(0, 2)):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()
