"""fe_smoke_cells_add_grad and its _dev form are HIP-engine extensions (include/fluidengine_ext.h, fluidlab_amd/csrc/fe_smoke_reads.h): the
header declares them, they are extension symbols and not part of the oracle ABI, the HIP library exports them, and an oracle engine refuses
the Engine method.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

from fluidlab_amd import _capi

sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_smoke_cells_add_grad', 'fe_smoke_cells_add_grad_dev']


def test_hip_library_exports_both_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []


def test_header_declares_both_names():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'fluidengine_ext.h')).read()
    assert [s for s in NAMES if f'int {s}(FeEngine* h, int list, int s, const fe_real* gv, const fe_real* gq);' not in text] == []


def test_engine_method_raises_on_an_oracle_engine(oracle64):
    import scenarios as S
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    for call in (lambda: eng.smoke_cells_add_grad(0, 0, np.zeros((0, 3)), None), lambda: eng.smoke_cells_add_grad(0, 0, None, None)):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()
