"""fe_smoke_index.h as the GPU compiles it: the device entry of tests/csrc/smoke_index_test.hip on the cases of tests/test_smoke_index.py, equal
to the host entry int for int and bit for bit.  The kernel only computes: it indexes no memory with what it computed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import smoke_index_cases as SI

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', SI.GRIDS)
def test_device_entry_equals_the_host_entry(n):
    p = SI.inputs(n)
    lib = SI.device_lib()
    rc_h, *host = SI.host_lib().axis(p, n)
    rc_d, *dev = lib.axis(p, n, entry='sit_axis')
    assert rc_h == 0 and rc_d == 0, (rc_h, rc_d)
    for name, h, d in zip(('base', 'f', 'c0', 'c1'), host, dev):
        bad = np.flatnonzero(h.view(np.uint32) != d.view(np.uint32))
        assert bad.size == 0, (name, p[bad[:5]], h[bad[:5]], d[bad[:5]])
    base, f, c0, c1 = dev
    assert (0 <= c0).all() and (c0 <= c1).all() and (c1 <= n - 1).all()
