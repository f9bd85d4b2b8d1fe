"""fe_smoke_index.h on the host (no GPU): sm_tri_axis against its numpy restatement on every case class -- +-0, +-0.5, n +- 0.5, +-2^24,
+-(2^30 - 64), +-2^30, +-3e9, +-2^31, +-3e38, +-FLT_MAX, +-inf, quiet and signalling NaN, denormals -- 100,000 seeded values over
+-1.5 * 2^30 and 100,000 in [-2, n + 2], for n in {1, 2, 16, 128}.  base, c0, c1 are equal as ints and f as float bits; 0 <= c0 <= c1 <= n - 1;
and for every finite |p| <= 2^30 base and f are what the expression the helper replaced gives, evaluated in int64 / float32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import smoke_index_cases as SI


@pytest.mark.parametrize('n', SI.GRIDS)
def test_host_entry_equals_the_numpy_restatement(n):
    p = SI.inputs(n)
    rc, base, f, c0, c1 = SI.host_lib().axis(p, n)
    assert rc == 0
    rb, rf, r0, r1 = SI.restate(p, n)
    assert (base.astype(np.int64) == rb).all()
    assert (c0.astype(np.int64) == r0).all() and (c1.astype(np.int64) == r1).all()
    assert (f.view(np.uint32) == rf.view(np.uint32)).all()
    assert (0 <= c0).all() and (c0 <= c1).all() and (c1 <= n - 1).all()
    assert np.isfinite(f).all() and (np.abs(base.astype(np.int64)) <= 2 ** 30).all()      # base + 1 fits an int


@pytest.mark.parametrize('n', SI.GRIDS)
def test_identity_with_the_old_expression_inside_the_clamp(n):
    p = SI.inputs(n)
    with np.errstate(invalid='ignore'):
        inside = np.isfinite(p) & (np.abs(p) <= SI.P_MAX)
    assert inside.sum() > 100000 and (~inside).sum() > 10000                              # both sides of the clamp are exercised
    rc, base, f, c0, c1 = SI.host_lib().axis(p, n)
    ob, of = SI.old_expression(p[inside])
    assert (base[inside].astype(np.int64) == ob).all()
    assert (f[inside].view(np.uint32) == of.view(np.uint32)).all()


def test_device_library_cross_compiles_and_its_cpu_entry_agrees():
    """the gfx950 build of the same file (no GPU needed to compile it); its CPU entry, compiled with the engine's flags, gives the same bits"""
    lib = SI.device_lib()
    assert hasattr(lib.lib, 'sit_axis') and hasattr(lib.lib, 'sit_axis_host')
    p = SI.inputs(16)
    a, b = SI.host_lib().axis(p, 16), lib.axis(p, 16)
    for x, y in zip(a[1:], b[1:]):
        assert (x.view(np.uint32) == y.view(np.uint32)).all()


def test_outside_the_clamp_every_cell_is_the_edge_cell_and_f_is_zero():
    n = 16
    p = np.array([2.0 ** 30, 3e9, 2.0 ** 31, 3e38, np.inf, -2.0 ** 30, -3e9, -2.0 ** 31, -3e38, -np.inf, np.nan], np.float32)
    rc, base, f, c0, c1 = SI.host_lib().axis(p, n)
    assert (f == 0).all()
    assert (c0[:5] == n - 1).all() and (c1[:5] == n - 1).all()
    assert (c0[5:] == 0).all() and (c1[5:] == 0).all()                                    # (NaN goes to the lower bound)
    assert (base[:5] == 2 ** 30).all() and (base[5:] == -2 ** 30).all()
