"""The host restatement of the observation fields (fluidlab_amd/fluidengine/losses/term_program.py: field_obs_of_points,
field_obs_grad_of_points) on its own: partition of unity, the guards, the projected axis, the gradient against central differences in fp64
with the yardstick of tests/test_closed_loop_oracle.py, and the one-rounding middle weight against exact rational arithmetic.  No GPU, no
engine."""
from fractions import Fraction

import numpy as np
import pytest

from fluidlab_amd.fluidengine.losses.term_program import (DensityField, density_of_points, density_stencil, field_obs_grad_of_points,
                                                          field_obs_of_points, fused_middle_weight)

M = 500
SPECS = {'8x8x8': DensityField((0.2, 0.2, 0.2), (0.075, 0.075, 0.075), (8, 8, 8)),
         '8x1x8': DensityField((0.2, 0.0, 0.2), (0.075, 1.0, 0.075), (8, 1, 8))}
H = 2e-4                                                     # the larger step of the central differences (the field is piecewise quadratic: no truncation away from a stencil switch, rounding ~ eps |value| / h); the yardstick compares h and h / 2


def _points(seed=11):
    """500 seeded points around the box [0.2, 0.8]^3: most inside, some near its faces and some beyond; velocities of a few units"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(0.1, 0.9, (M, 3))
    x[:40] = rng.uniform(0.75, 0.85, (40, 3))                # near and beyond the upper faces
    x[40:60] = rng.uniform(-0.3, 0.15, (20, 3))              # well outside
    v = rng.uniform(-3.0, 3.0, (M, 3))
    return x, v


def _switch_distance(x, spec):
    """per point: the distance in x, over the unprojected axes, to the nearest stencil switch (u integer: t jumps from 1.5 to 0.5)"""
    d = np.full(len(x), np.inf)
    for a in range(3):
        if int(spec.n[a]) == 1:
            continue
        u = (x[:, a] - spec.origin[a]) / spec.cell[a]
        d = np.minimum(d, np.abs(u - np.rint(u)) * spec.cell[a])
    return d


@pytest.mark.parametrize('name', list(SPECS))
def test_partition_of_unity(name):
    spec = SPECS[name]
    x, v = _points()
    ok, base, _, _ = density_stencil(x, spec)
    n = np.array(spec.n)
    inside = ok & np.all((base >= 0) & ((base + 2 < n) | (n == 1)), axis=1)
    m = int(inside.sum())
    assert 50 < m < M                                        # some stencils reach outside, some points are beyond the box
    plain = field_obs_of_points(x[inside], v[inside], spec, 4, quantise=False)
    fixed = field_obs_of_points(x[inside], v[inside], spec, 4, quantise=True)
    vsum = v[inside].sum(axis=0)
    print(f'{name}: {m} points inside; sum D plain {plain[0].sum()!r} fixed {fixed[0].sum()!r}; sum P plain {plain[1:].sum(axis=(1, 2, 3))!r} want {vsum!r}')
    eps = np.finfo(np.float64).eps
    assert abs(plain[0].sum() - m) <= 64 * eps * m
    assert np.all(np.abs(plain[1:].sum(axis=(1, 2, 3)) - vsum) <= 64 * eps * np.abs(v[inside]).sum())
    tol = 27 * m * 2.0 ** -29
    assert abs(fixed[0].sum() - m) <= tol and np.all(np.abs(fixed[1:].sum(axis=(1, 2, 3)) - vsum) <= tol)
    # per cell the fixed-point field is within k_c 2^-29 of the plain one, and channel 0 is the density field
    _, K = density_of_points(x[inside], spec, counts=True)
    assert np.all(np.abs(fixed - plain) <= K[None] * 2.0 ** -29 + 1e-13)
    assert np.all(np.abs(plain[0] - density_of_points(x[inside], spec)) <= 8 * eps * K)
    assert np.array_equal(field_obs_of_points(x[inside], v[inside], spec, 1), fixed[:1])
    # the words are integers at their scales, and the field does not depend on the order of the points
    assert np.array_equal(fixed[0] * 2.0 ** 40, np.rint(fixed[0] * 2.0 ** 40)) and np.array_equal(fixed[1:] * 2.0 ** 28, np.rint(fixed[1:] * 2.0 ** 28))
    perm = np.random.RandomState(3).permutation(m)
    assert np.array_equal(field_obs_of_points(x[inside][perm], v[inside][perm], spec, 4), fixed)


@pytest.mark.parametrize('name', list(SPECS))
@pytest.mark.parametrize('channels', [1, 4])
def test_gradient_against_central_differences(name, channels):
    spec = SPECS[name]
    x, v = _points()
    keep = _switch_distance(x, spec) > 2 * H
    x, v = x[keep], v[keep]
    assert len(x) > 400 and np.all(_switch_distance(x, spec) > 2 * H)      # no point within 2h of a stencil switch
    G = np.random.RandomState(5).uniform(-1.0, 1.0, (channels,) + spec.shape)
    gx, gv = field_obs_grad_of_points(x, v, spec, G)

    def value(xx, vv):
        return float((G * field_obs_of_points(xx, vv, spec, channels, quantise=False)).sum())

    def fd(dx, dv, h):
        return (value(x + h * dx, v + h * dv) - value(x - h * dx, v - h * dv)) / (2 * h)

    # Seeded unit directions in the space of all coordinates (x alone, v alone, both), as tests/test_closed_loop_oracle.py takes them in
    # parameter space: the difference quotient of the whole sum carries rounding eps |value| / h ~ 1e-11, which the yardstick's relative
    # term covers for a directional derivative of order 0.1 .. 10 and does not for the single coordinates of order 1e-5 among them.  No
    # coordinate moves by more than h, and no point lies within 2 h of a switch.
    rng = np.random.RandomState(9)
    checked = 0
    for which in ('x', 'v', 'xv') * 4:
        dx = rng.normal(size=x.shape) if 'x' in which else np.zeros_like(x)
        dv = rng.normal(size=v.shape) if 'v' in which else np.zeros_like(v)
        nrm = np.sqrt((dx * dx).sum() + (dv * dv).sum())
        dx, dv = dx / nrm, dv / nrm
        adj = float((gx * dx).sum() + (gv * dv).sum())
        f1, f2 = fd(dx, dv, H), fd(dx, dv, H / 2)
        tol = 10 * abs(f1 - f2) + 1e-9 * abs(f2)
        print(f'{name} C={channels} direction {which}: adjoint {adj!r} FD_h/2 {f2!r} |adj - FD| {abs(adj - f2):.3e} tolerance {tol:.3e}')
        assert abs(adj - f2) <= tol, (which, adj, f1, f2)
        checked += adj != 0
    assert checked >= (12 if channels == 4 else 8)
    if channels == 1:
        assert np.all(gv == 0)
    if spec.shape[1] == 1:
        assert np.all(gx[:, 1] == 0)                         # the projected axis has zero derivative
    far = np.all(x < 0.0, axis=1) if spec.shape[1] > 1 else (x[:, 0] < 0.0) & (x[:, 2] < 0.0)
    assert np.all(gx[far] == 0) and np.all(gv[far] == 0)     # a stencil wholly outside the field


@pytest.mark.parametrize('name', list(SPECS))
def test_dropped_particles_have_zero_rows_and_deposit_nothing(name):
    spec = SPECS[name]
    x, v = _points()
    x, v = x[100:300].copy(), v[100:300].copy()
    bad = np.arange(0, 14)
    clean_x, clean_v = np.delete(x, bad, axis=0), np.delete(v, bad, axis=0)
    above = float(np.nextafter(np.float32(1024.0), np.float32(np.inf)))
    x[0, 0] = np.nan; x[1, 2] = np.inf; x[2, 0] = 1e12       # the density guard (|u| > 2^30 on an unprojected axis)
    v[3, 0] = np.inf; v[4, 1] = -np.inf; v[5, 2] = np.nan    # non-finite velocity words
    v[6, 0] = above; v[7, 1] = -above; v[8, 2] = 2049.0      # beyond 2^10
    v[9, 1] = 1e30; x[10, 2] = -np.inf; v[11, 0] = np.nan; x[12, 0] = np.nan; v[13, 2] = -2049.0
    edge = len(x) - 1
    v[edge] = [1024.0, -1024.0, 1024.0]                      # |v| = 2^10 is kept
    clean_v[-1] = v[edge]
    G = np.random.RandomState(6).uniform(-1.0, 1.0, (4,) + spec.shape)
    for quantise in (True, False):
        with np.errstate(invalid='ignore', over='ignore'):
            got = field_obs_of_points(x, v, spec, 4, quantise=quantise)
        want = field_obs_of_points(clean_x, clean_v, spec, 4, quantise=quantise)
        assert np.array_equal(got, want) if quantise else np.allclose(got, want, rtol=0, atol=1e-9)
    with np.errstate(invalid='ignore', over='ignore'):
        gx, gv = field_obs_grad_of_points(x, v, spec, G)
    assert np.all(gx[bad] == 0) and np.all(gv[bad] == 0) and np.all(np.isfinite(gx)) and np.all(np.isfinite(gv))
    assert np.any(gv[edge] != 0)
    gx1, gv1, ax, av = field_obs_grad_of_points(clean_x, clean_v, spec, G, terms=True)
    assert np.array_equal(gx1, gx[14:]) and np.array_equal(gv1, gv[14:]) and np.all(ax >= np.abs(gx1)) and np.all(av >= np.abs(gv1))


def test_fused_middle_weight_is_one_rounding_of_the_exact_value():
    rng = np.random.RandomState(1)
    t = np.concatenate([rng.uniform(0.5, 1.5, 4000), 1.0 + rng.uniform(-1, 1, 500) * 2.0 ** -rng.randint(1, 53, 500),
                        [0.5, 1.0, 1.5 - 2.0 ** -53, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, 1.0 + 2.0 ** -27, 1.0 + 3 * 2.0 ** -28]])
    d = t - 1.0
    got = fused_middle_weight(d)
    want = np.array([float(Fraction(0.75) - Fraction(float(q)) ** 2) for q in d])      # (Fraction -> float rounds once, to nearest even)
    assert np.array_equal(got, want)
    plain = 0.75 - d * d
    print(f'{int((plain != want).sum())} of {len(d)} two-rounding weights differ from the one-rounding ones')
    assert (plain != want).sum() > 0                         # the two are not the same function: the restatement has to use the fused one
