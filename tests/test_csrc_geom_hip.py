"""The geometry and contact half of fluidlab_amd/csrc/fe_math.h as compiled for the GPU, function by function (kernels: tests/csrc/geom_device_test.hip;
cases and references: tests/geom_cases.py; the CPU half, which holds the fp64 build against numpy and finite differences and caps the host fp32 build, is
tests/test_csrc_geom_cases.py).  The device runs against the fp64 build of the same header on the same float32 words, class by class: each output block
within 4 x what the host fp32 build loses on that class (the factor of test_constitutive_device_against_fp64: two rounding realisations -- FMA contraction,
operation order -- of one fp32 algorithm in a maximum over a heavy-tailed sample); every flag, multiplier, base and 0 / 1 Jacobian entry equal.
Measured on an MI355X: see DESIGN.md (parity table, row of this file)."""
import numpy as np
import pytest

import geom_cases as G
from test_csrc_geom_cases import MEASURED, boundary_ties, flat_cell_properties, radial_ties

pytestmark = pytest.mark.gpu

ULP = 6e-8                  # one float32 step at 1: the floor under "4 x the host's error" where the host happens to round exactly


@pytest.fixture(scope='module')
def dev():
    return G.device_lib()


_DEV = {}


def _dev_class(dev, key):
    """the device's outputs for one class, launched once per module"""
    if key not in _DEV:
        cs = G.collide_class(*key)
        _DEV[key] = G.run_collide(dev, G.colliders()[key[0]], cs['x'], cs['fs'], device=True)
    return _DEV[key]


@pytest.mark.parametrize('key', G.CLASS_KEYS, ids=lambda k: f'{k[0]}-{k[1]}')
def test_collide_device_against_fp64(dev, key):
    col, cs = G.colliders()[key[0]], G.collide_class(*key)
    od = _dev_class(dev, key)
    oh, o64 = G.run_collide(dev, col, cs['x'], cs['fs']), G.run_collide(G.f64_lib(), col, cs['x'], cs['fs'])
    ed, eh = G.collide_errors(od, o64), G.collide_errors(oh, o64)
    print(f'MEASURED {key} device/host error vs fp64: out {ed["out"]:.3g}/{eh["out"]:.3g} J {ed["J"]:.3g}/{eh["J"]:.3g}')
    assert np.isfinite(od['out']).all() and np.isfinite(od['J']).all()
    assert np.array_equal(od['hit'], o64['hit'])
    # the host's error counts for no more than the cap the CPU test holds it under: an A/B library with a wrong header is wrong in its host half too
    cap_out, cap_J = (3 * m for m in MEASURED[key])
    assert ed['out'] <= 4.0 * min(eh['out'], cap_out) and ed['J'] <= 4.0 * min(eh['J'], cap_J), (key, ed, eh)


def test_collide_ties_on_the_device(dev):
    """sd exactly 0, infl exactly at its cap of 1, one step to either side, and either side of the soft edge infl = 0.1, frictional and sticky: the device's
    hit flags equal the fp64 build's (and the expected ones) on every tie, its values the host fp32 build's to rounding"""
    col = G.tie_collider()
    x, fs, hit = G.collide_ties()
    od, oh, o64 = G.run_collide(dev, col, x, fs, device=True), G.run_collide(dev, col, x, fs), G.run_collide(G.f64_lib(), col, x, fs)
    assert np.array_equal(od['hit'], o64['hit']) and np.array_equal(od['hit'].astype(bool), hit)
    assert np.isfinite(od['out']).all() and np.isfinite(od['J']).all()
    ed, eh = np.abs(od['out'] - o64['out']).max(), np.abs(oh['out'] - o64['out']).max()
    print(f'MEASURED collide ties device/host error vs fp64: out {ed:.3g}/{eh:.3g}')
    assert ed <= 4.0 * max(eh, ULP)
    assert np.array_equal(od['out'][~hit].astype(np.float64), x[~hit][:, G.MV])


@pytest.mark.parametrize('cname', ['thin', 'scaled'])
def test_flat_cell_layer_on_the_device(dev, cname):
    """Hits in the layer of voxel cells that straddles the plate's mid-plane (res = 28 is even: equal corner values on both sides, a flat trilinear field, a
    central difference that is 0 in fp64 and rounding noise of 5e-7 against sqrt(FE_EPS) = 1e-6 in fp32).  The normal is an arbitrary vector there, the device's
    as much as the host's, so NOTHING is asserted about agreement with fp64; what is asserted holds for any normal of length at most 1 (the contact law never
    lengthens the relative velocity, see flat_cell_properties) and that everything is finite."""
    col = G.colliders()[cname]
    for vi in (0, 1, 2):
        fl = G.collide_class(cname, vi)['flat']
        c, _ = G.classify(col, fl['x'], fl['fs'])
        od = G.run_collide(dev, col, fl['x'], fl['fs'], device=True)
        assert od['hit'].all()
        rc, (_, _, nrm), _ = dev.run('sdf', [c[:, G.C_PV]], collider=col, device=True)          # sdf_normal in the layer: any direction, never longer than 1
        assert rc == 0 and np.isfinite(nrm).all() and (np.linalg.norm(nrm.astype(np.float64), axis=1) <= 1 + 1e-6).all(), (cname, vi)
        flat_cell_properties(od, fl['x'], fl['fs'], c, fl['branch'], (cname, vi, 'device'), False)


@pytest.mark.parametrize('cname', ['thin', 'sphere'])
def test_mixed_collide_waves(dev, cname):
    """slide / stick / separating, soft, and sticky cases with their misses interleaved lane by lane (friction and softness are per lane), the last wave
    partial: every lane's result equal, float for float, to the launch of its own class"""
    n = 1983                                                                            # 4 n = 123 x 64 + 60
    per = [G.collide_class(cname, vi) for vi in range(4)]
    x = np.stack([p['x'][:n] for p in per], axis=1).reshape(4 * n, 20)
    fs = np.stack([p['fs'][:n] for p in per], axis=1).reshape(4 * n, 2)
    assert (4 * n) % 64 != 0 and (fs[:4, 0] == G.w32([v[0] for v in G.VARIANTS])).all()
    om = G.run_collide(dev, G.colliders()[cname], x, fs, device=True)
    for vi in range(4):
        o1 = _dev_class(dev, (cname, vi))
        for k in ('out', 'J', 'hit'):
            a, b = om[k][vi::4], o1[k][:n]
            assert np.isfinite(a).all()
            bad = np.flatnonzero((a != b).reshape(n, -1).any(axis=1))
            assert bad.size == 0, f'{cname} variant {vi} {k}: {bad.size} cases differ between the mixed and the per-class launch, first {bad[:5].tolist()}'


def _within(dev_out, host_out, ref, what, scale=None):
    """device error <= 4 x host fp32 error (floor: one float32 step of the field's range), both against the fp64 build"""
    scale = np.abs(ref).max() if scale is None else scale
    ed, eh = np.abs(dev_out.astype(np.float64) - ref).max() / scale, np.abs(host_out.astype(np.float64) - ref).max() / scale
    print(f'MEASURED {what} device/host error vs fp64: {ed:.3g}/{eh:.3g}')
    assert np.isfinite(dev_out).all(), what
    assert ed <= 4.0 * max(eh, ULP), (what, ed, eh)


def test_sdf_contact_law_static_collide_on_the_device(dev):
    f = G.f64_lib()
    for cname in ('thin', 'odd', 'sphere', 'scaled'):
        col = G.colliders()[cname]
        for pv, edge in ((G.sdf_points(cname), False), (G.sdf_edge_points(col), True)):
            (rd, od, _), (rh, oh, _), (_, o64, _) = (lib.run('sdf', [pv], collider=col, device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
            assert rd == 0 and rh == 0
            for j, name in enumerate(('sdf_sample', 't_sdf_sample', 'sdf_normal')):
                if not (edge and j == 2):                                               # a normal sampled across a face of the voxel box is a kink
                    _within(od[j], oh[j], o64[j], f'{cname} {name}{" edges" if edge else ""}', scale=1.0)
            assert np.array_equal(od[0] == 1.0, o64[0] == 1.0) and np.array_equal(od[1] == 1.0, o64[1] == 1.0)          # outside decided alike, ties included
    n, rv, g, fr = G.contact_law_cases()
    (rd, od, _), (_, oh, _), (_, o64, _) = (lib.run('contact_law', [n, rv, g, fr], device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
    assert rd == 0
    _within(od[0], oh[0], o64[0], 'contact_law out')
    _within(od[1], oh[1], o64[1], 'contact_law pull-back')
    assert np.array_equal((od[0] == 0).all(axis=1), (o64[0] == 0).all(axis=1))          # stick decided alike
    col, cs = G.colliders()['sphere'], G.collide_class('sphere', 0)
    pos = G.w32(G.qrot(cs['x'][:, G.POS] - cs['x'][:, G.P0], G.qconj_n(cs['x'][:, G.Q0])))          # the mesh-frame point as a world position: no pose
    ident = np.tile([0.0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0], (len(pos), 1))
    c, hit = G.classify(col, np.concatenate([ident, pos, cs['x'][:, G.MV]], axis=1), cs['fs'], dt=1e30)          # cv = 0: the static collider's margins
    sure = G.verdict(col, c, hit, cs['fs'])[0]
    pos, v, ff, gg = pos[sure], cs['x'][sure][:, G.MV], cs['fs'][sure][:, :1], g[:sure.sum()]
    assert sure.sum() >= 1500 and hit[sure].sum() >= 100
    (rd, od, _), (_, oh, _), (_, o64, _) = (lib.run('static_collide', [pos, v, gg, ff], collider=col, device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
    assert rd == 0 and (o64[0] != v).any()
    _within(od[0], oh[0], o64[0], 'static_collide v')
    _within(od[1], oh[1], o64[1], 'static_collide pull-back')


def test_quaternions_on_the_device(dev):
    f = G.f64_lib()
    wq, hand = G.move_quat_cases()
    for cases, what in ((wq, 'drawn'), (hand, 'w = 0 and |w| = 1e-7')):
        (rd, od, _), (_, oh, _), (_, o64, _) = (lib.run('move_quat', [cases], device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
        assert rd == 0
        _within(od[0], oh[0], o64[0], f't_move_quat {what}')
        _within(od[1], oh[1], o64[1], f't_move_quat<Dual> {what}')
    rng = np.random.RandomState(3)
    n = 2000
    ins = [G.w32(G.unit_quats(rng, n)), G.w32(G.unit_quats(rng, n)), G.w32(rng.normal(size=(n, 3))), G.w32(rng.normal(size=(n, 3)))]
    ins[2][:3] = [[0, 0, 0], [1e-7, 0, 0], [0, 0, -1e-7]]
    (rd, od, _), (_, oh, _), (_, o64, _) = (lib.run('quat', ins, device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
    assert rd == 0
    for j, name in enumerate(('quat_mul', 'quat_from_w', 'quat_rotate')):
        _within(od[j], oh[j], o64[j], name)


@pytest.mark.parametrize('bname', sorted(G.BOUNDARIES))
def test_boundaries_on_the_device(dev, bname):
    """multipliers, is_out and the 0 / 1 entries of the Jacobian equal to the fp64 build's on every margin-respecting case and every hand-written tie; the
    cylinder's wall within an ulp is decided by FE_EPS under the root, which fp32 cannot see: there the device equals the host fp32 build"""
    f = G.f64_lib()
    b, x, v = G.boundary_cases(bname)
    tx, tv = boundary_ties(b)
    for xx, vv, tie in ((x, v, False), (tx, tv, True)):
        (rd, od, iod), (_, oh, ioh), (_, o64, io64) = (lib.run('boundary', [xx, vv], bnd=b, device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
        assert rd == 0
        rad = radial_ties(b, len(xx)) if tie else np.zeros(len(xx), bool)
        assert np.array_equal(od[1][rad], oh[1][rad]) and np.array_equal(iod[0][rad], ioh[0][rad])
        if rad.any():                                   # (J beyond the wall is k - k3 rx^2, about 1 - 1: a dozen fp32 roundings of numbers up to 1)
            assert np.abs(od[3][rad] - oh[3][rad]).max() <= 1e-6
        k, J, out = od[1][~rad], od[3][~rad], iod[0][~rad]
        assert np.array_equal(k, o64[1][~rad]) and np.array_equal(out, io64[0][~rad])
        unit = (o64[3][~rad] == 0) | (o64[3][~rad] == 1)
        assert np.array_equal(J[unit], o64[3][~rad][unit])
        for j, name in ((0, 'v'), (2, 'xn'), (3, 'J')):
            _within(od[j][~rad], oh[j][~rad], o64[j][~rad], f'boundary {bname} {name}{" ties" if tie else ""}', scale=1.0)


def test_stencil_on_the_device(dev):
    f = G.f64_lib()
    x = G.stencil_cases()
    (rd, od, iod), (_, oh, _), (_, o64, io64) = (lib.run('stencil', [x], inv_dx=16.0, n_grid=16, device=dv) for lib, dv in ((dev, True), (dev, False), (f, False)))
    assert rd == 0 and np.array_equal(iod[0], io64[0]) and np.array_equal(iod[1], io64[1])
    for j, name in enumerate(('fx', 'w', 'dw')):
        _within(od[j], oh[j], o64[j], f'stencil {name}', scale=1.0)
    t = G.stencil_ties()                                                                # one float32 step from an integer: the float32 truncation is the reference
    base, fx, w, dw, inside = G.stencil_reference(t, 16, np.float32)
    rd, od, iod = dev.run('stencil', [t], inv_dx=16.0, n_grid=16, device=True)
    assert rd == 0 and np.array_equal(iod[0], base) and np.array_equal(iod[1][:, 0].astype(bool), inside)
    assert np.abs(od[0] - fx).max() <= 4e-6 and np.abs(od[1].reshape(-1, 3, 3) - w).max() <= 4e-6


def test_stencil_inside_rejects_wild_coordinates(dev):
    """1e30, -1e30, +inf and -inf in any one dimension: v_cvt_i32_f32 saturates them and stencil_inside compares without adding to the base, so none is
    reported inside.  NaN is converted to base 0, which passes the range test: the device reports such a particle inside (the x86 cast gives INT_MIN and
    rejects it).  A guard moves the register budgets of the substep kernels ("flat cell layer and NaN positions"), so the behaviour is recorded
    and pinned here: inside, base 0 in that dimension (in bounds), fx and all three weights of that dimension NaN -- whatever such a particle deposits or
    gathers is NaN, not a wrong number.  A later guard in stencil_inside has to change this test with it."""
    x = np.full((3 * len(G.STENCIL_WILD), 3), 0.53125)
    for j, wild in enumerate(G.STENCIL_WILD):
        x[3 * j + np.arange(3), np.arange(3)] = wild
    rd, od, iod = dev.run('stencil', [x], inv_dx=16.0, n_grid=16, device=True)
    assert rd == 0
    print('MEASURED stencil bases of 1e30, -1e30, inf, -inf, NaN:', iod[0][np.arange(0, len(x), 3), 0].tolist(), 'inside:', iod[1][:, 0].tolist())
    is_nan = np.isnan(x).any(axis=1)
    assert not iod[1][~is_nan].any(), x[~is_nan][iod[1][~is_nan, 0] != 0]
    for r in np.flatnonzero(is_nan):
        d = int(np.flatnonzero(np.isnan(x[r]))[0])
        assert iod[1][r, 0] == 1 and iod[0][r, d] == 0 and np.isnan(od[0][r, d]) and np.isnan(od[1][r].reshape(3, 3)[:, d]).all()
