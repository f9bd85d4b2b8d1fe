"""fluidlab_amd/csrc/fe_math.h as compiled for the GPU, function by function (kernels: tests/csrc/math_device_test.hip; cases and references:
tests/math_cases.py).  Three things exist only in the device compile and are reached by nothing else in isolation:
  * fe_cbrt_pos / fe_pow_m23 on the hardware's log2, exp2 and reciprocal: every float32 of a binade against pow in float64, and the ends of the range;
  * svd3's rotations and sweeps that end on a vote over the wave: the contract on 440,000 matrices in mixed waves, and a lane's result held equal, float
    for float, whatever its 63 wave-mates hold and whether they call svd3 at all;
  * FMA contraction and the device's operation order in the constitutive model and its adjoint: against the fp64 build of the same header, relative to what
    the host fp32 build of the same header loses on the same inputs; the clamp's ties; and material classes mixed within a wave.
Measured on an MI355X: see DESIGN.md (parity table, row of this file)."""
import functools

import numpy as np
import pytest

import math_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return M.device_lib()


# ---------------------------------------------------------------------------------------------------------------------------------------
# cube root
# ---------------------------------------------------------------------------------------------------------------------------------------
def _units(got, J, power):
    return np.abs(got.astype(np.float64) / np.power(J.astype(np.float64), power) - 1.0) / M.UNIT


def test_cbrt_every_float_of_a_binade(dev):
    """every float32 in [0.5, 2) -- the mantissas of two binades, 2^24 values; a state worth simulating has J there -- and 20,000 over exp(+-7)"""
    lo, hi = np.float32(0.5).view(np.uint32), np.float32(2.0).view(np.uint32)
    J = np.concatenate([np.arange(lo, hi, dtype=np.uint32).view(np.float32), M.f32(np.exp(np.random.RandomState(3).uniform(-7, 7, 20000)))])
    assert J.size == 2 ** 24 + 20000
    rc, cb, pm = dev.cbrt(J)
    assert rc == 0
    e1, e2 = _units(cb, J, 1.0 / 3.0), _units(pm, J, -2.0 / 3.0)
    i1, i2 = int(np.nanargmax(e1)), int(np.nanargmax(e2))
    print(f'device fe_cbrt_pos worst {e1[i1]:.3f} units at J = {J[i1]!r}; fe_pow_m23 worst {e2[i2]:.3f} units at J = {J[i2]!r}')
    assert np.isfinite(cb).all() and np.isfinite(pm).all()
    assert e1[i1] <= 2.0                    # the host bound and the header's claim
    assert e2[i2] <= 5.0                    # the root's 2, one ulp of v_rcp_f32 (up to 2 units at the low end of a binade), the product's rounding


def test_cbrt_ends_of_the_range(dev):
    flt_min = np.finfo(np.float32).tiny
    J = M.f32([0.0, -0.5, -1e-30, -3e38, -np.inf, 1e-42, np.inf, flt_min, 3e38])
    rc, cb, pm = dev.cbrt(J)
    assert rc == 0
    print('device fe_cbrt_pos', dict(zip(J.tolist(), cb.tolist())))
    assert cb[0] == 0.0
    assert np.isnan(cb[1:5]).all() and np.isnan(pm[1:5]).all()
    assert np.isfinite(cb[5]) and 0.0 <= cb[5] < 1e-10                     # a denormal: the hardware's log2 flushes it, the root stays finite
    assert np.isposinf(cb[6])
    assert np.isfinite(cb[7:]).all() and (cb[7:] > 0).all() and (_units(cb[7:], J[7:], 1.0 / 3.0) <= 2.0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# SVD
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_svd_contract_in_mixed_waves(dev):
    """40,000 matrices of each kind, shuffled together: every wave holds a mixture, rotations are skipped by some lanes and taken by others"""
    F, kind = M.svd_cases()
    s_ref, det_ref = M.svd_reference()
    rc, U, sig, V = dev.svd(F)
    assert rc == 0
    M.assert_svd_contract(M.svd_contract(F, U, sig, V, s_ref, det_ref), kind, 'device')


@functools.lru_cache(None)
def _probes():
    """64 matrices: six of every kind (five of the two dullest), the zero matrix among them"""
    F, kind = M.svd_cases()
    take = [np.flatnonzero(kind == k)[:5 if M.SVD_KINDS[k] in ('zero', 'scaled_identity') else 6] for k in range(len(M.SVD_KINDS))]
    P = F[np.concatenate(take)]
    assert P.shape == (64, 3, 3) and (np.abs(P).max(axis=(1, 2)) == 0).any()
    return P


def _wave_run(dev, filler, lane, mask='all'):
    """One wave (64-lane workgroup) per probe: probe w sits in `lane` of wave w, the other lanes hold filler[w].  -> (rc, U, sig, V) of the 64 probes."""
    P = _probes()
    F = np.array(filler, dtype=np.float32).reshape(64, 64, 3, 3)
    F[np.arange(64), lane] = P
    m = np.zeros((64, 64), np.int32)
    if mask == 'all':
        m[:] = 1
    elif mask == 'odd':
        m[:, 1::2] = 1
    m[np.arange(64), lane] = 1
    rc, U, sig, V = dev.svd(F.reshape(-1, 3, 3), m.reshape(-1))
    sel = np.arange(64) * 64 + lane
    if mask != 'all':                                # lanes that did not call svd3 wrote nothing
        off = np.flatnonzero(m.reshape(-1) == 0)
        assert np.isnan(U[off]).all() and np.isnan(sig[off]).all()
    return rc, U[sel], sig[sel], V[sel]


def test_svd_lane_does_not_see_its_wave(dev):
    rng = np.random.RandomState(9)
    ident = np.tile(np.eye(3, dtype=np.float32), (64, 64, 1, 1))
    busy = np.where((np.arange(64) % 2 == 0)[None, :, None, None], M.svd_kind('generic', 64 * 64, rng).reshape(64, 64, 3, 3),
                    M.svd_kind('rank1', 64 * 64, rng).reshape(64, 64, 3, 3))
    runs = {'A identity mates, lane 17': _wave_run(dev, ident, 17),
            'B generic and rank-1 mates': _wave_run(dev, busy, 17),
            'C alone in its wave': _wave_run(dev, busy, 17, mask='only'),
            'C odd lanes only': _wave_run(dev, busy, 17, mask='odd')}
    for lane in (0, 31, 32, 63):
        runs[f'A identity mates, lane {lane}'] = _wave_run(dev, ident, lane)
        runs[f'B busy mates, lane {lane}'] = _wave_run(dev, busy, lane)
    # a partial last wave: n = 3 * 64 + 17, four probes per launch (lane 5 of each wave), only the probes' lanes active
    P = _probes()
    part = [np.empty((64, 3, 3), np.float32), np.empty((64, 3), np.float32), np.empty((64, 3, 3), np.float32)]
    rc_part = 0
    for g in range(16):
        n = 3 * 64 + 17
        F = busy.reshape(-1, 3, 3)[:n].copy()
        sel = np.arange(4) * 64 + 5
        F[sel] = P[4 * g:4 * g + 4]
        m = np.zeros(n, np.int32); m[sel] = 1
        rc, U, sig, V = dev.svd(F, m)
        rc_part = rc_part or rc
        for dst, src in zip(part, (U, sig, V)):
            dst[4 * g:4 * g + 4] = src[sel]
    runs['C partial last wave'] = (rc_part, *part)

    for name, r in runs.items():
        assert r[0] == 0, name
    ref = runs['A identity mates, lane 17']
    assert all(np.isfinite(a).all() for a in ref[1:])
    for name, r in runs.items():
        for what, a, b in zip(('U', 'sig', 'V'), ref[1:], r[1:]):
            assert np.isfinite(b).all(), (name, what)
            bad = np.flatnonzero((a != b).reshape(64, -1).any(axis=1))          # (== on floats: -0 equals +0, an identity rotation may turn one into the other)
            assert bad.size == 0, f'{name}: {what} of probes {bad.tolist()} differs from the run among identities, by up to {np.abs(a - b).max():.3g}'
    # and the contract holds for the probes themselves
    s_ref = np.linalg.svd(P.astype(np.float64), compute_uv=False)
    c = M.svd_contract(P, *ref[1:], s_ref, np.linalg.det(P.astype(np.float64)))
    assert c['recon'].max() <= 3e-6 and c['orth'].max() <= 3e-6 and c['sigma'].max() <= 3e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
# constitutive model and adjoint
# ---------------------------------------------------------------------------------------------------------------------------------------
_DEV_OUT = {}


def _dev_class(dev, label, general=True):
    """the device's outputs for one class, launched once per module"""
    if (label, general) not in _DEV_OUT:
        _DEV_OUT[label, general] = dev.constitutive(M.constitutive_class(label), general=general)
    return _DEV_OUT[label, general]


@pytest.mark.parametrize('label,general', [(c, True) for c in sorted(M.CLASSES)] + [('a', False)])
def test_constitutive_device_against_fp64(dev, label, general):
    """device fp32 against the fp64 build, bounded by 4 x what the host fp32 build of the same header loses on the same inputs (held under its own cap by
    tests/test_csrc_math_cases.py): the factor covers two rounding realisations -- FMA contraction, operation order -- of one fp32 algorithm in a maximum over
    2,000 heavy-tailed draws; a device error beyond it is a finding."""
    cs = M.constitutive_class(label)
    rc, od = _dev_class(dev, label, general)
    assert rc == 0
    _, oh = dev.constitutive(cs, general=general, suffix='_host')
    _, o64 = M.f64_lib().constitutive(cs, suffix='_host')
    ed, eh = M.class_errors(od, o64), M.class_errors(oh, o64)
    print(f'class ({label}) GENERAL={general} device/host error vs fp64: ' +
          ' '.join(f'{k} {ed[k]:.3g}/{eh[k]:.3g}={ed[k] / eh[k]:.2f}' for k in M.BLOCKS + ('J',)))
    for k in M.CONST_OUT:
        assert np.isfinite(od[k]).all(), k
    assert np.array_equal(od['full'], o64['full'])
    for k in M.BLOCKS + ('J',):
        assert ed[k] <= 4.0 * eh[k], (label, k, ed[k], eh[k])


def test_clamp_ties_on_the_device(dev):
    """a sigma exactly on a clamp edge, and one float32 step to either side: the device's pass decision is the fp64 build's (and Taichi's tie rule)"""
    t = M.tie_cases()
    rc, od = dev.constitutive(t['cs32'])
    assert rc == 0
    rc64, o64 = M.f64_lib().constitutive(t['cs64'], suffix='_host')
    assert rc64 == 0
    at = t['where'] == 'at'
    edges = np.where(t['edge'] == 'lo', M.CLAMP_LO, M.CLAMP_HI)
    assert ((od['sig'] == edges[:, None]).any(axis=1) == at).all()                 # svd3 returned the sigma exactly: the tie is a tie
    pd, dd = M.tie_decisions(od, t['proj'])
    p64, d64 = M.tie_decisions(o64, t['proj'])
    print('device tie projections: at', pd[at].round(6).tolist()[:6], '... off', pd[~at].round(6).tolist()[:6])
    assert np.abs(pd - dd).max() < 1e-5 and np.abs(p64 - d64).max() < 1e-12        # 0 or 1, nothing between
    assert np.array_equal(dd, d64)
    assert np.array_equal(dd, t['expect'])


def test_mixed_material_waves(dev):
    """(a), (c) and (e) interleaved lane by lane -- if (k.full) and the material branches diverge in every wave -- against one launch per class"""
    labels = ('a', 'c', 'e')
    per = [M.constitutive_class(l) for l in labels]
    n = len(per[0]['mu'])
    mixed = {k: np.stack([p[k] for p in per], axis=1).reshape((3 * n,) + per[0][k].shape[1:]) for k in ('C', 'F', 'GA', 'Fg', 'mu', 'lam', 'cls')}
    assert (mixed['cls'][:6] == [M.LIQUID, M.ELASTIC, M.PLASTO] * 2).all()
    rc, om = dev.constitutive(mixed)
    assert rc == 0
    for j, l in enumerate(labels):
        rc1, o1 = _dev_class(dev, l)
        assert rc1 == 0
        for k in M.CONST_OUT:
            a, b = om[k][j::3], o1[k]
            assert np.isfinite(a).all() and np.isfinite(b).all(), (l, k)
            bad = np.flatnonzero((a != b).reshape(n, -1).any(axis=1))
            assert bad.size == 0, f'class ({l}) {k}: {bad.size} cases differ between the mixed and the per-class launch, first {bad[:5].tolist()}'
