"""fluidlab_amd/csrc/fe_math.h per function, the part that needs no GPU (tests/math_cases.py holds the cases and references):
the test kernels of tests/csrc/math_device_test.hip cross-compile for gfx950; the host fp32 svd3 meets the contract of tests/csrc/math_test.cpp on
40,000 matrices of every kind (rank-deficient, reflected, equal-sigma, clamp-band ... -- 440,000 instead of 2,000); the host fp32 constitutive model and
its adjoint stay within a measured cap of the fp64 build, class by class, so that the GPU test (tests/test_csrc_math_hip.py), which bounds the device
relative to the host fp32 build, is not relative to something that is itself wrong; and the fp64 build's forward pass agrees with numpy, which ties
the adjoint reference to something that is not the header."""
import numpy as np
import pytest

import math_cases as M

pytestmark = pytest.mark.skipif(M.hipcc() is None, reason='hipcc not available')

# Host fp32 against host fp64: class maximum over 2,000 cases of max|a - b| / max|b| per 3x3 block.  MEASURED is what this deterministic CPU run gives
# (the x86-64 half of the device library, i.e. the engine's flags; no FMA contraction there); the cap asserted is 3 x MEASURED.
MEASURED = {
    'a': dict(affine=3.49e-5, Fnew=1.52e-7, gC=4.80e-7, gF=3.13e-4),      # (affine, gF: the liquid's lam J (J - 1) with J within 2 % of 1)
    'b': dict(affine=3.63e-6, Fnew=3.59e-7, gC=4.73e-6, gF=3.83e-6),
    'c': dict(affine=3.77e-6, Fnew=1.86e-7, gC=9.40e-7, gF=7.48e-7),
    'd': dict(affine=4.86e-6, Fnew=1.71e-7, gC=1.98e-6, gF=1.95e-6),
    'e': dict(affine=1.15e-4, Fnew=6.42e-7, gC=1.15e-3, gF=1.26e-3),      # (sigma gaps down to ~1e-4 after F_tmp = (I + dt C) F: 1 / (s_j^2 - s_i^2))
    'f': dict(affine=1.23e-5, Fnew=4.28e-7, gC=8.26e-6, gF=1.76e-5),
}
WELL_GAPPED = ('b', 'c', 'f')          # gaps >= 0.05: fp32 eps x 1/gap x a dozen operations
WELL_GAPPED_CAP = 2e-5


def test_device_library_cross_compiles():
    import os
    lib = M.build_device_lib()
    assert os.path.getsize(lib) > 0
    with open(lib, 'rb') as f:
        blob = f.read()
    for k in (b'k_cbrt', b'k_svd', b'k_constitutive', b'gfx950'):
        assert k in blob, k
    d = M.device_lib()
    assert d.real is np.float32 and M.f64_lib().real is np.float64
    for name in ('mdt_cbrt', 'mdt_svd', 'mdt_constitutive', 'mdt_cbrt_host', 'mdt_svd_host', 'mdt_constitutive_host'):
        assert hasattr(d.lib, name), name


def test_host_svd_contract():
    F, kind = M.svd_cases()
    s_ref, det_ref = M.svd_reference()
    rc, U, sig, V = M.device_lib().svd(F, suffix='_host')
    assert rc == 0
    M.assert_svd_contract(M.svd_contract(F, U, sig, V, s_ref, det_ref), kind, 'host fp32')


def test_host_cbrt_matches_math_test_bounds():
    """the host branch over the inputs of the GPU test's sample (the exhaustive binades are the device's business): 2 and 4 units, as math_test.cpp"""
    rng = np.random.RandomState(3)
    J = M.f32(np.exp(rng.uniform(-7, 7, 20000)))
    rc, cb, pm = M.device_lib().cbrt(J, suffix='_host')
    assert rc == 0
    J64 = J.astype(np.float64)
    e1 = np.abs(cb / np.power(J64, 1 / 3) - 1).max() / M.UNIT
    e2 = np.abs(pm / np.power(J64, -2 / 3) - 1).max() / M.UNIT
    print(f'host fp32 fe_cbrt_pos {e1:.3f} units, fe_pow_m23 {e2:.3f} units')
    assert e1 <= 2.0 and e2 <= 4.0


@pytest.mark.parametrize('label', sorted(M.CLASSES))
def test_host_fp32_against_fp64(label):
    cs = M.constitutive_class(label)
    rc32, o32 = M.device_lib().constitutive(cs, suffix='_host')
    rc64, o64 = M.f64_lib().constitutive(cs, suffix='_host')
    assert rc32 == 0 and rc64 == 0
    assert np.array_equal(o32['full'], o64['full']) and (o32['full'] == (0 if label == 'a' else 1)).all()
    err = M.class_errors(o32, o64)
    print(f'class ({label}) host fp32 vs fp64: ' + ' '.join(f'{k} {err[k]:.3g}' for k in M.BLOCKS + ('J',)))
    for k in M.BLOCKS:
        assert err[k] <= 3.0 * MEASURED[label][k], (label, k, err[k], MEASURED[label][k])
        if label in WELL_GAPPED:
            assert err[k] <= WELL_GAPPED_CAP, (label, k, err[k])


def test_host_liquid_specialisation_matches_general():
    """class (a) through GENERAL = false (the engine's all-inviscid-liquid build) gives the floats of GENERAL = true on the host"""
    cs = M.constitutive_class('a')
    _, g = M.device_lib().constitutive(cs, general=True, suffix='_host')
    _, s = M.device_lib().constitutive(cs, general=False, suffix='_host')
    for k in M.CONST_OUT:
        assert np.array_equal(g[k], s[k]), k


@pytest.mark.parametrize('label', sorted(M.CLASSES))
def test_fp64_forward_against_numpy(label):
    cs = M.constitutive_class(label)
    rc, o = M.f64_lib().constitutive(cs, suffix='_host')
    assert rc == 0
    ref = M.numpy_forward(cs)
    # "relative" for affine: to the largest term of its sum (math_cases.numpy_forward).  Relative to the sum itself class (e), whose stress terms cancel
    # to 1/700, reads 2.0e-12: thirteen fp64 roundings of the Jacobi rotations in U V^T, amplified by that cancellation -- not a disagreement.
    errs = dict(affine=(np.abs(o['affine'] - ref['affine']).max(axis=(1, 2)) / ref['affine_scale']).max(), J=M.block_err(o['J'], ref['J']).max())
    if label != 'a':                                  # (a) takes no SVD: sig is not computed
        errs['sig'] = (np.abs(np.abs(o['sig']) - ref['sig']).max(axis=1) / ref['sig'][:, 0]).max()
    if 'Fnew' in ref:
        errs['Fnew'] = M.block_err(o['Fnew'], ref['Fnew']).max()
    print(f'class ({label}) fp64 header vs numpy: ' + ' '.join(f'{k} {v:.3g}' for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-12, (label, k, v)


def test_tie_cases_on_the_host():
    """the hand-made clamp ties: the exact sigma comes back from svd3, and host fp32 and fp64 both decide as Taichi's tie rule says"""
    t = M.tie_cases()
    rc32, o32 = M.device_lib().constitutive(t['cs32'], suffix='_host')
    rc64, o64 = M.f64_lib().constitutive(t['cs64'], suffix='_host')
    assert rc32 == 0 and rc64 == 0
    at = t['where'] == 'at'
    edges32 = np.where(t['edge'] == 'lo', M.CLAMP_LO, M.CLAMP_HI)
    assert ((o32['sig'] == edges32[:, None]).any(axis=1) == at).all()              # fp32: a sigma equal to the fp32 edge exactly where one was put
    edges64 = np.where(t['edge'] == 'lo', 1.0 - 2e-3, 1.0 + 3e-3)
    assert ((o64['sig'] == edges64[:, None]).any(axis=1) == at).all()
    for o in (o32, o64):
        p, dec = M.tie_decisions(o, t['proj'])
        assert np.abs(p - dec).max() < 1e-5                                       # the projection is 0 or 1
        assert np.array_equal(dec, t['expect'])
    assert not t['expect'][at].any() and t['expect'][~at].sum() == (~at).sum() // 2
