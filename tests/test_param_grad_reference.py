"""The yardstick of the material-parameter gradient tests (test_param_grad_hip.py): central finite differences of the fp64 oracle with
respect to per-particle mu, lam and rho (param_grad_common.py).  For every scene and direction used there, D at the step h and at h / 2
must agree -- the finite difference is a derivative at these points: no particle sits on the plastic clamp's kink or at coinciding
singular values within the step.  No GPU, and nothing of the feature itself: this passes without it.

Measured (worst direction per scene, |D(h/2) - D(h)| / max(|D(h)|, 1e-3 max |D| of the parameter)): water 2.8e-5 (mu, random signs: |D| =
6e-9, rounding), mixed 4.6e-6 (lam of ICECREAM), latte 3.0e-7.  That is the noise floor of the reference; the bound below is two orders
under the 1e-2 class the engine is held to.
"""
import pytest

import param_grad_common as P

FLOOR = 1e-4


@pytest.mark.parametrize('name', ['water', 'mixed', 'latte'])
def test_finite_difference_is_a_derivative(oracle64, name):
    a, b = P.reference(oracle64, name), P.reference(oracle64, name, shrink=0.5)
    dev = P.deviation(b, a)
    for key in sorted(a):
        print(f'MEASURED param_grad reference[{name}] {key}: D(h) {a[key]:.6e} D(h/2) {b[key]:.6e} deviation {dev[key]:.2e}')
    sc = P.scene(name)
    assert len(a) == 3 * (len(set(int(m) for m in sc['mat'])) + (name != 'latte'))          # every direction, none dropped
    assert all(abs(v) > 0 for v in a.values()), a                                            # ... and each one moves the objective
    worst = max(dev, key=dev.get)
    assert dev[worst] <= FLOOR, (worst, dev[worst])
