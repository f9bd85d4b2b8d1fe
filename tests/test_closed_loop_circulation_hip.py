"""The closed loop on Circulation-v0 on the GPU: the parameter gradient of the device road (fe_smoke_obs_get_dev / fe_smoke_obs_add_grad_dev, the
action and its adjoint read on the device) against the fp64 oracle's and against the HIP engine's own dense road.

Scene and policy: tests/test_closed_loop_circulation_oracle.py's, at horizon 4 as the parity figures are recorded, and at that file's horizon 6,
where the observation adjoint is not zero.  sm_trilerp_grad accumulates with fp32 atomics in an order that varies from run to run, so the
yardsticks are measured in the same test:
  device road against the fp64 oracle   <= 2 x (fp32 oracle against fp64 oracle) + 2 x (two runs of the HIP dense road against each other)
  device road against the dense road    <= 2 x that run-to-run distance
(all relative L2 over the parameter gradient; profiles/closed_loop_parity.txt section 4 has the figures; at horizon 6, which the parity
record does not set, the second bound takes the larger of the run-to-run distance and the fp32 oracle's own: see the comment there).
Measured: horizon 4  fp32 oracle 9.2e-7, run to run 0, device road against fp64 2.1e-7, against the dense road 0 (the same bits);
          horizon 6  fp32 oracle 4.0e-7, run to run 2.2e-7, device road against fp64 3.8e-7, against the dense road 0.  Nothing in the device loop downloads
a field: smoke_get_frame raises while it runs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import scenarios as S  # noqa: E402
import test_closed_loop_circulation_oracle as T  # noqa: E402

pytestmark = pytest.mark.gpu


def _gradient(lib, horizon, device_road=False, forbid_downloads=False):
    T_H, T.H = T.H, horizon
    try:
        env, pol, sol = T.build(lib, None)
    finally:
        T.H = T_H
    te = env.taichi_env
    state = te.get_state()['state']
    if lib is None:
        env.enable_device_loss()                                 # (both HIP roads: the roads differ in how the observation travels)
    if device_road:
        env.enable_device_obs()
        assert sol._device_road() and pol.device.type == 'cuda' and pol.dtype == torch.float32
    eng = te.simulator.engine
    if forbid_downloads:
        def refuse(*a, **k):
            raise AssertionError('the device road downloaded a smoke field')
        keep, eng.smoke_get_frame = eng.smoke_get_frame, refuse
    try:
        info = sol.forward_backward(state)
    finally:
        if forbid_downloads:
            eng.smoke_get_frame = keep
    g = sol.grad_vector()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    return info['loss'], g


@pytest.mark.parametrize('horizon', [4, T.H], ids=['h4', 'h6'])
def test_device_road_gradient(hiplib, oracle32, oracle64, horizon):
    l64, g64 = _gradient(oracle64, horizon)
    l32, g32 = _gradient(oracle32, horizon)
    la, ga = _gradient(None, horizon)
    lb, gb = _gradient(None, horizon)
    ld, gd = _gradient(None, horizon, device_road=True, forbid_downloads=horizon < 6)      # (at the env's full horizon the window's checkpoint is a download)
    own, run = S.rel_l2(g32, g64), S.rel_l2(ga, gb)
    to64, to_dense, dense64 = S.rel_l2(gd, g64), S.rel_l2(gd, ga), S.rel_l2(ga, g64)
    print(f'MEASURED closed loop on Circulation, horizon {horizon}: loss fp64 {l64!r} fp32 {l32!r} hip dense {la!r} hip device {ld!r}; '
          f'fp32 oracle vs fp64 {own:.3e}; hip dense run to run {run:.3e}; hip dense vs fp64 {dense64:.3e}; '
          f'device road vs fp64 {to64:.3e} (ratio to the fp32 oracle\'s {to64 / own if own else float("nan"):.3f}); device road vs dense {to_dense:.3e}')
    assert np.isfinite([l64, l32, la, lb, ld]).all()
    assert to64 <= 2 * own + 2 * run, (to64, own, run)
    if horizon == 4:
        assert to_dense <= 2 * run, (to_dense, run)
    else:
        # Two dense runs differ only when the atomics of sm_trilerp_grad happened to land in another order: measured 2.2e-7 one time, and
        # the same bits another.  A pair that happened to agree says nothing about a third run, so at this horizon the yardstick for
        # "differs by fp32 summation order alone" is the larger of that distance and the fp32 oracle's own distance from fp64 (4.0e-7).
        assert to_dense <= 2 * max(run, own), (to_dense, run, own)
