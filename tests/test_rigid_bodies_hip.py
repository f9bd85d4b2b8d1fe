"""GPU: k_rigid_body (MAT_RIGID shape matching, forward and adjoint) beyond one pass of its 256-thread workgroup.

scenarios.rigid_bodies_many has eight bodies of 40 .. 700 particles (1, 2 and 3 passes, tails of every kind), optionally with
unused particles scattered through two bodies, one body unused as a whole, or all pids interleaved.  The kernel is checked
  (a) alone: its output against a numpy fp64 chain fed with exactly the x[f], used, v[f+1] the engine holds, bounded by
      what the same chain loses in fp32;
  (b) in an 8-substep rollout, forward and adjoint, against the fp64 oracle, bounded by twice what the fp32 oracle loses
      (test_rigid_bodies_oracle.py shows those yardsticks sit far inside the 1e-2 cap), for sort_interval 0 / 1 / 3 and
      both reverse sweeps -- the ranged one writes the adjoint across a sort boundary in the next substep's order;
  (c) with a body that has no used particle;  (d) after fe_init_particles replaced eight bodies by three on one handle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402
import rigid_cases as RC  # noqa: E402
from fluidlab_amd.scenes import material_props  # noqa: E402

pytestmark = pytest.mark.gpu


def _fused(x, dt, v):
    """fl(x + dt v) with one rounding (v_fma_f32): the product of two fp32 numbers is exact in fp64"""
    return (x.astype(np.float64) + np.float64(np.float32(dt)) * v.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize('K', [0, 1])
@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave'])
def test_kernel_alone_forward(hiplib, variant, K):
    """One substep at f = 0 and, bodies mid-tumble and slots shuffled by the sort, at f = 5.  Only the kernel's arithmetic
    (fp64 sums, fp32 SVD, fp32 rotation) stands between the engine's x[f+1] and the fp64 chain; the fp32 chain's distance
    e32 from the fp64 one is the yardstick: max|dx| <= 2 e32 + 2^-23 per body (2: the upper end, 1.6, of the band the
    device's SVD was measured in against the host's fp32 build, DESIGN.md section 2, rounded up; 2^-23: one ulp at 1)."""
    sc = RC.scene(variant)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': K})
    bid, dt = sc['body_id'], sc['dt']
    for f in range(6):
        a = S.get_state(eng, f)
        eng.substep(f, f, 0)
        if f not in (0, 5):
            continue
        b = S.get_state(eng, f + 1)
        assert (a['used'] == sc['used']).all() and (b['used'] == sc['used']).all()
        ref = RC.shape_match(a['x'], b['v'], a['used'], bid, dt, np.float64)
        lo = RC.shape_match(a['x'], b['v'], a['used'], bid, dt, np.float32)
        assert sorted(ref) == list(RC.bodies(sc))
        for body, (sel, want) in ref.items():
            e32 = float(np.abs(lo[body][1] - want).max())
            bound = 2 * e32 + 2.0 ** -23
            err = float(np.abs(b['x'][sel] - want).max())
            derr = float(np.abs(RC.pairwise(b['x'][sel]) - RC.pairwise(a['x'][sel])).max())
            print(f'MEASURED rigid_kernel[{variant}, K={K}, f={f}] body {body} n {int((bid == body).sum())}: max|dx| {err:.2e}  '
                  f'pairwise {derr:.2e}  e32 {e32:.2e}  bound {bound:.2e}')
            assert err <= bound, (f, body, err, bound)
            assert derr <= bound, (f, body, derr, bound)
            assert np.abs(b['x'][sel] - a['x'][sel]).max() > 1e-5, (f, body)          # the body did move
        water = bid == 0
        plain, fused = a['x'][water] + np.float32(dt) * b['v'][water], _fused(a['x'][water], dt, b['v'][water])
        assert ((b['x'][water] == plain) | (b['x'][water] == fused)).all()             # not touched by the kernel
        unused = a['used'] == 0
        assert unused.sum() == (0 if variant != 'scattered' else 37 + 74)
        for k in 'xvCF':
            assert (b[k][unused] == a[k][unused]).all(), (f, k)
    eng.close()


def _check_rollout(tag, sc, final, grad, ref, yard, skip=None):
    """the bounds of (b): max|dx| on the rigid particles <= 2 d_x; every adjoint finite, cosine >= 0.999, rel L2 over all /
    over the rigid particles <= min(1e-2, 2 d_g) / min(1e-2, 2 d_grigid); rel L2 of gx per body <= 2 x the fp32 oracle's"""
    keep = np.ones(sc['N'], bool) if skip is None else ~skip
    d = RC.distances(sc, final, grad, ref, skip)
    print(f'MEASURED rigid_rollout[{tag}]: dx {d["d_x"]:.2e} (fp32 oracle {yard["d_x"]:.2e})  ' +
          '  '.join(f'{k} all {d["d_g"][k]:.2e} ({yard["d_g"][k]:.2e}) rigid {d["d_grigid"][k]:.2e} ({yard["d_grigid"][k]:.2e})' for k in RC.GRADS) +
          '  gx per body ' + ' '.join(f'{b}:{d["d_body"][b]:.1e} ({yard["d_body"][b]:.1e})' for b in d['d_body']))
    assert (final['used'] == ref['final']['used']).all()
    assert d['d_x'] <= 2 * yard['d_x'], ('dx', d['d_x'], yard['d_x'])
    for k in RC.GRADS:
        assert np.isfinite(grad[k]).all(), k
        assert S.cosine(grad[k][keep], ref['grad'][k][keep]) >= 0.999, (k, S.cosine(grad[k][keep], ref['grad'][k][keep]))
        assert d['d_g'][k] <= min(1e-2, 2 * yard['d_g'][k]), (k, 'all', d['d_g'][k], yard['d_g'][k])
        assert d['d_grigid'][k] <= min(1e-2, 2 * yard['d_grigid'][k]), (k, 'rigid', d['d_grigid'][k], yard['d_grigid'][k])
    for b in d['d_body']:
        assert d['d_body'][b] <= 2 * yard['d_body'][b], ('gx of body', b, d['d_body'][b], yard['d_body'][b])


@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave'])
@pytest.mark.parametrize('ranged', [False, True])
@pytest.mark.parametrize('K', [0, 1, 3])
def test_rollout_parity(hiplib, oracle32, oracle64, K, ranged, variant):
    sc = RC.scene(variant)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': K})
    final, grad = S.run_forward_backward(eng, RC.N_SUB, RC.cotangent(sc), ranged=ranged)
    eng.close()
    _check_rollout(f'{variant}, K={K}, ranged={int(ranged)}', sc, final, grad, RC.rollout(oracle64, variant), RC.yardstick(oracle32, oracle64, variant))


@pytest.mark.parametrize('ranged', [False, True])
def test_whole_unused_body(hiplib, oracle32, oracle64, ranged):
    """Body 3 has no used particle: its workgroup reduces nothing, runs svd3 / backward_svd on H = 0 and must write nothing.
    As on the oracle (test_whole_unused_body_on_the_oracle) its particles keep their state bit for bit in every frame and
    their frame-0 adjoint is the seeded cotangent, bit for bit; everything else meets the bounds of the rollout test.
    Engine.* raises on a non-zero return code, so coming through means every fe_* call returned 0."""
    sc = RC.scene('whole_body')
    body = sc['body_id'] == RC.UNUSED_BODY
    cot = RC.cotangent(sc)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': 3})
    final, grad = S.run_forward_backward(eng, RC.N_SUB, cot, ranged=ranged)
    first = S.get_state(eng, 0)
    for k, src in zip('xvCF', (sc['x'], sc['v'], sc['C'], sc['F'])):
        assert (first[k][body] == src[body]).all(), k
    for f in range(1, RC.N_SUB + 1):
        st = S.get_state(eng, f)
        assert (st['used'][body] == 0).all()
        for k in 'xvCF':
            assert (st[k][body] == first[k][body]).all(), (f, k)
    eng.sync()
    eng.close()
    for k in RC.GRADS:
        assert (grad[k][body] == cot[k][body]).all(), k
    _check_rollout(f'whole_body, K=3, ranged={int(ranged)}', sc, final, grad, RC.rollout(oracle64, 'whole_body'),
                   RC.yardstick(oracle32, oracle64, 'whole_body', skip=body), skip=body)


def _init(eng, sc):
    """what scenes.make_engine does after fe_create, on a handle that exists"""
    cls = np.array([S.MATERIALS[int(m)][3] for m in sc['mat']], np.int32)
    props = material_props(sc)
    eng.init_particles(sc['x'], sc['used'], sc['mat'], cls, props['mu'], props['lam'], props['rho'], sc['body_id'])
    eng.set_frame(0, v=sc['v'], C_=sc['C'], F=sc['F'])


@pytest.mark.parametrize('ranged', [False, True])
def test_reinitialised_handle(hiplib, oracle32, oracle64, ranged):
    """fe_init_particles on a handle that already holds bodies frees and rebuilds bodies_dev / body_start / body_pids.  A handle's
    particle count is fixed at fe_create, so the second scene is rigid_bodies_many with the same 2,150 rigid particles in three
    bodies (1213, 768, 169: 5, 3 and 1 passes) instead of eight; after it the handle meets the bounds a fresh engine meets."""
    first, sc = RC.scene('scattered'), RC.scene('three')
    assert first['N'] == sc['N']
    yard = RC.yardstick(oracle32, oracle64, 'three')
    eng = S.make_engine(hiplib, first, options={'sort_interval': 3})
    S.run_forward(eng, 2)
    _init(eng, sc)
    final, grad = S.run_forward_backward(eng, RC.N_SUB, RC.cotangent(sc), ranged=ranged)
    eng.close()
    _check_rollout(f'three, re-initialised, K=3, ranged={int(ranged)}', sc, final, grad, RC.rollout(oracle64, 'three'), yard)
    fresh = S.make_engine(hiplib, sc, options={'sort_interval': 3})
    final, grad = S.run_forward_backward(fresh, RC.N_SUB, RC.cotangent(sc), ranged=ranged)
    fresh.close()
    _check_rollout(f'three, fresh, K=3, ranged={int(ranged)}', sc, final, grad, RC.rollout(oracle64, 'three'), yard)
