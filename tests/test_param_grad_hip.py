"""Material-parameter gradients of the HIP engine (option param_grad, include/fluidengine_ext.h) against central finite differences of
the fp64 oracle (param_grad_common.py; test_param_grad_reference.py shows the differences are derivatives, to <= 3e-5).

Measure per direction: |engine - D| / max(|D|, 1e-3 * max |D| over the parameter's directions); no direction and no particle is left out.
Bounds: 4x the largest value measured on the MI355X per scene (run-to-run variation of the fp32 atomics upstream), never above the
1e-2 relative / 0.999 cosine class tests/test_hip_parity.py states for adjoints.
"""
import numpy as np
import pytest

import param_grad_common as P
import scenarios as S
from fluidlab_amd import _capi
from fluidlab_amd.optimizer import sysid

pytestmark = pytest.mark.gpu

# measured on the MI355X, worst direction over the twelve option sets: water 1.5e-3 ... 1.9e-3 (mu with random signs: |D| = 6e-9, 1/140 of the
# indicator's), mixed 1.1e-3 ... 1.95e-3 (lam of ICECREAM, the group with J - 1 ~ 1e-3 and |D| = 1/75 of the largest), latte 5.1e-6; every
# other direction is within 5e-4 (water) / 1.2e-4 (mixed)
TOL = {'water': 7.6e-3, 'mixed': 7.8e-3, 'latte': 2.1e-5}
assert all(t <= 1e-2 for t in TOL.values())


def _sweep(lib, sc, options, param_grad=True, n_sub=P.N_SUB, profile=False):
    """forward n_sub substeps as one call, the cotangent on the last frame, backward as one call"""
    eng = S.make_engine(lib, sc, options=options)
    if param_grad:
        eng.param_grad_enable()
    if profile:
        eng.profile_enable(True)
    cot = S.random_cotangent(sc['N'])
    eng.step(0, 0, n_sub, 0)
    eng.reset_grad()
    eng.add_grad(n_sub, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(0, 0, n_sub, 0)
    return eng


def _check(name, tag, sc, g, ref, random=True):
    got = P.engine_figures(sc, g, random=random)
    dev = P.deviation(got, ref)
    worst = max(dev, key=dev.get)
    print(f'MEASURED param_grad[{name}, {tag}]: worst {worst} {dev[worst]:.2e} | ' + ' '.join(f'{k[0]}/{k[1]} {got[k]:.4e} vs {ref[k]:.4e} ({dev[k]:.1e})' for k in sorted(ref)))
    for k in P.PARAMS:
        assert np.isfinite(g[k]).all(), k
        a, b = [got[key] for key in sorted(ref) if key[0] == k], [ref[key] for key in sorted(ref) if key[0] == k]
        assert S.cosine(a, b) >= 0.999, (k, S.cosine(a, b))
    assert dev[worst] <= TOL[name], (worst, dev[worst], got[worst], ref[worst])


@pytest.mark.parametrize('grid_store', [0, 1])
@pytest.mark.parametrize('fuse_bwd', [0, 1])
@pytest.mark.parametrize('K', [0, 3, 10])
@pytest.mark.parametrize('name', ['water', 'mixed'])
def test_parity_with_finite_differences_of_the_oracle(hiplib, oracle64, name, K, fuse_bwd, grid_store):
    """water: the liquid-only build with compact F (mu at mu = 0, lam, rho); mixed: all four constitutive branches, 10 % unused.
    K = 0 the global path, 3 sorts inside the fe_step_grad call, 10 the default; fused and unfused backward; with and without the grid store."""
    sc = P.scene(name)
    opts = {'sort_interval': K, 'fuse_bwd': fuse_bwd}
    if grid_store == 0:
        opts['grid_store'] = 0
    eng = _sweep(hiplib, sc, opts)
    g = eng.get_param_grad()
    assert eng.get_option('param_grad') == 1.0
    if name == 'water':
        assert eng.get_option('compact_F') == 1.0
    eng.close()
    unused = sc['used'] == 0
    for k in P.PARAMS:
        assert g[k].dtype == np.float64 and g[k].shape == (sc['N'],)
        assert (g[k][unused] == 0).all()                       # unused slots contribute nothing
    _check(name, f'K={K} fuse_bwd={fuse_bwd} grid_store={grid_store}', sc, g, P.reference(oracle64, name))


def test_injector_scene(hiplib, oracle64):
    """latte_mini: pool particles the Injector never took into use have exactly zero; a particle injected in substep f counts from f + 1 on
    (the per-material sums agree with the oracle's finite differences, MILK being the injected material)."""
    sc = P.scene('latte')
    eng, e = P.make_latte(hiplib, sc, None)
    eng.param_grad_enable()
    P.latte_forward(eng, e, sc)
    used_end = S.get_state(eng, sc['horizon'] * sc['n_substeps'])['used']
    P.latte_backward(eng, e, sc)
    g = eng.get_param_grad()
    eng.close()
    never = (sc['used'] == 0) & (used_end == 0)
    injected = (sc['used'] == 0) & (used_end != 0)
    assert never.sum() > 0 and injected.sum() > 0
    for k in P.PARAMS:
        assert (g[k][never] == 0).all(), k
    assert np.abs(g['rho'][injected]).max() > 0
    _check('latte', 'default options', sc, g, P.reference(oracle64, 'latte'), random=False)


def test_launch_accounting_and_untouched_state_adjoints(hiplib):
    """Option off: no param_grad launch in the profile of a fe_step + fe_step_grad pair; on: exactly one per backward substep.  The state
    adjoints are those of the run without it (to what two runs without it differ by, the bound of
    test_fused_p2g_grad_g2p_grad_launch_matches_separate_launches)."""
    sc = P.scene('water')
    runs = {}
    for tag, on in (('on', True), ('off', False), ('off2', False)):
        eng = _sweep(hiplib, sc, {}, param_grad=on, profile=True)
        runs[tag] = (dict(zip(('gx', 'gv', 'gC', 'gF'), eng.get_grad(0))), eng.profile_read())
        eng.close()
    assert 'param_grad' not in runs['off'][1], runs['off'][1]
    assert runs['on'][1]['param_grad'][1] == P.N_SUB, runs['on'][1]
    for k in runs['off'][1]:                                    # every other launch count is the same
        assert runs['on'][1][k][1] == runs['off'][1][k][1], k
    (got, _), (ref, _), (noise, _) = runs['on'], runs['off'], runs['off2']
    print('MEASURED param_grad on vs off, state adjoints:', {k: S.rel_l2(got[k], ref[k]) for k in got}, 'off vs off', {k: S.rel_l2(noise[k], ref[k]) for k in got})
    for k in got:
        assert S.rel_l2(got[k], ref[k]) <= 4.0 * S.rel_l2(noise[k], ref[k]) + 2e-5, k


def test_reset_and_accumulation(hiplib):
    """fe_reset_grad zeroes the accumulators; two backward passes without a reset add up to twice the values."""
    sc = P.scene('water')
    n_sub = 5                                                  # (frames 5 and 1 share a slot of the adjoint ring: see below)
    cot = S.random_cotangent(sc['N'])
    eng = S.make_engine(hiplib, sc, options={'fuse_bwd': 0})
    eng.param_grad_enable()
    eng.step(0, 0, n_sub, 0)

    def backward():
        eng.add_grad(n_sub, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        for f in reversed(range(n_sub)):
            eng.substep_grad(f, f, 0)

    eng.reset_grad()
    backward()
    g1 = eng.get_param_grad()
    assert all(np.abs(g1[k]).max() > 0 for k in P.PARAMS)
    # the same seed again: the ring slot frame n_sub's adjoint goes into holds frame 1's now -- cancelled exactly (x + (-x) = 0), not reset
    eng.add_grad(1, *[-a for a in eng.get_grad(1)])
    assert all((a == 0).all() for a in eng.get_grad(1))
    backward()
    g2 = eng.get_param_grad()
    for k in P.PARAMS:
        err = np.abs(g2[k] - 2.0 * g1[k]).max() / np.abs(g1[k]).max()
        print(f'MEASURED param_grad accumulation[{k}]: |second - 2 first| / |first|max = {err:.2e}')
        assert err <= 1e-12, (k, err)
    eng.reset_param_grad()
    assert all((v == 0).all() for v in eng.get_param_grad().values())
    backward()
    assert all(np.abs(v).max() > 0 for v in eng.get_param_grad().values())
    eng.reset_grad()
    assert all((v == 0).all() for v in eng.get_param_grad().values())
    eng.close()


def test_rigid_scenes_and_batched_backward_are_refused(hiplib):
    eng = S.make_engine(hiplib, S.rigid_in_water())
    with pytest.raises(_capi.FeEngineError, match='MAT_RIGID'):
        eng.param_grad_enable()
    assert eng.get_option('param_grad') == 0.0
    eng.close()
    with pytest.raises(_capi.FeEngineError, match='MAT_RIGID'):           # ... also when the option comes first
        S.make_engine(hiplib, S.rigid_in_water(), options={'param_grad': 1})
    sc = S.water_block(n_grid=16, n_particles=500)
    engs = [S.make_engine(hiplib, sc) for _ in range(2)]
    engs[1].param_grad_enable()
    _capi.Engine.step_batch(engs, 0, 0, 2, 0)
    for e in engs:
        e.reset_grad()
    with pytest.raises(_capi.FeEngineError, match='param_grad'):
        _capi.Engine.step_grad_batch(engs, 0, 0, 2, 0)
    engs[1].param_grad_enable(False)
    _capi.Engine.step_grad_batch(engs, 0, 0, 2, 0)                         # (off again: the batch runs)
    for e in engs:
        e.close()


def test_twin_experiment_recovers_the_shear_modulus(hiplib):
    """optimizer/sysid.py: a 6-substep target recorded with mixed_materials(), a restart with the ELASTIC group's mu scaled by 0.7, ten Adam
    iterations on that scale: the loss falls and the scale moves towards 1 (conditions, no rate)."""
    sc = S.mixed_materials()
    target = sysid.record_target(hiplib, sc, 1, 6)
    scales, hist = sysid.fit(hiplib, sc, target, 6, groups=[S.ELASTIC], scales0={'mu': [0.7]}, n_iters=10, fit_params=('mu',))
    last_loss, _ = sysid.loss_and_grad(hiplib, sc, _scaled(sc, scales['mu'][0]), target, 6)
    print('MEASURED param_grad twin experiment: loss', [float(f'{h[0]:.4g}') for h in hist], '->', float(f'{last_loss:.4g}'), 'scale', [round(float(h[1]['mu'][0]), 4) for h in hist], '->', round(float(scales['mu'][0]), 4))
    assert hist[0][1]['mu'][0] == 0.7 and hist[0][0] > 0
    assert last_loss < hist[0][0]
    assert abs(scales['mu'][0] - 1.0) < abs(0.7 - 1.0) and scales['mu'][0] > 0.7


def _scaled(sc, s):
    props = sysid.material_props(sc)
    props['mu'][sc['mat'] == S.ELASTIC] *= s
    return props
