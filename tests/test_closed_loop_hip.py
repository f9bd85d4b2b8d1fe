"""The closed-loop entries on the MI355X (include/fluidengine_ext.h, fe_policy_io.h): observation adjoint scatter, effector state adjoint,
device forms of the action crossings, and ClosedLoopSolver on the device road against the dense road and the fp64 oracle.

Raw-ABI cases run S.stirrer_mini (16^3, 1,500 particles, 4 x 4 substeps) with sort_interval = 3: the particle order changes at frames
3, 6, 9, 12, 15, so frames -- and the adjoint slots that follow them across a sort -- are stored in different orders.  Comparisons are
made within one engine: two rollouts of this engine do not end in the same bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import scenarios as S
from fluidlab_amd import _capi

pytestmark = pytest.mark.gpu

OPTS = {'sort_interval': 3}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _stirrer(hiplib, with_tool=True, move_water=False):
    sc = S.stirrer_mini()
    if move_water:                                               # the water in a far corner: nothing touches the tool, its pose chain is all there is
        rng = np.random.RandomState(4)
        sc['x'] = S.f32(rng.uniform([0.75, 0.12, 0.72], [0.9, 0.3, 0.9], (sc['N'], 3)))
    eng = S.make_engine(hiplib, sc, options=OPTS)
    e = None
    if with_tool:
        r = sc['rigid']
        e = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=r['action_dim'], action_scale_v=r['action_scale_v'], action_scale_p=r['action_scale_p'],
                             boundary=hiplib.make_boundary(**r['boundary']))
        eng.eff_set_mesh(e, r['voxels'], r['T'], friction=r['friction'], softness=r['softness'])
        st0 = eng.eff_get_state(e, 0)
        st0[:7] = r['init_state']
        eng.eff_set_state(e, 0, st0)
    return sc, eng, e


def _forward(sc, eng, e, actions=None, steps=None):
    ns = sc['n_substeps']
    actions = sc['actions'] if actions is None else actions
    for s in range(sc['horizon'] if steps is None else steps):
        eng.eff_set_action(e, s, s, ns, actions[s])
        eng.step(s * ns, s * ns, ns, 1)


def _obs_list(N, seed=9):
    """97 ids: 92 distinct, three of them once more, a fourth two more times, shuffled"""
    rng = np.random.RandomState(seed)
    base = rng.choice(N, 92, replace=False)
    ids = np.concatenate([base, base[[5, 17, 40]], base[[63, 63]]])
    rng.shuffle(ids)
    assert len(ids) == 97 and len(np.unique(ids)) == 92 and np.bincount(ids).max() == 3 and (np.bincount(ids) == 2).sum() == 3
    return ids.astype(np.int32)


def _rows(n, seed):
    rng = np.random.RandomState(seed)
    mk = lambda: (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 3))).astype(np.float32)
    return mk(), mk()


def _dense(N, ids, rows):
    d = np.zeros((N, 3), np.float32)
    np.add.at(d, ids, rows)                                      # (list order, fp32)
    return d


def _check_injection(eng, f, ids, gx, gv, dev, what):
    """G1 = G0 + dense bit for bit in gx and gv on the listed particles, nothing else changes; returns G1's (gx, gv)"""
    import torch
    N = eng.N
    G0 = eng.get_grad(f)
    if dev:
        d = torch.device('cuda', eng.device)
        eng.obs_add_grad_dev(f, torch.as_tensor(gx, device=d), torch.as_tensor(gv, device=d))
    else:
        eng.obs_add_grad(f, gx, gv)
    G1 = eng.get_grad(f)
    listed = np.zeros(N, bool); listed[ids] = True
    for k, rows in ((0, gx), (1, gv)):
        want = np.where(listed[:, None], G0[k] + _dense(N, ids, rows), G0[k])       # (one fp32 addition of the fp32 list-order sum)
        bad = int((_bits(G1[k]) != _bits(want)).sum())
        assert bad == 0, f'{what}: {bad} words of {"gx gv".split()[k]} differ from G0 + dense'
    assert (_bits(G1[2]) == _bits(G0[2])).all() and (_bits(G1[3]) == _bits(G0[3])).all(), f'{what}: gC / gF changed'
    return G1[0], G1[1]


@pytest.fixture(scope='module')
def rolled(hiplib):
    """one engine, rolled forward over the horizon with the scene's actions, with the 97-row observation list"""
    sc, eng, e = _stirrer(hiplib)
    _forward(sc, eng, e)
    ids = _obs_list(sc['N'])
    eng.obs_set_particles(ids)
    yield sc, eng, e, ids
    eng.close()


def test_obs_add_grad_cleared_slot_on_the_last_frame(rolled):
    sc, eng, e, ids = rolled
    f = sc['horizon'] * sc['n_substeps']
    gx, gv = _rows(len(ids), 1)
    out = []
    for dev in (False, True):
        eng.reset_grad()
        out.append(_check_injection(eng, f, ids, gx, gv, dev, f'cleared slot, dev={dev}'))
    assert (_bits(out[0][0]) == _bits(out[1][0])).all() and (_bits(out[0][1]) == _bits(out[1][1])).all()      # host and _dev: the same bits
    assert np.abs(out[0][0]).max() > 0
    # either array alone
    eng.reset_grad()
    eng.obs_add_grad(f, gx=gx)
    G = eng.get_grad(f)
    assert (_bits(G[0]) == _bits(out[0][0])).all() and not G[1].any()
    eng.reset_grad()


def test_obs_add_grad_occupied_slots_across_sorts(rolled):
    sc, eng, e, ids = rolled
    H, ns, N = sc['horizon'], sc['n_substeps'], sc['N']
    cot = S.random_cotangent(N)
    eng.reset_grad()
    eng.add_grad(H * ns, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad((H - 1) * ns, (H - 1) * ns, ns, 1)             # one step back: only frame f0 = 12's adjoint is defined, in the order the sweep left it in
    f0 = (H - 1) * ns
    assert np.abs(eng.get_grad(f0)[0]).max() > 0
    for k, dev in enumerate((False, True)):
        gx, gv = _rows(len(ids), 10 + k)
        _check_injection(eng, f0, ids, gx, gv, dev, f'occupied slot on f0, dev={dev}')
    # substep by substep down to frame 8: every position relative to the sorts at 9 and 12, the frames directly behind them included
    for f in range(f0 - 1, f0 - 5, -1):
        eng.substep_grad(f, f, 1)
        gx, gv = _rows(len(ids), 20 + f)
        _check_injection(eng, f, ids, gx, gv, f % 2 == 0, f'occupied slot on frame {f}')
    eng.reset_grad()


def test_refusals_leave_the_adjoint_unchanged(hiplib, rolled):
    sc, eng, e, ids = rolled
    H, ns, N = sc['horizon'], sc['n_substeps'], sc['N']
    gx, gv = _rows(len(ids), 3)
    f = H * ns
    eng.reset_grad()
    eng.obs_add_grad(f, gx, gv)
    G0 = eng.get_grad(f)
    # f out of range
    with pytest.raises(_capi.FeEngineError, match='frame index out of range'):
        eng.obs_add_grad(sc['max_substeps_local'] + 1, gx, gv)
    assert b'out of range' in eng.lib.fe_last_error(eng.h)
    with pytest.raises(_capi.FeEngineError, match='frame index out of range'):
        eng.obs_add_grad(-1, gx, gv)
    # no list
    eng.obs_set_particles(None)
    with pytest.raises(_capi.FeEngineError, match='no observation list'):
        eng.obs_add_grad(f, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    assert b'no observation list' in eng.lib.fe_last_error(eng.h)
    G1 = eng.get_grad(f)
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(G0, G1))
    eng.obs_set_particles(ids)
    eng.reset_grad()
    # a frame inside a fused fe_step_grad call: the water alone (a tool colliding at the particles keeps the backward substeps apart)
    sc2, eng2, _ = _stirrer(hiplib, with_tool=False)
    eng2.set_option('fuse_bwd', 1)
    eng2.obs_set_particles(ids)
    cot = S.random_cotangent(N)
    eng2.step(0, 0, 6, 0)
    eng2.reset_grad()
    eng2.add_grad(6, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng2.step_grad(3, 3, 3, 0)                                   # frames 5, 4, 3 share the order of the sort at 3: frame 4's x, v, C adjoint never reached memory
    G0 = eng2.get_grad(3)
    with pytest.raises(_capi.FeEngineError, match='registers'):
        eng2.obs_add_grad(4, gx, gv)
    assert b'registers' in eng2.lib.fe_last_error(eng2.h)
    import torch
    with pytest.raises(_capi.FeEngineError, match='registers'):
        eng2.obs_add_grad_dev(4, torch.as_tensor(gx, device=f'cuda:{eng2.device}'), None)
    G1 = eng2.get_grad(3)
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(G0, G1))
    _check_injection(eng2, 3, ids, gx, gv, False, 'the call\'s first frame')      # defined, and taken
    eng2.close()


def test_effector_state_grad_add_and_get(rolled):
    import torch
    sc, eng, e, ids = rolled
    H, ns, N = sc['horizon'], sc['n_substeps'], sc['N']
    cot = S.random_cotangent(N)
    eng.reset_grad()
    assert not eng.eff_get_state_grad(e, H * ns).any()
    eng.add_grad(H * ns, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad((H - 1) * ns, (H - 1) * ns, ns, 1)             # contact puts something into the pose adjoints of frames 12 ..
    f = (H - 1) * ns + 1
    g0 = eng.eff_get_state_grad(e, f)
    assert g0.dtype == np.float32 and g0.shape == (7,) and np.abs(g0).max() > 0
    g7 = (np.random.RandomState(2).normal(size=7) * np.abs(g0).max()).astype(np.float32)
    eng.eff_add_state_grad(e, f, g7)
    g1 = eng.eff_get_state_grad(e, f)
    assert (_bits(g1) == _bits(g0 + g7)).all()
    eng.eff_add_state_grad_dev(e, f, torch.as_tensor(g7, device=f'cuda:{eng.device}'))
    g2 = eng.eff_get_state_grad(e, f)
    assert (_bits(g2) == _bits(g1 + g7)).all()
    for bad_e, bad_f in ((e + 1, f), (e, -1), (e, sc['max_substeps_local'] + 1)):
        with pytest.raises(_capi.FeEngineError, match='out of range'):
            eng.eff_add_state_grad(bad_e, bad_f, g7)
    assert (_bits(eng.eff_get_state_grad(e, f)) == _bits(g2)).all()
    # the pose, device form
    s7 = torch.empty((7,), dtype=torch.float32, device=f'cuda:{eng.device}')
    eng.eff_get_state_dev(e, f, s7)
    assert (_bits(s7.cpu().numpy()) == _bits(eng.eff_get_state(e, f)[:7])).all()
    eng.reset_grad()


def test_effector_state_grad_end_to_end(hiplib):
    """<c, (pos, quat)[2 n_substeps]> with the water away from the tool: the action gradient of steps 0 and 1 against difference quotients"""
    sc, eng, e = _stirrer(hiplib, move_water=True)
    ns, ad = sc['n_substeps'], sc['rigid']['action_dim']
    f_end = 2 * ns
    c7 = np.array([1.0, -1.25, 0.75, 0.9, -0.5, 1.1, 0.6], np.float32)

    def value(actions):
        st0 = eng.eff_get_state(e, 0)
        st0[:7] = sc['rigid']['init_state']
        eng.eff_set_state(e, 0, st0)
        _forward(sc, eng, e, actions=actions, steps=2)
        return float(eng.eff_get_state(e, f_end)[:7].astype(np.float64) @ c7.astype(np.float64))

    base = sc['actions'].astype(np.float32).copy()
    v0 = value(base)
    eng.reset_grad()
    eng.eff_add_state_grad(e, f_end, c7)
    for s in (1, 0):
        eng.step_grad(s * ns, s * ns, ns, 1)
        eng.eff_set_action_grad(e, s, s, ns)
    grad = eng.eff_get_action_grad(e, 0, sc['horizon'], ad)[:sc['horizon']]
    assert not grad[2:].any()                                    # later steps: exactly 0
    for s in (0, 1):
        for k in range(3):                                       # translation: pos is linear in the action, the bound is fp32 rounding
            a = base.copy(); a[s, k] += np.float32(0.1)
            h = float(a[s, k]) - float(base[s, k])
            fd = (value(a) - v0) / h
            print(f'step {s} translation {k}: adjoint {grad[s, k]!r} forward difference {fd!r}')
            assert abs(grad[s, k] - fd) <= 1e-5 * abs(fd), (s, k, grad[s, k], fd)
        for k in range(3, 6):                                    # rotation: the finite difference's own truncation is the yardstick
            def central(h):
                ap = base.copy(); am = base.copy()
                ap[s, k] += np.float32(h); am[s, k] -= np.float32(h)
                return (value(ap) - value(am)) / (float(ap[s, k]) - float(am[s, k]))
            f1, f2 = central(0.1), central(0.05)
            tol = 10 * abs(f1 - f2) + 1e-5 * abs(f2)             # (floor: fp32 rounding of the pose words over the step, as for the translations)
            print(f'step {s} rotation {k}: adjoint {grad[s, k]!r} FD_h {f1!r} FD_h/2 {f2!r} tolerance {tol!r}')
            assert abs(grad[s, k] - f2) <= tol, (s, k, grad[s, k], f1, f2, tol)
    assert np.abs(grad[:2, 3:]).max() > 0
    eng.close()


def test_action_crossings_give_the_bits_of_the_host_variants(rolled):
    import torch
    sc, eng, e, ids = rolled
    H, ns, N, ad = sc['horizon'], sc['n_substeps'], sc['N'], sc['rigid']['action_dim']
    dev = torch.device('cuda', eng.device)
    a = np.array([0.013, -0.007, 0.019, 0.21, -0.33, 0.08], np.float32)
    eng.eff_set_action(e, 1, 1, ns, a)
    host = [eng.eff_get_vw(e, f) for f in range(ns, 2 * ns)]
    eng.eff_set_action_dev(e, 2, 2, ns, torch.as_tensor(a, device=dev))
    devv = [eng.eff_get_vw(e, f) for f in range(2 * ns, 3 * ns)]
    for (v0, w0), (v1, w1) in zip(host, devv):
        assert (_bits(v0) == _bits(v1)).all() and (_bits(w0) == _bits(w1)).all()
        assert (_bits(v0) == _bits(a[:3] / np.float32(ns))).all()
    with pytest.raises(_capi.FeEngineError, match='must be a contiguous'):
        eng.eff_set_action_dev(e, 2, 2, ns, torch.zeros(3, device=dev))
    with pytest.raises(_capi.FeEngineError, match='out of range'):
        eng.eff_set_action_dev(e, 2, H, ns, torch.as_tensor(a, device=dev))
    # the action gradient after a sweep
    _forward(sc, eng, e)                                         # (the scene's own actions again)
    cot = S.random_cotangent(N)
    eng.reset_grad()
    eng.add_grad(H * ns, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    for s in reversed(range(H)):
        eng.step_grad(s * ns, s * ns, ns, 1)
        eng.eff_set_action_grad(e, s, s, ns)
    want = eng.eff_get_action_grad(e, 0, H, ad)[:H]
    assert np.abs(want).max() > 0
    out = torch.zeros((H, ad), dtype=torch.float32, device=dev)
    eng.eff_get_action_grad_dev(e, 0, H, out)
    assert (_bits(out.cpu().numpy()) == _bits(want)).all()
    one = torch.zeros((1, ad), dtype=torch.float32, device=dev)
    eng.eff_get_action_grad_dev(e, 2, 1, one)
    assert (_bits(one.cpu().numpy()[0]) == _bits(want[2])).all()
    eng.reset_grad()


# ---- the whole loop ------------------------------------------------------------------------------------------------------------
HL = 4


def _loop(lib, use_agent_state, device_obs):
    from fluidlab_amd.envs import make
    from fluidlab_amd.optimizer.closed_loop import ClosedLoopSolver, ObsPolicy
    env = make('Mixing-v0', seed=0, loss=True, engine_lib=lib, quality=0.5, particle_density=3e4, horizon=HL, max_substeps_local=None, ckpt_dest='cpu')
    env.taichi_env.loss.temporal_range[1] = HL
    if device_obs:
        env.enable_device_obs()
    pol = ObsPolicy(env, hidden=16, use_agent_state=use_agent_state, input_gain=30.0, seed=1)
    sol = ClosedLoopSolver(env, pol)
    assert sol._device_road() == bool(device_obs)
    info = sol.forward_backward(env.taichi_env.get_state()['state'])
    g = sol.grad_vector()
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    return g, info['loss']


def test_closed_loop_device_road_against_dense_road(hiplib):
    """device road within 4 x the dense road's own run-to-run spread of the parameter gradient (relative L2), use_agent_state=True"""
    d1, l1 = _loop(hiplib, True, False)
    d2, l2 = _loop(hiplib, True, False)
    dv, lv = _loop(hiplib, True, True)
    spread = S.rel_l2(d2, d1)
    rel = S.rel_l2(dv, d1)
    print(f'closed loop on HIP, use_agent_state=True: dense road run to run {spread!r}, device road against dense road {rel!r}; losses {l1!r} {l2!r} {lv!r}')
    assert rel <= 4 * spread, (rel, spread)


def test_closed_loop_hip_against_the_fp64_oracle(hiplib, oracle32, oracle64):
    """HIP (device road) within 4 x what the fp32 oracle shows against the fp64 oracle on the same scene, use_agent_state=False"""
    g64, l64 = _loop(oracle64, False, False)
    g32, l32 = _loop(oracle32, False, False)
    gh, lh = _loop(hiplib, False, True)
    yard = S.rel_l2(g32, g64)
    rel = S.rel_l2(gh, g64)
    print(f'closed loop, use_agent_state=False: fp32 oracle against fp64 oracle {yard!r}, HIP against fp64 oracle {rel!r}; losses {l64!r} {l32!r} {lh!r}')
    assert rel <= 4 * yard, (rel, yard)
