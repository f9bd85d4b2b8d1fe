"""GPU: the observation gather (fe_obs_*) and the frame summary (fe_frame_summary) of the HIP engine through the C ABI, against numpy in
fp64 on what fe_get_frame returns for the same frame.  fe_get_frame is always called AFTER the summary: handing F out expands a compactly
stored F, which the summary must read as it is.

Tolerances: counts and extremes (v_max, bounding box) are exact -- they are comparisons of widened fp32 words.  Sums are compared within
1e-11 x sum |terms|: the engine adds the same fp64 terms in another order, which for n = 1,500 terms is bounded by (n - 1) 2^-53 ~ 2e-13 of
sum |terms|.  det F within 1e-12 x the sum of its six |triple products| (five fp64 roundings, ~6e-16)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

pytestmark = pytest.mark.gpu
SUM_TOL, DET_TOL = 1e-11, 1e-12


def _det(F):
    F = F.astype(np.float64).reshape(-1, 9)
    f = [F[:, i] for i in range(9)]
    J = f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6])
    Jabs = sum(np.abs(f[a] * f[b] * f[c]) for a, b, c in ((0, 4, 8), (0, 5, 7), (1, 3, 8), (1, 5, 6), (2, 3, 7), (2, 4, 6)))
    return J, Jabs


def _mass(sc):
    """what fe_init_particles stores: fp32 p_vol times fp32 rho, rounded to fp32"""
    from fluidlab_amd.scenes import material_props
    rho = material_props(sc)['rho']
    return (np.float32((0.5 / sc['n_grid']) ** 2) * rho.astype(np.float32)).astype(np.float32)


def _check_record(rec, st, mass, member, dt, dx, tag):
    """rec: one dict of Engine.frame_summary; st: the downloaded frame; member: bool [N], the particles of the group"""
    with np.errstate(invalid='ignore'):
        finite = np.isfinite(st['x']).all(1) & np.isfinite(st['v']).all(1) & np.isfinite(st['C']).all((1, 2)) & np.isfinite(st['F']).all((1, 2))
    sel = member & (st['used'] != 0)
    ok = sel & finite
    assert rec['n_used'] == int(sel.sum()), tag
    assert rec['n_nonfinite'] == int((sel & ~finite).sum()), tag
    vec = ('com', 'momentum', 'lo', 'hi')
    if not ok.any():
        for k, val in rec.items():
            if k not in ('n_used', 'n_nonfinite'):
                assert np.all(np.asarray(val) == 0.0), (tag, k)
        return
    m = mass[ok].astype(np.float64)
    x, v = st['x'][ok].astype(np.float64), st['v'][ok].astype(np.float64)
    for k in vec + ('mass', 'kinetic', 'v_max', 'courant', 'J_min', 'J_max'):
        assert np.all(np.isfinite(rec[k])), (tag, k)
    # exact: comparisons of widened fp32 words
    assert rec['v_max'] == np.abs(v).max(), tag
    assert np.array_equal(rec['lo'], x.min(0)) and np.array_equal(rec['hi'], x.max(0)), tag
    want_c = dt * np.abs(v).max() / dx
    print(f'{tag}: courant {rec["courant"]!r} numpy {want_c!r}')
    assert abs(rec['courant'] - want_c) <= np.spacing(want_c), tag          # at most one rounding apart
    # sums
    def close(name, got, terms):
        want, bound = terms.sum(0), SUM_TOL * np.abs(terms).sum(0)
        print(f'{tag}: {name} err {np.max(np.abs(got - want))!r} bound {np.min(bound)!r}')
        assert np.all(np.abs(got - want) <= bound), (tag, name, got, want)
    close('mass', rec['mass'], m)
    close('com * mass', rec['com'] * rec['mass'], m[:, None] * x)
    close('momentum', rec['momentum'], m[:, None] * v)
    close('kinetic', rec['kinetic'], 0.5 * m * (v * v).sum(1))
    J, Jabs = _det(st['F'][ok])
    print(f'{tag}: J_min err {abs(rec["J_min"] - J.min())!r} J_max err {abs(rec["J_max"] - J.max())!r} bound {DET_TOL * Jabs.min()!r}')
    assert abs(rec['J_min'] - J.min()) <= DET_TOL * Jabs[np.argmin(J)], tag
    assert abs(rec['J_max'] - J.max()) <= DET_TOL * Jabs[np.argmax(J)], tag


def _dt_dx(sc):
    return float(np.float32(sc['dt'])), float(np.float32(1.0) / np.float32(sc['n_grid']))


def _rows_equal(got, st, ids):
    for k in ('x', 'v', 'used'):
        assert got[k].dtype == st[k].dtype and got[k].shape == st[k][ids].shape, k
        assert np.array_equal(got[k].view(np.uint32), st[k][ids].view(np.uint32)), k


def _gather_both_ways(eng, f, ids):
    """host and device variant of the gather at frame f, then the frame itself"""
    import torch
    n = len(ids)
    host = eng.get_obs(f)
    dev = torch.device('cuda', eng.device)
    tx, tv = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev), torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    tu = torch.full((n,), -7, dtype=torch.int32, device=dev)
    eng.get_obs_dev(f, tx, tv, tu)
    st = S.get_state(eng, f)
    _rows_equal(host, st, ids)
    _rows_equal({'x': tx.cpu().numpy(), 'v': tv.cpu().numpy(), 'used': tu.cpu().numpy()}, st, ids)


def test_gather_identity_order(hiplib):
    sc = S.water_block(n_grid=16, n_particles=1500)
    sc['v'] = S.f32(np.random.RandomState(3).normal(0, 0.5, (1500, 3)))
    eng = S.make_engine(hiplib, sc)
    with pytest.raises(Exception, match='no observation list'):
        eng.get_obs(0)
    rng = np.random.RandomState(0)
    ids = np.concatenate([[0, 1499, 7, 7, 1499], rng.randint(0, 1500, 195)]).astype(np.int32)
    assert len(ids) == 200 and len(np.unique(ids)) < 200
    for lst in (ids, np.array([733], np.int32), rng.permutation(1500).astype(np.int32)):
        eng.obs_set_particles(lst)
        _gather_both_ways(eng, 0, lst)
    with pytest.raises(Exception, match='out of range'):
        eng.obs_set_particles([0, 1500])
    _gather_both_ways(eng, 0, lst)                            # a refused list leaves the old one in place
    import torch
    with pytest.raises(Exception, match='get_obs_dev: x must be'):   # a tensor that does not fit the list never reaches the kernel
        eng.get_obs_dev(0, x=torch.zeros((len(lst) - 1, 3), dtype=torch.float32, device=torch.device('cuda', eng.device)))
    eng.obs_set_particles(None)
    with pytest.raises(Exception, match='no observation list'):
        eng.get_obs(0)
    eng.close()


def test_gather_across_sorts(hiplib):
    sc = S.water_block(n_grid=16, n_particles=1500)
    eng = S.make_engine(hiplib, sc, max_substeps_local=32)
    assert eng.get_option('sort_interval') == 10
    ids = np.concatenate([[0, 1499, 5, 5], np.random.RandomState(1).randint(0, 1500, 196)]).astype(np.int32)
    eng.obs_set_particles(ids)
    eng.step(0, 0, 25, 0)
    for f in (0, 9, 10, 25):
        _gather_both_ways(eng, f, ids)
    x25 = eng.get_obs(25)['x']
    assert not np.array_equal(x25, eng.get_obs(0)['x'])
    eng.copy_frame(25, 0)
    _gather_both_ways(eng, 0, ids)
    assert np.array_equal(eng.get_obs(0)['x'], x25)
    eng.close()


def test_summary_general_materials(hiplib):
    sc = S.mixed_materials(n_grid=16, n_particles=1500)
    eng = S.make_engine(hiplib, sc)
    pid = np.arange(1500)
    group = (pid % 3).astype(np.int32)
    group[::7] = -1
    eng.summary_set_groups(group, 4)                          # group 3 has no particle
    eng.step(0, 0, 12, 0)
    recs = eng.frame_summary(12)
    st = S.get_state(eng, 12)
    assert len(recs) == 5
    dt, dx = _dt_dx(sc)
    mass = _mass(sc)
    for g in range(4):
        _check_record(recs[g], st, mass, group == g, dt, dx, f'general group {g}')
    _check_record(recs[4], st, mass, np.ones(1500, bool), dt, dx, 'general frame')
    assert recs[3]['n_used'] == 0 and recs[4]['n_used'] == int(st['used'].sum()) and recs[4]['n_used'] > sum(r['n_used'] for r in recs[:4])
    assert recs[4]['J_min'] < recs[4]['J_max'] and recs[4]['kinetic'] > 0
    with pytest.raises(Exception, match='out of range'):
        eng.summary_set_groups(np.full(1500, 4, np.int32), 4)
    eng.summary_set_groups(None)
    only = eng.frame_summary(12)
    assert len(only) == 1 and only[0]['n_used'] == recs[4]['n_used'] and only[0]['v_max'] == recs[4]['v_max']
    eng.close()


def test_summary_compact_liquid_frames(hiplib):
    sc = S.water_block(n_grid=16, n_particles=1500)
    eng, plain = S.make_engine(hiplib, sc), S.make_engine(hiplib, sc)
    assert eng.get_option('compact_F') == 1
    group = (np.arange(1500) % 2).astype(np.int32)
    eng.summary_set_groups(group, 2)
    for e in (eng, plain):
        e.profile_enable(True)
        e.step(0, 0, 5, 0)

    def xvC(e):                                               # (no F: this download does not expand it)
        x, v, C_, u = np.zeros((1500, 3), np.float32), np.zeros((1500, 3), np.float32), np.zeros((1500, 3, 3), np.float32), np.zeros(1500, np.int32)
        e.get_frame(5, x, v, C_, None, u)
        return x, v, C_, u

    before = xvC(eng)
    a = eng.frame_summary(5)
    b = eng.frame_summary(5)
    for p, q in zip(before, xvC(eng)):                        # the frame was only read
        assert np.array_equal(p.view(np.uint32), q.view(np.uint32))
    for e in (eng, plain):
        e.step(5, 5, 5, 0)
    # ... and the rollout goes on with the launches of one without summaries (whose kernels are not in the profile)
    launches = [{k: n for k, (ms, n) in e.profile_read().items()} for e in (eng, plain)]
    assert launches[0] == launches[1] and sum(launches[0].values()) > 0, launches
    st = S.get_state(eng, 5)                                  # (after the summaries: this expands frame 5's F)
    dt, dx = _dt_dx(sc)
    mass = _mass(sc)
    for g in range(2):
        _check_record(a[g], st, mass, group == g, dt, dx, f'liquid group {g}')
    _check_record(a[2], st, mass, np.ones(1500, bool), dt, dx, 'liquid frame')
    F = st['F'].astype(np.float64)
    assert np.all(F[:, 0, 0] == F[:, 2, 2]) and np.all(F[:, 0, 1] == 0)       # F = c I: what the compact store held
    for ra, rb in zip(a, b):
        for k in ('n_used', 'n_nonfinite', 'v_max', 'courant', 'J_min', 'J_max'):
            assert ra[k] == rb[k], k
        assert np.array_equal(ra['lo'], rb['lo']) and np.array_equal(ra['hi'], rb['hi'])
        for k in ('mass', 'kinetic', 'momentum', 'com'):
            assert np.all(np.abs(ra[k] - rb[k]) <= SUM_TOL * np.abs(ra[k])), k       # (|sum| <= sum |terms|: no looser than the bound above)
    c = eng.frame_summary(5)                                  # and the expanded frame gives what the compact one gave
    assert c[2]['J_min'] == a[2]['J_min'] and c[2]['J_max'] == a[2]['J_max'] and c[2]['n_used'] == a[2]['n_used']
    eng.close(); plain.close()


def test_summary_skips_unused_particles(hiplib):
    sc = S.latte_mini()
    inj = sc['injector']
    eng = S.make_engine(hiplib, sc)
    e = eng.add_effector(type=S.FE_EFF_INJECTOR, action_dim=inj['action_dim'], action_scale_v=inj['action_scale_v'],
                         action_scale_p=inj['action_scale_p'], boundary=hiplib.make_boundary(**inj['boundary']),
                         flux=inj['flux'], radius=inj['radius'], inject_v=inj['inject_v'], inject_p=inj['inject_p'],
                         locally_random=inj['locally_random'], random_vector=inj['random_vector'])
    eng.eff_set_act_range(e, np.where(sc['used'] == 0)[0].astype(np.int32))
    st0 = eng.eff_get_state(e, 0)
    st0[:7] = [0.5, 0.5, 0.5, 1.0, 0.0, 0.0, 0.0]
    eng.eff_set_state(e, 0, st0)
    eng.eff_apply_action_p(e, sc['action_p'])
    ns = sc['n_substeps']
    eng.eff_set_action(e, 0, 0, ns, sc['actions'][0])
    eng.step(0, 0, ns, 1)
    rec = eng.frame_summary(ns)
    st = S.get_state(eng, ns)
    assert len(rec) == 1
    n_coffee = int(sc['used'].sum())
    assert rec[0]['n_used'] == int(st['used'].sum()) and n_coffee < rec[0]['n_used'] < sc['N']       # some of the pool is in use, most of it still parked
    assert rec[0]['lo'].min() > 0.0 and rec[0]['hi'].max() < 1.0
    dt, dx = _dt_dx(sc)
    _check_record(rec[0], st, _mass(sc), np.ones(sc['N'], bool), dt, dx, 'injector frame')
    eng.close()


def test_summary_counts_non_finite_particles(hiplib):
    """frame 0 is written with fe_set_frame and only summarised: an engine holding a non-finite value is never stepped"""
    sc = S.water_block(n_grid=16, n_particles=1500)
    eng = S.make_engine(hiplib, sc)
    group = (np.arange(1500) % 3).astype(np.int32)
    eng.summary_set_groups(group, 3)
    rng = np.random.RandomState(4)
    x, v, C = sc['x'].copy(), S.f32(rng.normal(0, 0.5, (1500, 3))), S.f32(rng.normal(0, 1.0, (1500, 3, 3)))
    x[10, 1] = np.nan          # group 1
    v[20, 0] = np.inf          # group 2
    C[31, 2, 1] = np.nan       # group 1
    eng.set_frame(0, x=x, v=v, C_=C)
    recs = eng.frame_summary(0)
    st = S.get_state(eng, 0)
    assert [r['n_nonfinite'] for r in recs] == [0, 2, 1, 3]
    assert [r['n_used'] for r in recs] == [500, 500, 500, 1500]
    dt, dx = _dt_dx(sc)
    mass = _mass(sc)
    for g in range(3):
        _check_record(recs[g], st, mass, group == g, dt, dx, f'non-finite group {g}')
    _check_record(recs[3], st, mass, np.ones(1500, bool), dt, dx, 'non-finite frame')
    eng.close()


def test_env_device_obs_and_diagnostics(hiplib):
    from fluidlab_amd.envs import make
    from fluidlab_amd.optimizer.recorder import Recorder
    import test_hip_env as E
    tgt = Recorder(make('LatteArt-v0', seed=0, loss=False, **E.MINI)).record(write=False)
    env = make('LatteArt-v0', seed=0, loss=True, target=tgt, **E.MINI)
    sim = env.taichi_env.simulator
    assert sim.engine.elib.backend == 'hip-gfx950'
    action = np.full(env.action_space.shape, 0.004, np.float32)
    env.reset()
    assert env.step(action)[3] == {}                          # neither enabled: as before

    def host_obs():
        env._device_obs = False
        try:
            return env._get_obs()
        finally:
            env._device_obs = True

    env.enable_device_obs()
    obs = env.reset()
    ref = host_obs()
    assert obs.dtype == ref.dtype and np.array_equal(obs, ref) and obs.size > 0
    assert env.step(action)[3] == {}
    env.enable_diagnostics()
    obs = env.reset()
    dt, dx = float(np.float32(sim.dt)), float(np.float32(1.0) / np.float32(sim.n_grid))
    for _ in range(3):
        obs, reward, done, info = env.step(action)
        ref = host_obs()
        assert obs.dtype == ref.dtype and np.array_equal(obs, ref)
        assert set(info) == {'courant', 'kinetic', 'n_used', 'n_nonfinite'}
        state = env.taichi_env.get_state_RL()
        vmax = float(np.abs(state['v'][state['used'] != 0].astype(np.float64)).max())
        want = dt * vmax / dx
        print(f'courant {info["courant"]!r} numpy {want!r}')
        assert abs(info['courant'] - want) <= np.spacing(want)           # at most one rounding apart
        assert info['n_used'] == int((state['used'] != 0).sum()) and info['n_nonfinite'] == 0 and info['kinetic'] > 0
        assert not done
    per_body = env.taichi_env.frame_summary(by='body')
    assert len(per_body) == sim.n_bodies and sum(r['n_used'] for r in per_body) == info['n_used']
