"""GPU: the smoke-field reads of include/fluidengine_ext.h (fe_smoke_cells_*, fe_smoke_loss_*, fe_smoke_summary; fluidlab_amd/csrc/fe_smoke_reads.h)
against numpy on downloaded frames, and Circulation-v0 on the device roads against the roads it has always had."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402
import test_smoke as TS  # noqa: E402

from fluidlab_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
RES, STEPS = 12, 3
U = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _engine(hiplib, q_dim, seed=0):
    """res 12, max_steps_local 3; frames 0 and 3 filled from seeded random arrays"""
    eng, _ = TS.make_smoke_engine(hiplib, steps=STEPS, q_dim=q_dim, seed=seed)
    rng = np.random.RandomState(100 + seed)
    frames = {}
    for s in (0, STEPS):
        v = rng.normal(0, 1.5, (RES, RES, RES, 3)).astype(np.float32)
        q = rng.uniform(-0.5, 1.5, (RES, RES, RES, q_dim)).astype(np.float32)
        eng.smoke_set_frame(s, v=v, q=q)
        frames[s] = eng.smoke_get_frame(s, ('v', 'q'))
        assert np.array_equal(_bits(frames[s]['v']), _bits(v)) and np.array_equal(_bits(frames[s]['q']), _bits(q))
    return eng, frames


@pytest.fixture(scope='module', params=[1, 3], ids=['q1', 'q3'])
def field(hiplib, request):
    eng, frames = _engine(hiplib, request.param)
    yield eng, frames, request.param
    eng.close()


def _unique_cells(rng, n):
    return np.stack(np.unravel_index(rng.choice(RES ** 3, n, replace=False), (RES,) * 3), axis=1).astype(np.int32)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_gather_is_the_indexed_frame(field, n):
    import torch
    eng, frames, qd = field
    rng = np.random.RandomState(n)
    cells = rng.randint(0, RES, (n, 3)).astype(np.int32)
    cells[0] = (0, 0, 0)
    if n > 1:
        cells[-1] = (RES - 1,) * 3
    if n > 2:
        cells[n // 2] = cells[1]                                  # a duplicate
        cells[1 + n // 3] = (0, 0, 0)
    lid = n % _capi.FE_SMOKE_MAX_LISTS
    eng.smoke_cells_set(lid, cells)
    i, j, k = cells.T
    for s in (0, STEPS):
        rows = eng.smoke_cells_get(lid, s)
        assert rows['v'].shape == (n, 3) and rows['q'].shape == (n, qd)
        assert np.array_equal(_bits(rows['v']), _bits(frames[s]['v'][i, j, k]))
        assert np.array_equal(_bits(rows['q']), _bits(frames[s]['q'][i, j, k]))
        tv = torch.full((n, 3), -7.0, dtype=torch.float32, device='cuda:0')
        tq = torch.full((n, qd), -7.0, dtype=torch.float32, device='cuda:0')
        eng.smoke_cells_get_dev(lid, s, v=tv, q=tq)
        eng.sync()
        assert np.array_equal(_bits(tv.cpu().numpy()), _bits(rows['v'])) and np.array_equal(_bits(tq.cpu().numpy()), _bits(rows['q']))
        tq.fill_(-7.0)
        eng.smoke_cells_get_dev(lid, s, v=None, q=tq)              # a NULL pointer is skipped
        eng.sync()
        assert np.array_equal(_bits(tq.cpu().numpy()), _bits(rows['q']))
    eng.smoke_cells_set(lid, None)
    with pytest.raises(_capi.FeEngineError, match='not set'):
        eng.smoke_cells_get(lid, 0)


def _dense_grad(cells, comp, qd, g):
    """add_q_grad_at's arithmetic (fluidengine/simulators/smoke_field.py), for component comp"""
    gq = np.zeros((RES, RES, RES, qd), np.float32)
    np.add.at(gq, (cells[:, 0], cells[:, 1], cells[:, 2], comp), np.asarray(g))
    return gq


@pytest.mark.parametrize('kind', [_capi.FE_SMOKE_L1, _capi.FE_SMOKE_SQ], ids=['l1', 'sq'])
@pytest.mark.parametrize('n', [1, 15, 65, 300])
def test_loss_value_and_gradient(field, n, kind):
    eng, frames, qd = field
    comp = 0 if qd == 1 else 2
    s, scale = STEPS, 0.37
    rng = np.random.RandomState(1000 + n)
    cells = _unique_cells(rng, n)
    i, j, k = cells.T
    q64 = frames[s]['q'][i, j, k, comp].astype(np.float64)
    w = rng.uniform(0.2, 2.0, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    if n > 1:
        w[0], w[1] = -abs(w[0]), abs(w[1])                        # mixed signs
    t = rng.uniform(-0.5, 1.5, n)
    tie = n // 2
    t[tie] = q64[tie]                                             # exactly the cell's fp32 value
    eng.smoke_cells_set(0, cells)
    eng.smoke_loss_alloc(3)
    eng.smoke_loss_set(0, t, weight=w, comp=comp, kind=kind)
    eng.smoke_cells_set(0, cells[::-1][:1])                       # the loss keeps the cells it was set with
    d = q64 - t
    terms = w * (np.abs(d) if kind == _capi.FE_SMOKE_L1 else d * d)
    want, bound = terms.sum(), (n - 1) * U * np.abs(terms).sum()
    eng.smoke_loss_step(1, s)
    one = eng.smoke_loss_get(3)
    print(f'n {n} kind {kind} q_dim {qd}: value {one[1]!r} numpy {want!r} diff {abs(one[1] - want):.3e} bound {bound:.3e}')
    assert one[0] == 0 and one[2] == 0
    assert abs(one[1] - want) <= bound
    eng.smoke_loss_step(1, s)
    eng.smoke_loss_step(2, s)
    two = eng.smoke_loss_get(3)
    assert two[2] == one[1]                                       # two evaluations of a frame: the same bits
    assert two[1] == 2 * one[1] and abs(two[1] - 2 * want) <= 2 * bound            # ... and a second call accumulates (v + v is exact)
    eng.smoke_loss_clear()
    assert np.all(eng.smoke_loss_get(3) == 0)

    # CirculationLoss.step_grad's g = sign(q - t) * weight * total_loss_grad; the squared kind as the header states it
    g = np.sign(d) * w * scale if kind == _capi.FE_SMOKE_L1 else scale * w * (2.0 * d)
    dense = _dense_grad(cells, comp, qd, g)
    got = []
    for rep in range(2):
        eng.smoke_reset_grad()
        eng.smoke_loss_step_grad(1, s, scale)
        gv, gq = eng.smoke_get_grad(s)
        assert not gv.any()
        assert np.array_equal(_bits(gq), _bits(dense))
        got.append(gq)
        gv0, gq0 = eng.smoke_get_grad(0)
        assert not gv0.any() and not gq0.any()
    assert np.array_equal(_bits(got[0]), _bits(got[1]))
    assert got[0][i[tie], j[tie], k[tie], comp] == 0
    assert np.count_nonzero(got[0]) == n - 1
    after = eng.smoke_get_frame(s, ('v', 'q'))                      # the loss calls changed no field
    assert np.array_equal(_bits(after['v']), _bits(frames[s]['v'])) and np.array_equal(_bits(after['q']), _bits(frames[s]['q']))

    # a NaN planted in a detector cell: the value is NaN, that cell gets no gradient, the others theirs
    bad = 0
    qn = frames[s]['q'].copy()
    qn[i[bad], j[bad], k[bad], comp] = np.nan
    eng.smoke_set_frame(s, q=qn)
    try:
        eng.smoke_loss_clear()
        eng.smoke_loss_step(0, s)
        assert np.isnan(eng.smoke_loss_get(1)[0])
        eng.smoke_reset_grad()
        eng.smoke_loss_step_grad(0, s, scale)
        gq = eng.smoke_get_grad(s)[1]
        gn = np.array(g)
        gn[bad] = 0.0
        assert gq[i[bad], j[bad], k[bad], comp] == 0
        assert np.array_equal(_bits(gq), _bits(_dense_grad(cells, comp, qd, gn)))
    finally:
        eng.smoke_set_frame(s, q=frames[s]['q'])
        eng.smoke_reset_grad()
        eng.smoke_loss_clear()


def test_errors_leave_the_previous_state(hiplib):
    bare = S.make_engine(hiplib, S.water_block(n_grid=8, n_particles=8))
    for call in (lambda: bare.smoke_cells_set(0, np.zeros((1, 3), np.int32)), lambda: bare.smoke_cells_get(0, 0), lambda: bare.smoke_loss_alloc(2),
                 lambda: bare.smoke_loss_set(0, np.zeros(1)), lambda: bare.smoke_loss_clear(), lambda: bare.smoke_loss_step(0, 0),
                 lambda: bare.smoke_loss_step_grad(0, 0), lambda: bare.smoke_loss_get(1), lambda: bare.smoke_summary(0)):
        with pytest.raises(_capi.FeEngineError, match='no smoke field'):
            call()
    t = _capi.FeLossTerm()
    t.kind, t.axis_mask = 7, 1
    t.a = _capi.FeLossSel(0, 8, -1, 0)
    with pytest.raises(_capi.FeEngineError, match='unknown term kind'):                 # kind 7 still names nothing
        bare.task_loss_set_terms([t])
    bare.close()

    qd = 3
    eng, frames = _engine(hiplib, qd, seed=1)
    rng = np.random.RandomState(9)
    cells = _unique_cells(rng, 20)
    i, j, k = cells.T
    # steps before alloc / set
    eng.smoke_cells_set(1, cells)
    with pytest.raises(_capi.FeEngineError, match='fe_smoke_loss_alloc first'):
        eng.smoke_loss_step(0, 0)
    with pytest.raises(_capi.FeEngineError, match='fe_smoke_loss_alloc first'):
        eng.smoke_loss_get(1)
    eng.smoke_loss_alloc(2)
    for call in (lambda: eng.smoke_loss_step(0, 0), lambda: eng.smoke_loss_step_grad(0, 0, 1.0)):
        with pytest.raises(_capi.FeEngineError, match='fe_smoke_loss_set first'):
            call()
    t, w = rng.uniform(0, 1, 20), rng.uniform(-1, 1, 20)
    eng.smoke_loss_set(1, t, weight=w, comp=1)
    eng.smoke_loss_step(0, STEPS)
    value = eng.smoke_loss_get(2)[0]
    assert value != 0

    def survived():
        rows = eng.smoke_cells_get(1, STEPS)
        assert np.array_equal(_bits(rows['v']), _bits(frames[STEPS]['v'][i, j, k])) and np.array_equal(_bits(rows['q']), _bits(frames[STEPS]['q'][i, j, k]))
        eng.smoke_loss_step(1, STEPS)
        sl = eng.smoke_loss_get(2)
        assert sl[0] == value and sl[1] == value
        eng.smoke_loss_clear()
        eng.smoke_loss_step(0, STEPS)

    one = np.zeros((1, 3), np.int32)
    for lid in (-1, _capi.FE_SMOKE_MAX_LISTS):
        for call in (lambda: eng.smoke_cells_set(lid, one), lambda: eng.smoke_cells_get(lid, 0), lambda: eng.smoke_loss_set(lid, np.zeros(1))):
            with pytest.raises(_capi.FeEngineError, match='list id out of range'):
                call()
    for call in (lambda: eng.smoke_cells_get(2, 0), lambda: eng.smoke_loss_set(2, np.zeros(1))):
        with pytest.raises(_capi.FeEngineError, match='not set'):
            call()
    for bad in ((RES, 0, 0), (0, -1, 0), (0, 0, RES)):
        worse = cells.copy()
        worse[7] = bad
        with pytest.raises(_capi.FeEngineError, match='cell out of range'):
            eng.smoke_cells_set(1, worse)
    with pytest.raises(_capi.FeEngineError, match='FE_SMOKE_MAX_LIST_CELLS'):
        eng.smoke_cells_set(1, np.zeros((_capi.FE_SMOKE_MAX_LIST_CELLS + 1, 3), np.int32))
    survived()
    for comp in (-1, qd):
        with pytest.raises(_capi.FeEngineError, match='comp outside'):
            eng.smoke_loss_set(1, t, weight=w, comp=comp)
    for kind in (-1, 2):
        with pytest.raises(_capi.FeEngineError, match='unknown kind'):
            eng.smoke_loss_set(1, t, weight=w, comp=1, kind=kind)
    dup = cells.copy()
    dup[11] = dup[3]
    eng.smoke_cells_set(3, dup)                                   # fine for reading ...
    assert np.array_equal(_bits(eng.smoke_cells_get(3, 0)['q']), _bits(frames[0]['q'][dup[:, 0], dup[:, 1], dup[:, 2]]))
    with pytest.raises(_capi.FeEngineError, match='twice'):       # ... refused as detectors
        eng.smoke_loss_set(3, t, weight=w, comp=1)
    survived()
    for s_loss in (-1, 2):
        for call in (lambda: eng.smoke_loss_step(s_loss, 0), lambda: eng.smoke_loss_step_grad(s_loss, 0, 1.0)):
            with pytest.raises(_capi.FeEngineError, match='loss step out of range'):
                call()
    with pytest.raises(_capi.FeEngineError, match='steps out of range'):
        eng.smoke_loss_get(3)
    for s in (-1, STEPS + 1):
        for call in (lambda: eng.smoke_cells_get(1, s), lambda: eng.smoke_loss_step(0, s), lambda: eng.smoke_loss_step_grad(0, s, 1.0), lambda: eng.smoke_summary(s)):
            with pytest.raises(_capi.FeEngineError, match='smoke frame out of range'):
                call()
    rec = _capi.FeSmokeSummary()
    assert eng.lib.fe_smoke_summary(eng.h, 0, ctypes.byref(rec), ctypes.sizeof(rec) - 8) != 0
    assert b'record_size' in eng.lib.fe_last_error(eng.h)
    survived()
    # fe_smoke_create drops every list and the loss
    eng.smoke_create(res=RES, dt=0.03, solver_iters=2, q_dim=1, max_steps_local=2, lower_y=3, higher_y=8)
    with pytest.raises(_capi.FeEngineError, match='not set'):
        eng.smoke_cells_get(1, 0)
    with pytest.raises(_capi.FeEngineError, match='fe_smoke_loss_alloc first'):
        eng.smoke_loss_step(0, 0)
    eng.close()


def _summary_reference(v, q, ly, hy, dt):
    n = v.shape[0]
    j0, j1 = max(ly + 1, 0), min(hy, n)
    qd = q.shape[-1]
    vs, qs = v[:, j0:j1].reshape(-1, 3).astype(np.float64), q[:, j0:j1].reshape(-1, qd).astype(np.float64)
    ok = np.isfinite(vs).all(1) & np.isfinite(qs).all(1)
    r = dict(n_cells=len(vs), n_nonfinite=int((~ok).sum()), v_max=0.0, kinetic=0.0, a_kinetic=0.0, q_sum=np.zeros(3), a_q=np.zeros(3), q_min=np.zeros(3), q_max=np.zeros(3))
    if ok.any():
        vs, qs = vs[ok], qs[ok]
        r['v_max'] = np.abs(vs).max()
        r['kinetic'] = r['a_kinetic'] = 0.5 * (vs * vs).sum()
        r['q_sum'][:qd], r['a_q'][:qd], r['q_min'][:qd], r['q_max'][:qd] = qs.sum(0), np.abs(qs).sum(0), qs.min(0), qs.max(0)
    r['courant'] = float(np.float32(dt)) * r['v_max']
    return r


def _check_summary(got, want):
    print('summary', {k: got[k] for k in ('n_cells', 'n_nonfinite', 'v_max', 'courant', 'kinetic')}, got['q_sum'], got['q_min'], got['q_max'])
    assert got['n_cells'] == want['n_cells'] and got['n_nonfinite'] == want['n_nonfinite']
    assert got['v_max'] == want['v_max']
    assert abs(got['courant'] - want['courant']) <= 2.0 ** -52 * abs(want['courant'])
    assert abs(got['kinetic'] - want['kinetic']) <= 1e-11 * want['a_kinetic']
    assert np.all(np.abs(got['q_sum'] - want['q_sum']) <= 1e-11 * want['a_q'])
    assert np.array_equal(got['q_min'], want['q_min']) and np.array_equal(got['q_max'], want['q_max'])


@pytest.mark.parametrize('res,ly,hy,qd', [(12, 3, 8, 1), (20, 0, 19, 3), (12, 5, 6, 1)], ids=['res12-576', 'res20-7200', 'empty'])
def test_summary(hiplib, res, ly, hy, qd):
    eng, _ = TS.make_smoke_engine(hiplib, steps=2, q_dim=1)
    dt = 0.03
    eng.smoke_create(res=res, dt=dt, solver_iters=2, q_dim=qd, max_steps_local=2, lower_y=ly, higher_y=hy)
    rng = np.random.RandomState(res + hy)
    v = rng.normal(0, 1.5, (res, res, res, 3)).astype(np.float32)
    q = rng.uniform(-0.5, 1.5, (res, res, res, qd)).astype(np.float32)
    v[:, ly], q[:, ly] = 1e6, -1e6                                 # huge values just outside the slab must not show
    v[:, hy], q[:, hy] = -1e6, 1e6
    cells = res * max(hy - ly - 1, 0) * res
    if cells:
        v[0, ly + 1, 0, 1] = -50.0                                # the maximum of |v| in the first slab cell
        q[res - 1, hy - 1, res - 1, 0] = -9.0                     # the minimum of q in the last
        v[2, ly + 1, 5, 2] = np.nan
        q[res - 2, hy - 1, 3, qd - 1] = np.inf
    other = rng.normal(0, 1, (res, res, res, 3)).astype(np.float32)
    eng.smoke_set_frame(0, v=other, q=q)
    eng.smoke_set_frame(2, v=v, q=q)
    want = _summary_reference(v, q, ly, hy, dt)
    assert want['n_cells'] == cells and want['n_nonfinite'] == (2 if cells else 0)
    got = eng.smoke_summary(2)
    _check_summary(got, want)
    if cells:
        assert got['v_max'] == 50.0 and got['q_min'][0] == -9.0 and got['q_max'][0] < 2.0 and np.all(got['q_sum'][qd:] == 0)
        again = eng.smoke_summary(2)
        assert all(np.array_equal(np.asarray(got[k]), np.asarray(again[k])) for k in got)      # the same bits twice
        _check_summary(eng.smoke_summary(0), _summary_reference(other, q, ly, hy, dt))
        # every cell non-finite: zeros apart from the two counts
        eng.smoke_set_frame(1, v=np.full_like(v, np.nan), q=q)
        rec = eng.smoke_summary(1)
        assert rec['n_cells'] == cells == rec['n_nonfinite']
        assert rec['v_max'] == 0 and rec['courant'] == 0 and rec['kinetic'] == 0 and not rec['q_sum'].any() and not rec['q_min'].any() and not rec['q_max'].any()
    else:
        assert got['n_cells'] == 0 and got['n_nonfinite'] == 0 and got['v_max'] == 0 and got['kinetic'] == 0 and not got['q_min'].any() and not got['q_max'].any()
    back = eng.smoke_get_frame(2, ('v', 'q'))
    assert np.array_equal(_bits(back['v']), _bits(v)) and np.array_equal(_bits(back['q']), _bits(q))
    eng.close()


def test_reads_leave_a_rollout_bit_identical(hiplib):
    """run_smoke's forward rollout (tests/test_smoke.py) with gather, loss-step and summary calls between its steps, against run_smoke itself"""
    res, H = TS.RES, 3
    acts = TS._actions(H)
    zero_v, zero_q = np.zeros((res, res, res, 3), np.float32), np.zeros((res, res, res, 1), np.float32)
    plain = TS.run_smoke(hiplib, acts, zero_v, zero_q)['final']
    eng, e = TS.make_smoke_engine(hiplib)
    rng = np.random.RandomState(4)
    eng.smoke_cells_set(0, rng.randint(0, res, (100, 3)))
    eng.smoke_cells_set(1, _unique_cells(rng, 15))
    eng.smoke_loss_alloc(H)
    eng.smoke_loss_set(1, rng.uniform(0, 1, 15))
    for s in range(H):
        eng.eff_set_action(e, s, s, 2, acts[s])
        eng.smoke_cells_get(0, s)
        eng.smoke_step(s, 2 * s)
        eng.smoke_loss_step(s, s + 1)
        eng.smoke_summary(s + 1)
        eng.step(2 * s, 2 * s, 2, 1)
        eng.smoke_cells_get(1, s + 1)
    assert np.all(np.isfinite(eng.smoke_loss_get(H))) and eng.smoke_loss_get(H).all()
    fin = eng.smoke_get_frame(H, ('v', 'q', 'p'))
    eng.close()
    for k in ('v', 'q', 'p'):
        assert np.array_equal(_bits(fin[k]), _bits(plain[k])), k


@pytest.mark.parametrize('kw', [dict(max_substeps_local=None), dict(max_substeps_local=20, ckpt_dest='cpu')], ids=['resident', 'chunked'])
def test_circulation_env_on_the_device_roads(hiplib, kw):
    """Circulation-v0 as built against the same environment with enable_device_obs(), enable_device_loss() and enable_diagnostics() on"""
    import test_host_env as H
    from fluidlab_amd.optimizer.solver import Solver
    from fluidlab_amd.utils.config import load_config
    out = []
    for device in (False, True):
        env = H._circulation(None, **kw)
        if device:
            env.enable_device_obs()
            env.enable_device_loss()
            env.enable_diagnostics()
        cfg = load_config('configs/exp_circulation.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        pol.actions_v[:] = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04])
        pol.actions_p[:] = np.array([0.55, 0.5, 0.27, 0.0, 0.0, 0.0, 0.0, 0.0])
        info, g = Solver(env, None, cfg).forward_backward(env._init_state['state'], pol, env.horizon, env.horizon_action)
        temp = np.array(env.taichi_env.loss.temp_loss)
        obs, rewards, infos = [env.reset()], [], []
        for i in range(env.horizon):
            o, r, done, step_info = env.step(np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04]) * (1 + 0.1 * i))
            obs.append(o); rewards.append(r); infos.append(step_info)
        assert done
        out.append((info['loss'], np.asarray(g), obs, rewards, infos, temp))
    (la, ga, oa, ra, ia, ta), (lb, gb, ob, rb, ib, tb) = out
    for a, b in zip(oa, ob):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))
    assert len(oa) == 7 and np.isfinite(oa[-1]).all() and not np.array_equal(oa[0], oa[-1])
    print(f'loss host {la!r} device {lb!r}; grad cos {S.cosine(ga, gb):.8f} rel L2 {S.rel_l2(ga, gb):.3e}')
    assert la != 0 and abs(la - lb) <= 1e-12 * abs(la)
    assert S.cosine(ga, gb) >= 0.9999 and S.rel_l2(ga, gb) <= 2e-2
    assert np.allclose(ra, rb, rtol=0, atol=1e-12 * 11) and np.allclose(ta, tb, rtol=1e-12, atol=0)
    assert all(i == {} for i in ia)
    for i in ib:
        assert set(i) == {'courant', 'kinetic', 'n_nonfinite', 'q_min', 'q_max'}
        assert i['n_nonfinite'] == 0 and np.isfinite(i['courant']) and np.isfinite(i['kinetic']) and np.isfinite(i['q_min']).all() and np.isfinite(i['q_max']).all()
    assert ib[-1]['kinetic'] > 0 and ib[-1]['q_min'][0] < ib[-1]['q_max'][0]
