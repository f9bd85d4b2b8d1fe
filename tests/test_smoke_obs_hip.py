"""fe_smoke_obs_get* / fe_smoke_obs_add_grad* / fe_eff_add_sr_grad on the GPU: Circulation's observation vector and its cotangent, one launch
each, against the host road and against the composition of the entries they replace -- bit for bit.

Scene: tests/test_host_env.py::_circulation (res 32, 10 Jacobi sweeps) on the HIP engine, after two steps with the demo's action.  Besides the
environment's lattice (list 0, 32 cells) a list of 300 rows with duplicate cells, 288 distinct ones: more than one workgroup of the scatter."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

import test_host_env as H  # noqa: E402
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd._capi import Engine, FeEngineError  # noqa: E402

pytestmark = pytest.mark.gpu

DEMO_ROW = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04])
START_POSE = [0.55, 0.5, 0.27, 0.0, 0.0, 0.0, 0.0, 0.0]
BIG = 2                                                           # the cell list with duplicates


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope='module')
def scene(hiplib):
    env = H._circulation(None, max_substeps_local=None)
    te = env.taichi_env
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(START_POSE)
    host_obs = [np.asarray(env._get_obs())]                      # the host road: the fields are downloaded whole
    for _ in range(2):
        te.step(DEMO_ROW)
        host_obs.append(np.asarray(env._get_obs()))
    env.enable_device_obs()
    eng = te.simulator.engine
    rng = np.random.RandomState(5)
    n = te.smoke_field.n_grid
    distinct = np.stack(np.unravel_index(rng.choice(n ** 3, 288, replace=False), (n,) * 3), axis=1).astype(np.int32)
    cells = np.concatenate([distinct, distinct[rng.choice(288, 12, replace=False)]])[rng.permutation(300)]
    assert len(np.unique(cells, axis=0)) == 288 > 256
    eng.smoke_cells_set(BIG, cells)
    return dict(env=env, te=te, eng=eng, host_obs=host_obs, cells={env.OBS_LIST: env.obs_layout()['smoke']['cells'], BIG: cells})


def _host_vector(sc, list_id, s, f):
    """the vector as the host road builds it, for any (s, f): the effector's state, then the rows of the downloaded fields"""
    te, c = sc['te'], sc['cells'][list_id]
    st = te.smoke_field.get_state(s)
    return np.concatenate([te.agent.get_state(f)[0].flatten(), st['v'][c[:, 0], c[:, 1], c[:, 2]].flatten(), st['q'][c[:, 0], c[:, 1], c[:, 2]].flatten()])


def test_obs_get_equals_the_host_road(scene):
    env, te, eng = scene['env'], scene['te'], scene['eng']
    sim = te.simulator
    ns, S_, L = sim.n_substeps, sim.max_steps_local, sim.max_substeps_local
    e = env.agent.effectors[0].index
    # the current frame: against _get_obs() of the host road itself, and _get_obs() of the device road
    cur = (sim.cur_step_local, sim.cur_substep_local)
    assert cur == (2, 2 * ns)
    want = scene['host_obs'][2]
    assert np.abs(want[9:]).max() > 0 and want.shape == (eng.smoke_obs_size(env.OBS_LIST),)
    got = eng.smoke_obs_get(env.OBS_LIST, cur[0], e, cur[1])
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(env._get_obs()), _bits(want))
    dev = env.observe_dev()
    assert dev.is_cuda and dev.dtype == torch.float32
    eng.sync()
    assert np.array_equal(_bits(dev.cpu().numpy()), _bits(want))
    # frame 0, a middle frame, the last frame; both lists
    for list_id in (env.OBS_LIST, BIG):
        for s, f in ((0, 0), (1, ns), (S_, L)):
            want = _host_vector(scene, list_id, s, f)
            if list_id == env.OBS_LIST and s < 2:
                assert np.array_equal(_bits(want[9:]), _bits(scene['host_obs'][s][9:]))      # (the pose at a frame's first substep is the same; s, r are not)
            got = eng.smoke_obs_get(list_id, s, e, f)
            assert np.array_equal(_bits(got), _bits(want)), (list_id, s, f)
            out = torch.full((eng.smoke_obs_size(list_id),), float('nan'), dtype=torch.float32, device=dev.device)
            eng.smoke_obs_get(list_id, s, e, f, out=out)
            eng.sync()
            assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), (list_id, s, f)


def _adjoints(sc, s, f):
    """every adjoint word the entries may touch, and their neighbours: the smoke adjoints of frames s and s + 1, the AirCon's of f and f + 1"""
    eng, e = sc['eng'], sc['env'].agent.effectors[0].index
    out = []
    for ss in (s, s + 1):
        out += list(eng.smoke_get_grad(ss))
    for ff in (f, f + 1):
        out += [eng.eff_get_state_grad(e, ff), np.array(eng.eff_get_sr_grad(e, ff), np.float32)]
    return [np.array(a) for a in out]


def _occupy(sc, s, f, rng):
    eng, e = sc['eng'], sc['env'].agent.effectors[0].index
    n, qd = eng.smoke_res, eng.smoke_q_dim
    for ss in (s, s + 1):
        eng.smoke_add_grad(ss, gv=rng.normal(size=(n, n, n, 3)).astype(np.float32), gq=rng.normal(size=(n, n, n, qd)).astype(np.float32))
    for ff in (f, f + 1):
        eng.eff_add_state_grad(e, ff, rng.normal(size=7).astype(np.float32))
        eng.eff_add_sr_grad(e, ff, *rng.normal(size=2).astype(np.float32))


def _compose(sc, list_id, s, f, g):
    """the entries fe_smoke_obs_add_grad replaces: the dense fe_smoke_add_grad of np.add.at fields, fe_eff_add_state_grad, fe_eff_add_sr_grad"""
    eng, e, c = sc['eng'], sc['env'].agent.effectors[0].index, sc['cells'][list_id]
    n, qd, m = eng.smoke_res, eng.smoke_q_dim, len(sc['cells'][list_id])
    gv, gq = np.zeros((n, n, n, 3), np.float32), np.zeros((n, n, n, qd), np.float32)
    np.add.at(gv, (c[:, 0], c[:, 1], c[:, 2]), g[9:9 + 3 * m].reshape(m, 3))
    np.add.at(gq, (c[:, 0], c[:, 1], c[:, 2]), g[9 + 3 * m:].reshape(m, qd))
    eng.smoke_add_grad(s, gv=gv, gq=gq)
    eng.eff_add_state_grad(e, f, g[:7])
    eng.eff_add_sr_grad(e, f, g[7], g[8])


@pytest.mark.parametrize('occupied', [False, True], ids=['cleared', 'occupied'])
@pytest.mark.parametrize('list_id', [0, BIG], ids=['lattice', 'dup300'])
@pytest.mark.parametrize('dev', [False, True], ids=['host', 'dev'])
def test_obs_add_grad_equals_the_composition(scene, list_id, occupied, dev):
    te, eng = scene['te'], scene['eng']
    e = scene['env'].agent.effectors[0].index
    s, f = 1, te.simulator.n_substeps
    g = np.random.RandomState(17 + list_id).normal(size=eng.smoke_obs_size(list_id)).astype(np.float32)
    res = []
    for road in ('compose', 'one launch'):
        te.reset_grad()
        if occupied:
            _occupy(scene, s, f, np.random.RandomState(3))
        before = _adjoints(scene, s, f)
        if road == 'compose':
            _compose(scene, list_id, s, f, g)
        else:
            eng.smoke_obs_add_grad(list_id, s, e, f, torch.as_tensor(g).cuda() if dev else g)
            eng.sync()
        res.append((before, _adjoints(scene, s, f)))
    (b0, a0), (b1, a1) = res
    for x, y in zip(b0, b1):
        assert np.array_equal(_bits(x), _bits(y))                # the same starting point on both roads
    for k, (x, y) in enumerate(zip(a0, a1)):
        assert np.array_equal(_bits(x), _bits(y)), k             # every word of frame s / f: at the listed cells and everywhere else
    assert not np.array_equal(_bits(a1[0]), _bits(b1[0])) and not np.array_equal(_bits(a1[1]), _bits(b1[1]))      # gv[s], gq[s] changed
    assert not np.array_equal(_bits(a1[4]), _bits(b1[4])) and not np.array_equal(_bits(a1[5]), _bits(b1[5]))      # pose and s, r of f changed
    for k in (2, 3, 6, 7):                                       # frame s + 1 and frame f + 1: no word changed
        assert np.array_equal(_bits(a1[k]), _bits(b1[k])), k
    c = scene['cells'][list_id]
    other = np.ones((eng.smoke_res,) * 3, bool)
    other[c[:, 0], c[:, 1], c[:, 2]] = False
    assert np.array_equal(_bits(a1[0][other]), _bits(b1[0][other])) and np.array_equal(_bits(a1[1][other]), _bits(b1[1][other]))
    te.reset_grad()


def test_sr_grad_roundtrip(scene):
    te, eng = scene['te'], scene['eng']
    aircon = scene['env'].agent.effectors[0]
    te.reset_grad()
    assert aircon.get_sr_grad(3) == (0.0, 0.0)
    aircon.add_sr_grad(3, 0.25, -1.5)
    aircon.add_sr_grad(3, 0.5, 0.25)
    assert aircon.get_sr_grad(3) == (0.75, -1.25) and aircon.get_sr_grad(2) == (0.0, 0.0) and aircon.get_sr_grad(4) == (0.0, 0.0)
    te.reset_grad()


def _rc(eng, name, *args):
    return getattr(eng.lib, name)(eng.h, *args)


def test_refusals_change_nothing(scene, hiplib):
    te, eng, env = scene['te'], scene['eng'], scene['env']
    e = env.agent.effectors[0].index
    sim = te.simulator
    S_, L = sim.max_steps_local, sim.max_substeps_local
    n0 = eng.smoke_obs_size(0)
    te.reset_grad()
    _occupy(scene, 1, sim.n_substeps, np.random.RandomState(9))
    before = _adjoints(scene, 1, sim.n_substeps)
    g = np.ones(n0 + 4, np.float32)
    out = np.full(n0 + 4, 7.0, np.float32)
    gd, outd = torch.ones(n0 + 4, dtype=torch.float32, device='cuda'), torch.full((n0 + 4,), 7.0, dtype=torch.float32, device='cuda')
    torch.cuda.synchronize()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    t = lambda a: C.c_void_p(a.data_ptr())
    f1 = sim.n_substeps
    bad = [(3, 1, e, f1, n0),            # a list that is not set
           (-1, 1, e, f1, n0), (_capi.FE_SMOKE_MAX_LISTS, 1, e, f1, n0),
           (0, -1, e, f1, n0), (0, S_ + 1, e, f1, n0),           # s out of range
           (0, 1, e, -1, n0), (0, 1, e, L + 1, n0),              # f out of range
           (0, 1, e + 1, f1, n0), (0, 1, -1, f1, n0),            # no such effector
           (0, 1, e, f1, n0 - 1), (0, 1, e, f1, n0 + 1), (0, 1, e, f1, eng.smoke_obs_size(BIG))]     # a wrong length
    for lst, s, ee, f, nn in bad:
        for name, host, devp in (('fe_smoke_obs_get', p(out), t(outd)), ('fe_smoke_obs_add_grad', p(g), t(gd))):
            assert _rc(eng, name, lst, s, ee, f, host, nn) != 0, (name, lst, s, ee, f, nn)
            assert eng.lib.fe_last_error(eng.h)
            assert _rc(eng, name + '_dev', lst, s, ee, f, devp, nn) != 0, (name, lst, s, ee, f, nn)
    for name in ('fe_smoke_obs_get', 'fe_smoke_obs_get_dev', 'fe_smoke_obs_add_grad', 'fe_smoke_obs_add_grad_dev'):
        assert _rc(eng, name, 0, 1, e, f1, None, n0) != 0        # a NULL pointer
    eng.sync()
    assert (out == 7.0).all() and bool((outd == 7.0).all())
    for x, y in zip(before, _adjoints(scene, 1, sim.n_substeps)):
        assert np.array_equal(_bits(x), _bits(y))
    with pytest.raises(FeEngineError):
        eng.smoke_obs_add_grad(3, 1, e, f1, np.ones(9, np.float32))
    te.reset_grad()
    # an effector that is not an AirCon, and an engine without a smoke field
    import test_smoke as TS
    eng2, e2 = TS.make_smoke_engine(hiplib, res=12, steps=3)
    plain = eng2.add_effector(type=_capi.FE_EFF_PLAIN, action_dim=3, action_scale_v=(1, 1, 1), action_scale_p=(1, 1, 1), boundary=hiplib.make_boundary())
    eng2.smoke_cells_set(0, np.array([[1, 4, 1], [2, 5, 2]], np.int32))
    n2 = eng2.smoke_obs_size(0)
    eng2.reset_grad()
    buf = np.ones(n2, np.float32)
    assert _rc(eng2, 'fe_smoke_obs_add_grad', 0, 1, e2, 2, p(buf), n2) == 0       # (the AirCon passes)
    ref = [np.array(a) for a in eng2.smoke_get_grad(1)] + [eng2.eff_get_state_grad(plain, 2), eng2.eff_get_state_grad(e2, 2)]
    for name in ('fe_smoke_obs_get', 'fe_smoke_obs_add_grad'):
        assert _rc(eng2, name, 0, 1, plain, 2, p(buf), n2) != 0
        assert b'AirCon' in eng2.lib.fe_last_error(eng2.h)
    with pytest.raises(FeEngineError):
        eng2.eff_add_sr_grad(plain, 2, 1.0, 1.0)
    with pytest.raises(FeEngineError):
        eng2.eff_get_sr_grad(plain, 2)
    now = [np.array(a) for a in eng2.smoke_get_grad(1)] + [eng2.eff_get_state_grad(plain, 2), eng2.eff_get_state_grad(e2, 2)]
    for x, y in zip(ref, now):
        assert np.array_equal(_bits(x), _bits(y))
    assert (buf == 1.0).all()
    eng2.close()
    eng3 = Engine(hiplib, n_grid=8, n_particles=4, max_substeps_local=6, n_substeps=2, max_action_steps=3, dt=2e-4, p_vol=(0.5 / 8) ** 2,
                  gravity=(0.0, -10.0, 0.0), boundary=hiplib.make_boundary(), device=0)
    eng3.init_particles(np.full((4, 3), -100.0, np.float32), np.zeros(4, np.int32), np.zeros(4, np.int32), np.full(4, 200, np.int32),
                        np.zeros(4), np.full(4, 277.78), np.ones(4), np.zeros(4, np.int32))
    a3 = eng3.add_effector(type=_capi.FE_EFF_AIRCON, action_dim=8, action_scale_v=(1,) * 8, action_scale_p=(1,) * 8, boundary=hiplib.make_boundary(),
                           inject_v=(-0.3, 0.1, 1.0))
    for name in ('fe_smoke_obs_get', 'fe_smoke_obs_add_grad'):
        assert _rc(eng3, name, 0, 0, a3, 0, p(buf), n2) != 0
        assert b'no smoke field' in eng3.lib.fe_last_error(eng3.h)
    assert eng3.eff_get_sr_grad(a3, 0) == (0.0, 0.0) and not eng3.eff_get_state_grad(a3, 0).any()
    eng3.close()
