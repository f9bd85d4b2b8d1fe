"""GPU: the full Python stack (envs -> TaichiEnv -> MPMSimulator -> C ABI -> HIP kernels) against the same stack
on the fp64 oracle library, including the chunked checkpoint/recompute protocol on sorted particle orders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd.envs import make
from fluidlab_amd.optimizer.recorder import Recorder
from fluidlab_amd.optimizer.solver import Solver
from fluidlab_amd.utils.config import load_config

pytestmark = pytest.mark.gpu
MINI = dict(quality=0.5, particle_density=4e4, n_pool=300, horizon=12, horizon_action=8)


def _solver_cfg():
    cfg = load_config('configs/exp_latteart.yaml').SOLVER
    cfg.n_iters = 2
    return cfg


def _fwd_bwd(lib, target, seed_actions=4, **kw):
    env = make('LatteArt-v0', seed=0, loss=True, target=target, engine_lib=lib, **MINI, **kw)
    cfg = _solver_cfg()
    policy = env.trainable_policy(cfg.optim, cfg.init_range)
    policy.actions_v[:] = np.random.RandomState(seed_actions).uniform(-0.004, 0.004, policy.actions_v.shape)
    info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], policy, env.horizon, env.horizon_action)
    return info['loss'], g, env


def test_latteart_env_on_hip_matches_oracle(hiplib, oracle64, monkeypatch):
    from fluidlab_amd.fluidengine.effectors import Injector
    base = np.random.RandomState(7).uniform(size=(20, 2, 3)).astype(np.float32)
    monkeypatch.setattr(Injector, 'random_vector_factory', staticmethod(lambda n, flux, dim: np.tile(base, (n // 20 + 1, 1, 1))[:n]))
    tgt = Recorder(make('LatteArt-v0', seed=0, loss=False, engine_lib=oracle64, **MINI)).record(write=False)
    tgt_gpu = Recorder(make('LatteArt-v0', seed=0, loss=False, engine_lib=None, **MINI)).record(write=False)   # None = HIP library
    assert (tgt_gpu['used'][-1] == tgt['used'][-1]).all()
    assert S.rel_l2(tgt_gpu['x'][-1][tgt['used'][-1] == 1], tgt['x'][-1][tgt['used'][-1] == 1]) <= 1e-5
    tgt32 = dict(tgt, x=[np.asarray(t, np.float32) for t in tgt['x']])
    loss_o, g_o, _ = _fwd_bwd(oracle64, tgt)
    # 'gpu': chunk checkpoints kept in HBM as torch tensors, filled through fe_get_frame_dev / fe_set_frame_dev
    for kw in (dict(max_substeps_local=None), dict(max_substeps_local=20, ckpt_dest='cpu'), dict(max_substeps_local=40, ckpt_dest='disk'),
               dict(max_substeps_local=20, ckpt_dest='gpu')):
        loss_g, g_g, env = _fwd_bwd(hiplib, tgt32, **kw)
        if kw.get('ckpt_dest') == 'gpu':
            ck = next(iter(env.taichi_env.simulator.ckpt_ram.values()))
            assert ck['x'].is_cuda and ck['used'].is_cuda
        assert env.taichi_env.simulator.engine.elib.backend == 'hip-gfx950'
        assert abs(loss_g - loss_o) <= 1e-4 * abs(loss_o), kw
        # measured ~8e-7; a 1e-2 bound once let a 1% error of a stale-grid bug through
        assert S.cosine(g_g, g_o) >= 0.999999 and S.rel_l2(g_g, g_o) <= 1e-4, (kw, S.rel_l2(g_g, g_o))


def test_solver_reduces_loss_on_hip(hiplib):
    tgt = Recorder(make('LatteArt-v0', seed=0, loss=False, **MINI)).record(write=False)
    env = make('LatteArt-v0', seed=0, loss=True, target=tgt, **MINI)
    cfg = _solver_cfg()
    cfg.n_iters = 3
    losses = []
    Solver(env, None, cfg).solve(callback=lambda it, info, pol: losses.append(info['loss']))
    assert losses[0] > losses[1] > losses[2] > 0


def test_static_cup_through_python_stack(hiplib, oracle32):
    """Same analytic-cup scene on the HIP engine and on the oracle through TaichiEnv.add_static (meshes.py)."""
    import test_host_env as H
    a, b = H._cup_scene(None), H._cup_scene(oracle32)
    for _ in range(60):
        a.step(None); b.step(None)
    xa, xb = a.get_state()['state']['x'], b.get_state()['state']['x']
    assert np.isfinite(xa).all()
    assert np.abs(xa - xb).max() <= 2e-4          # fp32 engine vs fp32 oracle over 600 substeps with contact


def test_agent_rigid_through_python_stack(hiplib, oracle32):
    """AgentRigid + Rigid (analytic cylinder mesh) on the HIP engine vs the oracle through TaichiEnv, forward and action
    gradient."""
    import test_host_env as H
    out = []
    for lib in (None, oracle32):
        te = H._stir_env(lib)
        te.set_state(te.get_state()['state'], grad_enabled=True)
        actions = np.tile([0.02, 0.0, 0.0, 0.0, 0.3, 0.0], (6, 1))
        for a in actions:
            te.step(a)
        x1 = te.get_state()['state']['x']
        te.reset_grad()
        te.simulator.engine.add_grad(te.simulator.cur_substep_local, np.ones_like(x1), None, None, None)
        for a in actions[::-1]:
            te.step_grad(a)
        out.append((x1, te.agent.get_grad(6)))
    (xa, ga), (xb, gb) = out
    assert np.abs(xa - xb).max() <= 2e-5
    assert S.cosine(ga, gb) >= 0.9999 and S.rel_l2(ga, gb) <= 2e-2


def test_circulation_env_on_the_gpu(hiplib, oracle32):
    """Circulation-v0 (SmokeField + AirCon + room SDF + CirculationLoss) on the HIP engine vs the oracle: loss and the
    8-dof action gradient of one Solver pass."""
    import test_host_env as H
    out = []
    for lib in (None, oracle32):
        env = H._circulation(lib, max_substeps_local=None)
        cfg = load_config('configs/exp_circulation.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        pol.actions_v[:] = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04])
        pol.actions_p[:] = np.array([0.55, 0.5, 0.27, 0.0, 0.0, 0.0, 0.0, 0.0])
        info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], pol, env.horizon, env.horizon_action)
        out.append((info['loss'], g, env.taichi_env.smoke_field.get_state(6)['q']))
    (la, ga, qa), (lb, gb, qb) = out
    assert abs(la - lb) <= 1e-4 * abs(lb)
    assert np.abs(qa - qb).max() <= 1e-4
    assert S.cosine(ga, gb) >= 0.9999 and S.rel_l2(ga, gb) <= 2e-2



def _grad_no_worse_than_fp32_oracle(tag, g_hip, g_o32, g_o64, margin):
    """Where contact branches and the rigid-body SVD make the action gradient ill-conditioned in fp32, two fp32 implementations
    need not agree with each other; what can be asked is that the engine is as close to the fp64 oracle as the oracle's own fp32
    build is (up to `margin` in the cosine)."""
    c_hip, c_o32 = S.cosine(g_hip, g_o64), S.cosine(g_o32, g_o64)
    print(f'MEASURED {tag}: grad cos vs fp64 oracle: hip {c_hip:.6f}, fp32 oracle {c_o32:.6f}; hip vs fp32 oracle {S.cosine(g_hip, g_o32):.6f}')
    assert np.isfinite(g_hip).all() and c_hip >= c_o32 - margin, (tag, c_hip, c_o32)


def _report(tag, xa, xb, la, lb, ga, gb, mask=None):
    """measured agreement, printed with -s (the bounds asserted below are ~3x these)"""
    d = np.abs(xa - xb).max(1) if mask is None else np.abs(xa[mask] - xb[mask]).max(1)
    print(f'MEASURED {tag}: |dx| median {np.median(d):.2e} p95 {np.quantile(d, 0.95):.2e} p99 {np.quantile(d, 0.99):.2e} max {d.max():.2e} '
          f'frac>1e-5 {np.mean(d > 1e-5):.4f} frac>1e-4 {np.mean(d > 1e-4):.4f} | loss rel {abs(la - lb) / abs(lb):.2e} | grad cos {S.cosine(ga, gb):.6f} relL2 {S.rel_l2(ga, gb):.3e}')


def test_icecream_dynamic_on_the_gpu(hiplib, oracle32):
    """IceCreamDynamic-v0 (BallInjector + Rigid cone SDF + plasto-elastic ICECREAM) at a reduced size, HIP vs oracle:
    recorded target and the action gradient of a drifted policy."""
    import test_host_env as H
    res = []
    for lib in (None, oracle32):
        env = H._icecream(lib, loss=False, max_substeps_local=None)
        tgt = Recorder(env).record(write=False)
        env = H._icecream(lib, target=tgt, max_substeps_local=None)
        cfg = load_config('configs/exp_icecream_dynamic.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        demo = env.demo_policy()
        pol.actions_v[:] = demo.actions_v; pol.actions_p[:] = demo.actions_p
        pol.actions_v[40:, 0] += 0.0004
        env.taichi_env.loss.temporal_range[1] = env.horizon
        info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], pol, env.horizon, env.horizon_action)
        res.append((tgt['x'][-1], tgt['used'][-1], info['loss'], g))
    (xa, ua, la, ga), (xb, ub, lb, gb) = res
    assert (ua == ub).all()
    m = ua > 0
    _report('icecream_dynamic', xa, xb, la, lb, ga, gb, m)
    # plasto-elastic contact: a few particles sit on branch edges (measured: 0.13 % beyond 1e-4, p99 1.9e-5, max 1.4e-4)
    d = np.abs(xa[m] - xb[m]).max(1)
    assert np.mean(d > 1e-4) <= 5e-3 and np.quantile(d, 0.99) <= 6e-5 and d.max() <= 1e-3
    # measured over repeated runs: 3e-5 .. 1e-4 (round 2's kernels: 3e-5 .. 4e-5), and 1.9e-2 in the one run in ~20 where a clump at the
    # cone takes the other contact branch; the scatter's slow path and shell hand-over are order-dependent fp32 atomics, like the reference's
    assert abs(la - lb) <= 3e-2 * abs(lb)
    assert S.cosine(ga, gb) >= 0.9999 and S.rel_l2(ga, gb) <= 1.5e-2         # measured 0.999998, 1.5e-3 .. 5.2e-3 (order of the fp32 sums)


def test_latteart_stir_on_the_gpu(hiplib, oracle32):
    """LatteArtStir-v0 (viscous two-liquid bath, Rigid rod, match-all loss) at a reduced size, HIP vs oracle."""
    import test_host_env as H
    res = []
    for lib in (None, oracle32):
        env = H._stir(lib, loss=False, max_substeps_local=None)
        tgt = Recorder(env).record(write=False)
        env = H._stir(lib, target=tgt, max_substeps_local=None)
        cfg = load_config('configs/exp_latteart_stir.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        demo = env.demo_policy()
        pol.actions_v[:] = demo.actions_v; pol.actions_p[:] = demo.actions_p
        pol.actions_v[8:, 2] += 0.001
        env.taichi_env.loss.temporal_range[1] = env.horizon
        info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], pol, env.horizon, env.horizon_action)
        res.append((tgt['x'][-1], info['loss'], info['loss_milk'], g))
    (xa, la, ma, ga), (xb, lb, mb, gb) = res
    _report('latteart_stir', xa, xb, la, lb, ga, gb)
    assert np.abs(xa - xb).max() <= 3e-6                                     # measured 8.9e-7
    assert abs(la - lb) <= 2e-4 * abs(lb) and abs(ma - mb) <= 2e-4 * abs(mb)  # measured 5.8e-5
    assert S.cosine(ga, gb) >= 0.99999 and S.rel_l2(ga, gb) <= 2e-3          # measured 1.000000, 6.9e-4


def test_icecream_static_on_the_gpu(hiplib, oracle32):
    """IceCreamStatic-v0 (controllable Injector over a static SDF cone) at a reduced size, HIP vs oracle."""
    import test_host_env as H
    res = []
    for lib in (None, oracle32):
        env = H._icecream_static(lib, loss=False, max_substeps_local=None)
        tgt = Recorder(env).record(write=False)
        env = H._icecream_static(lib, target=tgt, max_substeps_local=None)
        cfg = load_config('configs/exp_icecream_static.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        demo = env.demo_policy()
        pol.actions_v[:] = demo.actions_v; pol.actions_p[:] = demo.actions_p
        pol.actions_v[5:, 0] += 0.0005
        env.taichi_env.loss.temporal_range[1] = env.horizon
        info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], pol, env.horizon, env.horizon_action)
        res.append((tgt['x'][-1], tgt['used'][-1], info['loss'], g))
    (xa, ua, la, ga), (xb, ub, lb, gb) = res
    assert (ua == ub).all()
    m = ua > 0
    _report('icecream_static', xa, xb, la, lb, ga, gb, m)
    assert np.abs(xa[m] - xb[m]).max() <= 3e-6                               # measured 8.3e-7
    assert abs(la - lb) <= 1e-5 * abs(lb) and S.cosine(ga, gb) >= 0.999999 and S.rel_l2(ga, gb) <= 1e-5     # measured 3.1e-6, 2.5e-6


def test_gathering_easy_on_the_gpu(hiplib, oracle32, oracle64):
    """GatheringEasy-v0 (MAT_RIGID bodies in water pushed by a Rigid plate, host-side L1 loss through fe_add_grad), HIP vs oracle."""
    import test_host_env as H
    res = []
    for lib in (None, oracle32, oracle64):
        env = H._gathering(lib)
        cfg = load_config('configs/exp_gathering_easy.yaml').SOLVER
        pol = env.trainable_policy(cfg.optim, cfg.init_range)
        pol.actions_v[:, 0] = 0.003
        pol.actions_p[:] = [0.46, 0.42, 0.5]
        env.taichi_env.loss.temporal_range[1] = env.horizon
        info, g = Solver(env, None, cfg).forward_backward(env.taichi_env.get_state()['state'], pol, env.horizon, env.horizon_action)
        res.append((H._final_frame(env.taichi_env, env.horizon)['x'], info['loss'], g))
        if lib is None:                                  # a printed figure only: the plate's contacts of the last step that sit in the flat cell layer
            import contact_plate_cases as P
            sim = env.taichi_env.simulator
            last = range((env.horizon - 1) * sim.n_substeps, env.horizon * sim.n_substeps)
            flat, contacts = P.flat_cell_share(sim.engine, env.taichi_env.agent.effectors[0], last, sim.dt)
    (xa, la, ga), (xb, lb, gb), (xc, lc, gc) = res
    _report('gathering_easy', xa, xb, la, lb, ga, gb)
    d = np.abs(xa - xb).max(1)
    # the plate's soft contact flips branches for a few per cent of the water under fp32 rounding (measured: median 1.1e-6, 2.9 %
    # of the particles beyond 1e-4, max 1.7e-3)
    assert np.median(d) <= 5e-6 and np.mean(d > 1e-4) <= 0.08 and d.max() <= 6e-3
    assert abs(la - lb) <= 1e-4 * abs(lb)                                    # measured 1.2e-5
    # The action gradient of this scene runs through the plate's contact branches and the rigid bodies' SVD adjoint and is
    # ill-conditioned in fp32: the three implementations agree pairwise to cos 0.64 (hip / fp64 oracle), 0.80 (fp32 / fp64 oracle)
    # and 0.82 (hip / fp32 oracle) -- a handful of particles on the other side of a contact branch carry most of the difference.
    # (Not the flat cell layer of the plate's SDF, DESIGN.md: the share of the last step's plate contacts in it is printed below and measured 0 of 205.)
    # What is asserted is that the engine's gradient is finite and of the same family: no pair is far off the other two.
    c_ab, c_ac, c_bc = S.cosine(ga, gb), S.cosine(ga, gc), S.cosine(gb, gc)
    print(f'MEASURED gathering_easy: grad cos hip/fp32 {c_ab:.4f} hip/fp64 {c_ac:.4f} fp32/fp64 {c_bc:.4f}; plate contacts of the last step in the flat cell '
          f'layer: {flat} of {contacts} ({100.0 * flat / max(contacts, 1):.1f} %)')
    assert np.isfinite(ga).all() and c_ab >= 0.75 and c_ac >= c_bc - 0.25


def _both(hiplib_unused, oracle32, name, cfg_file, prepare, horizon, oracle64=None, **kw):
    """the same reduced environment through the Solver on the HIP engine and on the oracle (and on its fp64 build when given)"""
    import test_host_env as H
    res = []
    for lib in (None, oracle32) + ((oracle64,) if oracle64 is not None else ()):
        env = H._small(name, lib, horizon=horizon, **kw)
        if hasattr(env.taichi_env.loss, 'temporal_range'):
            env.taichi_env.loss.temporal_range[1] = env.horizon
        info, g, pol = H._solver_pass(env, cfg_file, prepare)
        fin = H._final_frame(env.taichi_env, horizon)
        res.append((fin['x'], fin['used'], info['loss'], g))
    return res


def test_pouring_on_the_gpu(hiplib, oracle32):
    """Pouring-v0 reduced (collide_type='both' + collector + PouringLoss), HIP vs oracle through the Solver."""
    def prepare(pol):
        pol.actions_v[:, 5] = 0.02
    (xa, ua, la, ga), (xb, ub, lb, gb) = _both(hiplib, oracle32, 'Pouring-v0', 'configs/exp_pouring.yaml', prepare, 10)
    _report('pouring', xa, xb, la, lb, ga[:, 5], gb[:, 5])
    assert (ua == ub).all()
    assert np.abs(xa - xb).max() <= 3e-6                                     # measured 8.9e-7
    assert abs(la - lb) <= 1e-5 * abs(lb)                                    # measured 7.4e-7
    # the glass' rotation gradient runs through the contact Jacobian with heavy cancellation: the oracle's own fp32 and fp64 builds
    # differ by 4.8e-3 here, two builds of the engine that differ only in instruction selection by 5e-3 (measured 1.5e-3 / 6.9e-3)
    assert np.isfinite(ga).all() and S.cosine(ga[:, 5], gb[:, 5]) >= 0.99999 and S.rel_l2(ga[:, 5], gb[:, 5]) <= 2e-2     # measured 0.999998, 6.9e-3


def test_transporting_on_the_gpu(hiplib, oracle32):
    """Transporting-v0 reduced (turning Injector + WATER collector + RIGID_HEAVY cube, z locked), HIP vs oracle."""
    def prepare(pol):
        pol.actions_p[:] = [0.42, 0.5, 0.5, 0.0, 0.0, 0.0]
        pol.actions_v[:, 5] = 0.002
    (xa, ua, la, ga), (xb, ub, lb, gb) = _both(hiplib, oracle32, 'Transporting-v0', 'configs/exp_transporting.yaml', prepare, 10,
                                               n_pool=400, particle_density=2e5)
    _report('transporting', xa, xb, la, lb, ga[:, [0, 5]], gb[:, [0, 5]])
    assert (ua == ub).all() and ua[:400].sum() == 400
    assert np.abs(xa - xb).max() <= 6e-6                                     # measured 1.8e-6
    assert abs(la - lb) <= 1e-5 * abs(lb)                                    # measured 1.8e-6
    assert np.isfinite(ga).all() and S.cosine(ga[:, [0, 5]], gb[:, [0, 5]]) >= 0.99999 and S.rel_l2(ga[:, [0, 5]], gb[:, [0, 5]]) <= 2e-3   # measured 1.000000, 4.6e-4


def test_mixing_on_the_gpu(hiplib, oracle32, oracle64):
    """Mixing-v0 reduced (viscous liquids, Rigid stirrer, pairwise-spread loss), HIP vs oracle."""
    def prepare(pol):
        pol.actions_p[:] = [0.5, 0.62, 0.5]
        pol.actions_v[:, 0] = 0.005
    (xa, ua, la, ga), (xb, ub, lb, gb), (xc, uc, lc, gc) = _both(hiplib, oracle32, 'Mixing-v0', 'configs/exp_mixing.yaml', prepare, 10, oracle64=oracle64)
    _report('mixing', xa, xb, la, lb, ga, gb)
    assert np.abs(xa - xb).max() <= 2e-6                                     # measured 4.8e-7
    assert abs(la - lb) <= 1e-5 * abs(lb)                                    # measured 1.7e-7
    # the gradient runs through the stirrer's contact and the viscous liquid's SVD adjoint: fp32 noise of ~14 % relL2 between the
    # two fp32 implementations (cos 0.995)
    assert S.cosine(ga, gb) >= 0.99
    _grad_no_worse_than_fp32_oracle('mixing', ga, gb, gc, 0.01)


def test_gathering_o_on_the_gpu(hiplib, oracle32, oracle64):
    """GatheringO-v0 reduced (static island in grid_op + Rigid plate + rigid bodies), HIP vs oracle."""
    def prepare(pol):
        pol.actions_v[:, 0] = 0.003
    (xa, ua, la, ga), (xb, ub, lb, gb), (xc, uc, lc, gc) = _both(hiplib, oracle32, 'GatheringO-v0', 'configs/exp_gatheringO.yaml', prepare, 12, oracle64=oracle64)
    _report('gathering_o', xa, xb, la, lb, ga, gb)
    # like the reference, the water block is sampled over the whole tank, island included (gatheringo_env.py:54-59); water
    # inside the island sits where the SDF normal flips between voxels, and takes different contact branches in two fp32
    # implementations: compare the water around it
    away = np.hypot(xb[:, 0] - 0.5, xb[:, 2] - 0.5) > 0.25
    assert away.sum() > 1500
    # ... and even there nodes on the island's surface flip between contact and free under rounding: the oracle's own f32 and f64
    # builds differ by 4.6e-3 at the 99th percentile of this scene (max 1.6e-2, action-gradient cosine 0.977)
    d = np.abs(xa - xb).max(1)
    # measured: median 5.4e-7, 1.6 % of the particles beyond 1e-4 (the flipped ones), max 1.1e-3
    assert np.median(d) <= 2e-6 and np.mean(d > 1e-4) <= 0.05 and np.quantile(d[away], 0.99) <= 5e-4 and d.max() <= 4e-3
    assert abs(la - lb) <= 1e-6 * abs(lb)                                    # measured 2.6e-8
    assert S.cosine(ga, gb) >= 0.97                                          # measured 0.9899
    _grad_no_worse_than_fp32_oracle('gathering_o', ga, gb, gc, 0.02)


def test_env_batch_on_the_gpu(hiplib):
    """The same on the HIP engine, where the batch really shares launches (gridDim.y = 2): each replica within fp32 atomics noise of
    the run it makes alone."""
    import test_host_env as H
    env = H.make('LatteArt-v0', seed=0, loss=False, engine_lib=hiplib, **H.MINI)
    tgt = Recorder(env).record(write=False)
    single, batch = H._batch_vs_single(hiplib, tgt)
    for (ia, ga), (ib, gb) in zip(single, batch):
        assert abs(ia['loss'] - ib['loss']) <= 1e-5 * abs(ia['loss'])
        assert S.cosine(ga, gb) >= 0.999999 and S.rel_l2(ga, gb) <= 1e-4
