"""Density fields are HIP-engine extensions (include/fluidengine_ext.h): the HIP library exports their three names, the ctypes mirror of
FeDensitySpec has the layout of the C struct and FeLossTerm keeps its 72 bytes, an oracle engine and an oracle-backed environment refuse
the new calls, and DensityMatchingLoss's host path -- the fp64 interpreter on downloaded frames -- runs against the oracle.  No GPU needed."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from fluidlab_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(__file__))

NAMES = ['fe_density_set_field', 'fe_density_set_target', 'fe_density_get']


def test_hip_library_exports_the_three_names():
    if not os.path.exists(_capi.HIP_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _capi.load_hip()
    assert set(NAMES) <= set(_capi.EXT_SYMBOLS)
    assert [s for s in NAMES if not hasattr(lib.lib, s)] == []
    assert lib.has_ext and lib.missing_symbols() == []
    assert not set(NAMES) & set(_capi.ABI_SYMBOLS)


def test_ctypes_spec_has_the_layout_of_the_c_struct(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or ('/opt/rocm/llvm/bin/clang' if os.path.exists('/opt/rocm/llvm/bin/clang') else None)
    if cc is None:
        pytest.skip('no C compiler')
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fluidengine_ext.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(FeDensitySpec), offsetof(FeDensitySpec, cell), offsetof(FeDensitySpec, n),\n'
                   '    offsetof(FeDensitySpec, pad), sizeof(FeLossTerm), FE_DENSITY_MAX_FIELDS, FE_DENSITY_MAX_CELLS, FE_DENSITY_LDS_CELLS, FE_TASK_LOSS_MAX_DENSITY_TERMS,\n'
                   '    FE_TERM_DENSITY_SQ); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(t) for t in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    size, off_cell, off_n, off_pad, term_size = out[:5]
    S = _capi.FeDensitySpec
    assert ctypes.sizeof(S) == size == 64 and S.cell.offset == off_cell == 24 and S.n.offset == off_n == 48 and S.pad.offset == off_pad == 60
    assert ctypes.sizeof(_capi.FeLossTerm) == term_size == 72
    assert out[5:] == [_capi.FE_DENSITY_MAX_FIELDS, _capi.FE_DENSITY_MAX_CELLS, _capi.FE_DENSITY_LDS_CELLS, _capi.FE_TASK_LOSS_MAX_DENSITY_TERMS,
                       _capi.FE_TERM_DENSITY_SQ] == [2, 1 << 21, 8192, 2, 4]


def test_new_engine_methods_raise_on_an_oracle_engine(oracle64):
    import scenarios as S
    from fluidlab_amd.fluidengine.losses.term_program import DensityField
    eng = S.make_engine(oracle64, S.water_block(n_grid=8, n_particles=8))
    spec = DensityField((0, 0, 0), (0.1, 1, 0.1), (8, 1, 8))
    calls = [lambda: eng.density_set_field(0, spec), lambda: eng.density_set_field(0, None), lambda: eng.density_set_target(0, np.zeros((8, 1, 8))),
             lambda: eng.density_field(0)]
    for call in calls:
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    eng.close()


@pytest.fixture(scope='module')
def latte(oracle64):
    """a small LatteArt with the density loss on the fp64 oracle, rolled out for its four steps; the target is a point cloud of another size"""
    import test_host_env as H
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, loss_type='density', n_pool=300)
    te = env.taichi_env
    loss = te.loss
    rng = np.random.RandomState(5)
    cloud = np.stack([rng.uniform(0.3, 0.7, 777), rng.uniform(0.5, 0.9, 777), rng.uniform(0.35, 0.65, 777)], axis=1)
    loss.set_target_points(cloud)
    pol = env.demo_policy()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    frames = []
    for i in range(env.horizon):
        te.step(pol.get_action_v(i, agent=te.agent, update=True))
        frames.append((te.simulator.cur_step_global - 1, te.simulator.cur_substep_local))
    return env, cloud, frames


def test_density_loss_on_the_oracle_matches_the_interpreter(latte):
    from fluidlab_amd.configs.macros import MILK
    from fluidlab_amd.fluidengine.losses import DensityMatchingLoss
    from fluidlab_amd.fluidengine.losses.term_program import density_of_points, eval_terms_numpy
    env, cloud, frames = latte
    te = env.taichi_env
    loss, sim = te.loss, te.simulator
    assert isinstance(loss, DensityMatchingLoss) and loss.matching_mat == MILK and loss.field.shape == (64, 1, 64)
    assert loss.temporal_range == [env.horizon - 1, env.horizon] and not loss._device_loss
    assert abs(loss.target.sum() - len(cloud)) <= 1e-9 * len(cloud)              # the whole cloud lies inside the cup's field
    terms = loss.device_terms()
    assert len(terms) == 1 and terms[0].a.require_used
    mat = sim.particles_i.mat.to_numpy()
    want = []
    for s, f in frames:
        x = np.zeros((sim.n_particles, 3), np.float64)
        used = np.zeros((sim.n_particles,), np.int32)
        sim.engine.get_frame(f, x=x, used=used)
        vals, _ = eval_terms_numpy(terms, x, used, mat, fields={0: loss.field}, targets={0: loss.target})
        want.append(vals[0])
        if s == frames[-1][0]:
            milk = (used != 0) & (mat == MILK)
            assert milk.sum() > 0
            D = density_of_points(x[milk], loss.field)
            assert abs(((D - loss.target) ** 2).sum() - vals[0]) <= 1e-12 * vals[0]
    got = np.asarray(loss.step_loss, np.float64)
    print(f'step_loss {got!r} interpreter {np.array(want)!r}')
    assert np.all(np.array(want) > 0) and np.array_equal(got, np.array(want))
    info = te.get_final_loss()
    assert info['loss'] == want[-1]                                               # temporal range 'last'
    # the host gradient reaches the engine's adjoint: the milk of the last frame, x and z only (y is projected)
    sim.engine.reset_grad()
    loss.compute_step_loss_grad(*frames[-1])
    g = sim.engine.get_grad(frames[-1][1])[0]
    assert np.abs(g[:, [0, 2]]).max() > 0 and np.all(g[:, 1] == 0) and np.all(g[mat != MILK] == 0)


def test_oracle_backed_env_refuses_the_device_calls(latte):
    env, _, _ = latte
    te = env.taichi_env
    for call in (env.enable_device_loss, te.enable_device_loss, te.loss.enable_device_loss, lambda: te.density_field(), lambda: te.simulator.density_field(0, te.loss.field)):
        with pytest.raises(_capi.FeEngineError, match='not available on oracle-f64'):
            call()
    assert not te.loss._device_loss


def test_latteart_diff_is_unchanged_and_density_builds_empty(oracle64):
    import test_host_env as H
    from fluidlab_amd.fluidengine.losses import DensityMatchingLoss, LatteArtLoss
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300)
    assert type(env.taichi_env.loss) is LatteArtLoss and env.loss_type == 'diff'
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300, loss_type='density')
    assert type(env.taichi_env.loss) is DensityMatchingLoss and env.taichi_env.loss.target is None
    target = np.arange(64 * 64, dtype=np.float64).reshape(64, 64)
    env = H._small('LatteArt-v0', oracle64, horizon=4, horizon_action=4, n_pool=300, loss_type='density', target=target)
    assert np.array_equal(env.taichi_env.loss.target, target.reshape(64, 1, 64))
