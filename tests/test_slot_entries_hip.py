"""GPU: the C entries that read or write a frame or an adjoint ring slot from outside the substep drivers, all behind the engine's two host
accessors (fe_engine.hip: frame_written, adj_slot).

Scene: a moving block of water at 32^3, 4,000 particles (10 % unused), sort_interval = 4, a window of 16 substeps.

1. Every adjoint entry refuses a slot whose x, v, C a fused fe_step_grad kept in registers: the same message, the slot's order and the
   neighbouring slot's words untouched.
2. On a cleared slot a read returns zeros and leaves the slot cleared; every accumulating entry gives it the order of its frame (a frame
   behind a sort, so that the order is not the identity).
3. A frame with pre-counted sort keys is overwritten through fe_set_frame, fe_set_frame_dev and fe_copy_frame and stepped on across the next
   sort: the result is that of a fresh engine given the same state, within the run-to-run bound of tests/test_hip_parity.py
   (test_sort_keys_counted_in_g2p: four times the difference of two identical runs plus a few ulp of the field's range)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import AXIS_Y, AXIS_Z, SQ_CONST, DensityField, Sel, Term  # noqa: E402

pytestmark = pytest.mark.gpu
N = 4000
K = 4
L = 16
MSG = ("this frame's adjoint was passed on in registers inside a fused fe_step_grad call and is not in memory (after fe_step_grad(f0, n) only the "
       "adjoint of frame f0 is defined; option fuse_bwd = 0 keeps every frame's)")
OBS_IDS = [5, 17, 5, 900]
FIELD = DensityField((0.2, 0.2, 0.2), (0.1, 0.1, 0.1), (6, 6, 6))


def _scene():
    rng = np.random.RandomState(5)
    sc = S.water_block(n_grid=32, n_particles=N, seed=3, lo=0.3, hi=0.6)
    sc['v'] = S.f32(rng.normal(0, 1.0, (N, 3)) + [2.0, -3.0, 1.0])
    sc['used'] = (rng.rand(N) > 0.1).astype(np.int32)
    return sc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(eng, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=f'cuda:{eng.device}')


COT = S.random_cotangent(N, seed=2)
ROWS = S.f32(np.random.RandomState(6).normal(size=(len(OBS_IDS), 3)))
G = np.random.RandomState(7).uniform(-1, 1, (4,) + FIELD.n).astype(np.float32)

# the ten entries: name -> (call on frame f, accumulates into the slot)
ENTRIES = {
    'fe_copy_grad': (lambda e, f: e.copy_grad(f, f + 1), False),
    'fe_get_grad': (lambda e, f: e.get_grad(f), False),
    'fe_add_grad': (lambda e, f: e.add_grad(f, gx=COT['gx']), True),
    'fe_add_grad_dev': (lambda e, f: e.add_grad_dev(f, gx=_dev(e, COT['gx'])), True),
    'fe_loss_step_grad': (lambda e, f: e.loss_step_grad(0, f, S.WATER, 1.0, 1.0), True),
    'fe_task_loss_step_grad': (lambda e, f: e.task_loss_step_grad(0, f, 1.0), True),
    'fe_obs_add_grad': (lambda e, f: e.obs_add_grad(f, gx=ROWS, gv=ROWS), True),
    'fe_obs_add_grad_dev': (lambda e, f: e.obs_add_grad_dev(f, gx=_dev(e, ROWS)), True),
    'fe_field_obs_add_grad': (lambda e, f: e.field_obs_add_grad(f, 0, G), True),
    'fe_field_obs_add_grad_dev': (lambda e, f: e.field_obs_add_grad(f, 0, _dev(e, G)), True),
}
ADDING = [n for n, (_, adds) in ENTRIES.items() if adds]


@pytest.fixture(scope='module')
def eng(hiplib):
    """one rollout over the window, with everything the ten entries need set up; the tests only touch the adjoint ring"""
    sc = _scene()
    e = S.make_engine(hiplib, sc, max_substeps_local=L, options={'sort_interval': K, 'fuse_bwd': 1})
    e.loss_alloc(1)
    e.loss_set_target(0, sc['x'])
    e.task_loss_alloc(1)
    e.task_loss_set_terms([Term(SQ_CONST, AXIS_Y | AXIS_Z, Sel(0, 900), c=(0.0, 0.3, 0.4), weight=0.7)])
    e.obs_set_particles(OBS_IDS)
    e.field_obs_set(0, FIELD, Sel(0, N, -1, True), 4)
    e.step(0, 0, 12, 0)
    yield e
    e.close()


@pytest.mark.parametrize('name', list(ENTRIES))
def test_incomplete_slot_is_refused_by_every_entry(eng, name):
    """the arrangement of test_incomplete_adjoint_slots_are_refused, inside one particle order: fe_step_grad(4, 4) runs frames 7 .. 4 fused,
    frame 5's slot keeps only F's adjoint"""
    call, _ = ENTRIES[name]
    eng.reset_grad()
    eng.add_grad(8, COT['gx'], COT['gv'], COT['gC'], COT['gF'])
    eng.step_grad(4, 4, 4, 0)
    first = eng.get_grad(4)                                   # the call's first frame: defined
    assert np.abs(first[0]).max() > 0
    order = eng.get_option('table_of_grad_5')
    with pytest.raises(_capi.FeEngineError) as err:
        call(eng, 5)
    assert str(err.value) == MSG and eng.lib.fe_last_error(eng.h) == MSG.encode()
    assert eng.get_option('table_of_grad_5') == order
    for a, b in zip(first, eng.get_grad(4)):
        assert np.array_equal(_bits(a), _bits(b))
    call(eng, 4)                                              # ... and the same call is taken on the frame next to it


def test_read_of_a_cleared_slot(eng):
    f = 8
    tf = eng.get_option(f'table_of_frame_{f}')
    assert tf > 0                                             # behind the sort at 8: not the identity order
    eng.reset_grad()
    assert eng.get_option(f'table_of_grad_{f}') == -1
    for g in eng.get_grad(f):
        assert not g.any()
    assert eng.get_option(f'table_of_grad_{f}') == -1         # a read assigns no order
    eng.copy_grad(f, f + 1)                                   # ... nor does the source side of a copy; the copy is a cleared slot too
    assert eng.get_option(f'table_of_grad_{f}') == -1 and eng.get_option(f'table_of_grad_{f + 1}') == -1


@pytest.mark.parametrize('name', ADDING)
def test_accumulating_entry_gives_a_cleared_slot_its_frames_order(eng, name):
    f = 8
    tf = eng.get_option(f'table_of_frame_{f}')
    assert tf > 0
    eng.reset_grad()
    ENTRIES[name][0](eng, f)
    assert eng.get_option(f'table_of_grad_{f}') == tf
    gx = eng.get_grad(f)[0]
    assert gx.any() and eng.get_option(f'table_of_grad_{f}') == tf
    if name.startswith('fe_add_grad'):                        # 0 + gx, particle by particle: the words went to the slots of the frame's order
        assert np.array_equal(_bits(gx), _bits(COT['gx']))


def _edited(st):
    """a different, valid state on the same particles: every seventh one moved by three and a half cells"""
    x = st['x'].copy()
    x[::7] += np.float32(0.11)
    return dict(st, x=np.clip(x, 0.1, 0.9).astype(np.float32))


def _fresh_run(hiplib, sc, st, n):
    e = S.make_engine(hiplib, sc, max_substeps_local=L, options={'sort_interval': K})
    e.set_frame(0, x=st['x'], v=st['v'], C_=st['C'], F=st['F'], used=st['used'])
    e.step(0, 0, n, 0)
    out = S.get_state(e, n)
    e.sync()
    e.close()
    return out


def _assert_run_to_run(a, b, c, what):
    """tests/test_hip_parity.py, test_sort_keys_counted_in_g2p: a against b, where c is b once more"""
    assert (a['used'] == b['used']).all(), what
    u = b['used'] > 0
    for k in 'xvCF':
        scale = max(1.0, float(np.abs(b[k][u]).max()))
        d, nz = float(np.abs(a[k][u] - b[k][u]).max()) / scale, float(np.abs(c[k][u] - b[k][u]).max()) / scale
        print(f'MEASURED frame written by {what}: {k} differs by {d:.3g} of its range, two fresh engines by {nz:.3g}')
        assert d <= 4.0 * nz + {'x': 5e-7, 'v': 4e-6, 'C': 8e-5, 'F': 4e-6}[k], (what, k, d, nz)


@pytest.fixture(scope='module')
def edit_case(hiplib):
    """the state fe_set_frame* write over frame 8, and two fresh engines stepped six substeps from it (sorts at 0 and 4)"""
    sc = _scene()
    e = S.make_engine(hiplib, sc, max_substeps_local=L, options={'sort_interval': K})
    e.step(0, 0, 8, 0)
    st = _edited(S.get_state(e, 8))
    e.close()
    return sc, st, _fresh_run(hiplib, sc, st, 6), _fresh_run(hiplib, sc, st, 6)


@pytest.mark.parametrize('entry', ['fe_set_frame', 'fe_set_frame_dev'])
def test_set_frame_over_precounted_keys(hiplib, edit_case, entry):
    """substep 7 counted the keys of the sort at frame 8 (k_g2p_sortkey); the frame is then replaced and stepped across the sorts at 8 and 12"""
    sc, st, b, c = edit_case
    e = S.make_engine(hiplib, sc, max_substeps_local=L, options={'sort_interval': K})
    assert e.get_option('sort_keys_in_g2p') == 1
    e.step(0, 0, 8, 0)
    if entry == 'fe_set_frame':
        e.set_frame(8, x=st['x'], v=st['v'], C_=st['C'], F=st['F'], used=st['used'])
    else:
        e.set_frame_dev(8, x=_dev(e, st['x']), v=_dev(e, st['v']), C_=_dev(e, st['C']), F=_dev(e, st['F']), used=_dev(e, st['used']))
    e.step(8, 8, 6, 0)
    a = S.get_state(e, 14)
    e.sync()
    e.close()
    _assert_run_to_run(a, b, c, entry)


def test_copy_frame_wraps_the_window(hiplib):
    """fluidlab's window wrap: the last frame of the window, with the keys substep 15 counted for it, becomes frame 0 and is sorted there"""
    sc = _scene()
    e = S.make_engine(hiplib, sc, max_substeps_local=L, options={'sort_interval': K})
    e.step(0, 0, L, 0)
    st = S.get_state(e, L)
    assert np.abs(st['x'] - sc['x']).max() > 1e-3             # not what frame 0 held
    e.copy_frame(L, 0)
    e.step(0, 0, 6, 0)
    a = S.get_state(e, 6)
    e.sync()
    e.close()
    _assert_run_to_run(a, _fresh_run(hiplib, sc, st, 6), _fresh_run(hiplib, sc, st, 6), 'fe_copy_frame')
