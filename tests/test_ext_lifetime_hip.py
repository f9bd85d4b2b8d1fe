"""GPU: the lifetime of the state behind the observation gather, the frame summary, the loss-term programs, the density fields and the target
clouds (csrc/fe_summary.h, fe_task_loss.h, fe_density.h, fe_nearest.h): each keeps one struct behind one pointer of the engine, allocated at
first use and freed by fe_destroy.

(a) an engine on which none of them was ever called; the entries called before any set-up answer with the return codes and messages recorded
    from the build before the state moved out of the engine struct (EARLY), and leave fe_last_error as that build did;
(b) an engine that used all four, destroyed, and a second one created afterwards: the same calls give the same bits;
(c) buffers that grow -- a field re-set to more cells, a cloud replaced by a larger one, more pair chunks -- give the bits of an engine that had
    the final sizes from the start.

The substep itself does not repeat bit for bit between two engines (the sort ranks the particles of a cell with returning
atomics), and the separable terms and the summary add in slot order.  So (b) pins what the calls read: both engines roll out on their own, sorts
included, and then evaluate on a frame beyond the rollout -- identity order -- that holds the first engine's final state, word for word.  (c)
evaluates on frame 0 as uploaded.  Every comparison is of bits; there is no tolerance in this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402
from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import (AXIS_ALL, AXIS_X, AXIS_Y, COVER_SQ, DENSITY_SQ, L1_CONST, NEAREST_SQ, PAIR_L1,  # noqa: E402
                                                          DensityField, Sel, Term)

pytestmark = pytest.mark.gpu
N = 1500
F_END, F_EVAL = 12, 20                                       # the rollout's last frame (sorts at 0 and 10); a frame no substep writes

NO_LIST = 'no observation list: fe_obs_set_particles first'
NO_PROGRAM = 'no loss-term program: fe_task_loss_set_terms first'
NO_ARRAYS = 'no task-loss arrays: fe_task_loss_alloc first'
NO_FIELD = 'fe_density_get: the field is not set: fe_density_set_field first'
NO_CLOUD = 'fe_cloud_query: the cloud is not set: fe_cloud_set first'
BAD_SIZE = 'fe_frame_summary: record_size is not sizeof(FeFrameSummary)'
# (call, return code, fe_last_error afterwards): a call that succeeds leaves the message of the last refusal in place
EARLY = [
    ('fe_obs_get', 1, NO_LIST),
    ('fe_obs_get_dev', 1, NO_LIST),
    ('fe_obs_add_grad', 1, NO_LIST),
    ('fe_frame_summary 1 record', 0, NO_LIST),
    ('fe_frame_summary 3 records, no groups', 0, NO_LIST),
    ('fe_frame_summary record_size', 1, BAD_SIZE),
    ('fe_task_loss_step', 1, NO_PROGRAM),
    ('fe_task_loss_step_grad', 1, NO_PROGRAM),
    ('fe_task_loss_get', 1, NO_ARRAYS),
    ('fe_task_loss_clear', 0, NO_ARRAYS),
    ('fe_density_get', 1, NO_FIELD),
    ('fe_cloud_query', 1, NO_CLOUD),
    ('fe_cloud_set removal', 0, NO_CLOUD),
    ('fe_summary_set_groups', 0, NO_CLOUD),
    ('fe_frame_summary 3 records, 2 groups', 0, NO_CLOUD),
]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        p, q = np.asarray(a[k]), np.asarray(b[k])
        assert p.shape == q.shape and p.dtype == q.dtype and np.array_equal(_bits(p), _bits(q)), f'{tag}: {k} differs'


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def early_calls(hiplib):
    """The entries of the four subsystems on an engine that was created and stepped once and has seen no extension call, in the order of EARLY:
    [(call, return code, fe_last_error afterwards)], and the summary records the three successful summary calls wrote."""
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=N))
    eng.step(0, 0, 1, 0)
    lib, h = eng.lib, eng.h
    assert lib.fe_last_error(h) == b''
    log, recs = [], []
    x, v, u = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), np.zeros(1, np.int32)
    out8, nn, d2 = np.zeros(8, np.float64), np.zeros(N, np.int32), np.zeros(N, np.float64)
    size = C.sizeof(_capi.FeFrameSummary)

    def note(name, rc):
        log.append((name, int(rc), lib.fe_last_error(h).decode()))

    def summary(name, n_records, record_size=size):
        rec = (_capi.FeFrameSummary * 3)()
        for r in rec:
            r.n_used = -7
        note(name, lib.fe_frame_summary(h, 1, C.byref(rec), n_records, record_size))
        recs.append([int(r.n_used) for r in rec])

    note('fe_obs_get', lib.fe_obs_get(h, 1, _ptr(x), _ptr(v), _ptr(u)))
    note('fe_obs_get_dev', lib.fe_obs_get_dev(h, 1, None, None, None))
    note('fe_obs_add_grad', lib.fe_obs_add_grad(h, 1, _ptr(x), _ptr(v)))
    summary('fe_frame_summary 1 record', 1)
    summary('fe_frame_summary 3 records, no groups', 3)
    summary('fe_frame_summary record_size', 1, size - 8)
    note('fe_task_loss_step', lib.fe_task_loss_step(h, 0, 1))
    note('fe_task_loss_step_grad', lib.fe_task_loss_step_grad(h, 0, 1, C.c_double(1.0)))
    note('fe_task_loss_get', lib.fe_task_loss_get(h, 0, 1, _ptr(out8), None))
    note('fe_task_loss_clear', lib.fe_task_loss_clear(h))
    note('fe_density_get', lib.fe_density_get(h, 1, 0, None, _ptr(out8), C.c_longlong(8)))
    note('fe_cloud_query', lib.fe_cloud_query(h, 1, 0, None, 7, _ptr(nn), _ptr(d2), None, None))
    note('fe_cloud_set removal', lib.fe_cloud_set(h, 0, None, 0))
    group = (np.arange(N) % 2).astype(np.int32)
    note('fe_summary_set_groups', lib.fe_summary_set_groups(h, _ptr(group), 2))
    summary('fe_frame_summary 3 records, 2 groups', 3)
    eng.sync()
    eng.close()
    return log, recs


def test_a_plain_engine_is_created_stepped_and_destroyed(hiplib):
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=N))
    eng.step(0, 0, 1, 0)
    eng.sync()
    eng.close()


def test_entries_before_any_set_up_answer_as_ever(hiplib):
    log, recs = early_calls(hiplib)
    for got, want in zip(log, EARLY):
        print(got)
        assert got == want
    assert len(log) == len(EARLY)
    # the summaries that succeeded: one whole-frame record without groups however many were asked for, nothing written by the refused call
    assert recs == [[N, -7, -7], [N, -7, -7], [-7, -7, -7], [N // 2, N // 2, N]]


# ---- (b), (c): the same calls on two engines
FIELD_SMALL = DensityField(origin=(0.25, 0.25, 0.25), cell=(0.12, 0.12, 0.12), n=(3, 3, 3))
FIELD = DensityField(origin=(0.25, 0.25, 0.25), cell=(0.04, 0.05, 0.07), n=(9, 7, 5))
ALL_USED = Sel(0, N, -1, True)


def _cloud(n, seed):
    return (0.28 + 0.3 * np.random.RandomState(seed).rand(n, 3)).astype(np.float32)


def _target(field, seed):
    return 3.0 * np.random.RandomState(seed).rand(*field.shape)


def _terms(extra_cover):
    t = [Term(L1_CONST, AXIS_X | AXIS_Y, ALL_USED, c=(0.4, 0.35, 0.0), weight=1.3),
         Term(PAIR_L1, AXIS_ALL, Sel(0, 700), b=Sel(700, N), weight=0.01),
         Term(DENSITY_SQ, AXIS_ALL, ALL_USED, weight=0.5, field=1),
         Term(NEAREST_SQ, AXIS_ALL, Sel(100, 1400, -1, True), weight=0.7, cloud=2)]
    return t + ([Term(COVER_SQ, AXIS_X | AXIS_Y, ALL_USED, weight=0.2, cloud=2)] if extra_cover else [])


def _evaluate(eng, f, step):
    """the program forward and backward on frame f into loss step `step`, a density field, a cloud query, the summary, the gather"""
    eng.task_loss_step(step, f)
    eng.reset_grad()
    eng.task_loss_step_grad(step, f, 0.37)
    sl, tl = eng.task_loss_get(1, s0=step, terms=True)
    out = {'step_loss': sl, 'term_loss': tl, 'gx': eng.get_grad(f)[0], 'density': eng.density_field(f, 1, Sel(0, 900))}
    out.update(zip(('nn_p', 'd2_p', 'nn_c', 'd2_c'), eng.cloud_query(f, 2, Sel(50, 1450, -1, True), AXIS_ALL)))
    for g, r in enumerate(eng.frame_summary(f)):
        out.update({f'summary {g} {k}': np.asarray(val) for k, val in r.items()})
    out.update({f'obs {k}': val for k, val in eng.get_obs(f).items()})
    assert np.all(np.isfinite(sl)) and np.all(tl != 0) and np.any(out['gx'] != 0) and out['density'].sum() > 0 and (out['nn_p'] >= 0).sum() > 1000
    return out


def _rollout(hiplib, state=None):
    """an engine that uses all four subsystems over a short rollout; `state`: what frame F_EVAL is to hold (None: this engine's frame F_END)"""
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=N), max_substeps_local=32)
    assert eng.get_option('sort_interval') == 10
    eng.obs_set_particles(np.concatenate([[0, N - 1, 7, 7], np.random.RandomState(1).randint(0, N, 96)]).astype(np.int32))
    eng.summary_set_groups((np.arange(N) % 3).astype(np.int32), 3)
    eng.density_set_field(1, FIELD)
    eng.density_set_target(1, _target(FIELD, 4))
    eng.cloud_set(2, _cloud(300, 5))
    eng.task_loss_alloc(2)
    eng.task_loss_set_terms(_terms(False))
    for f0 in (0, 6):                                         # the calls inside the rollout, on its own frames: sorted orders, compact F
        eng.step(f0, f0, 6, 0)
        eng.task_loss_step(0, f0 + 6)
        eng.task_loss_step_grad(0, f0 + 6, 1.0)
        assert eng.frame_summary(f0 + 6)[3]['n_used'] == N and len(eng.get_obs(f0 + 3)['x']) == 100
        eng.cloud_query(f0 + 6, 2)
    eng.sync()
    if state is None:
        state = S.get_state(eng, F_END)
    eng.set_frame(F_EVAL, state['x'], state['v'], state['C'], state['F'], state['used'])
    out = _evaluate(eng, F_EVAL, 1)
    eng.sync()
    eng.close()
    return out, state


def test_a_second_engine_after_the_first_was_destroyed_gives_the_same_bits(hiplib):
    first, state = _rollout(hiplib)
    assert not np.array_equal(state['x'], S.water_block(n_grid=16, n_particles=N)['x'])
    second, _ = _rollout(hiplib, state)
    _same(first, second, 'second engine')
    third, _ = _rollout(hiplib, state)                        # ... and once more, into whatever the second one's buffers left behind
    _same(first, third, 'third engine')


def _grown(hiplib, grow):
    """frame 0 of the block through the program, a field and a query; grow: every buffer starts small and is re-set to the final size"""
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=N))
    eng.obs_set_particles(np.arange(0, N, 15, dtype=np.int32))
    eng.task_loss_alloc(2)
    if grow:
        eng.set_option('task_pair_chunk', 1024)               # 3 workgroup partials of the pair term; 39 with chunks of 64
        eng.density_set_field(1, FIELD_SMALL)                 # 27 cells; 315 in the end
        eng.density_set_target(1, _target(FIELD_SMALL, 3))
        eng.cloud_set(2, _cloud(40, 6))                       # 40 points; in the end more than N, the size the result buffers start with
        eng.task_loss_set_terms(_terms(True))
        small = _evaluate(eng, 0, 0)
        assert small['density'].shape == (3, 3, 3) and small['nn_c'].shape == (40,)
    eng.set_option('task_pair_chunk', 64)
    eng.density_set_field(1, FIELD)
    eng.density_set_target(1, _target(FIELD, 4))
    eng.cloud_set(2, _cloud(N + 200, 5))
    eng.task_loss_set_terms(_terms(True))
    out = _evaluate(eng, 0, 1)
    assert out['density'].shape == (9, 7, 5) and out['nn_c'].shape == (N + 200,)
    eng.sync()
    eng.close()
    return out


def test_grown_buffers_give_the_bits_of_a_fresh_engine(hiplib):
    _same(_grown(hiplib, True), _grown(hiplib, False), 'grown')
