"""GPU: fe_smoke_cells_add_grad* (fluidlab_amd/csrc/fe_smoke_reads.h) against the dense road bit for bit, and its refusals.

Raw ABI on the res-12 smoke cases of tests/smoke_cases.py ('base': q_dim 1, 'q3': q_dim 3), a smoke ring of frames 0 .. 4.  The expected bits
are before + D at the listed cells, with D the rows added in list order on an fp32 zero field (np.add.at), and `before` everywhere else: a
cell the list does not name is not written (fe_smoke_add_grad of the dense field adds +0 there, which turns a -0 into +0)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402
import smoke_cases as SC  # noqa: E402

from fluidlab_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
RES, RING = 12, 4                                                # frames 0 .. RING
FRAMES = (0, 2, RING)                                            # the first, a middle one, s = max_steps_local
SCRATCH = 3                                                      # a frame no case scatters into: the copy the _dev variant works on


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _lists():
    """name -> cells [n, 3]: one cell; 97 rows over 92 distinct cells (three named twice, one three times), shuffled; 300 rows -- more than
    one workgroup of distinct cells -- with one cell named five times"""
    rng = np.random.RandomState(11)
    pick = lambda n: np.stack(np.unravel_index(rng.choice(RES ** 3, n, replace=False), (RES,) * 3), axis=1).astype(np.int32)
    c92 = pick(92)
    c97 = np.concatenate([c92, c92[[3, 40, 91]], c92[[17, 17]]])
    c97 = c97[rng.permutation(97)]
    c296 = pick(296)
    c300 = np.concatenate([c296, c296[[100] * 4]])[rng.permutation(300)]
    out = {'n1': np.array([[RES - 1, 0, 5]], np.int32), 'n97': c97, 'n300': c300}
    assert len(np.unique(c97, axis=0)) == 92 and len(np.unique(c300, axis=0)) == 296 > 256
    return out


LISTS = _lists()


def _dense(cells, rows, comps):
    """what the dense road uploads: the rows added in list order on an fp32 zero field"""
    D = np.zeros((RES, RES, RES, comps), np.float32)
    np.add.at(D, (cells[:, 0], cells[:, 1], cells[:, 2]), rows)
    return D


def _all_grads(eng):
    return [eng.smoke_get_grad(s) for s in range(RING + 1)]


def _all_fields(eng):
    return [eng.smoke_get_frame(s, ('v', 'q')) for s in range(RING + 1)]


@pytest.fixture(scope='module', params=['base', 'q3'])
def field(hiplib, request):
    """an engine two smoke steps into a rollout, its adjoint cleared"""
    case = SC.CASES[request.param]
    eng, e = SC.make_engine(hiplib, case, action_steps=RING)
    acts = SC.actions(2)
    for s in range(2):
        eng.eff_set_action(e, s, s, 2, acts[s])
        eng.smoke_step(s, 2 * s)
        eng.step(2 * s, 2 * s, 2, 1)
    eng.reset_grad()
    eng.smoke_reset_grad()
    yield dict(eng=eng, e=e, qd=case['q_dim'], case=case)
    eng.close()


def _occupy(f):
    """a loss seeded on frame 2 and two smoke_step_grad: the adjoints of frames 0, 1 and 2 are in use"""
    eng, qd = f['eng'], f['qd']
    rng = np.random.RandomState(5)
    eng.reset_grad()
    eng.smoke_reset_grad()
    eng.smoke_add_grad(2, gv=rng.normal(size=(RES, RES, RES, 3)).astype(np.float32), gq=rng.normal(size=(RES, RES, RES, qd)).astype(np.float32))
    for s in (1, 0):
        eng.step_grad(2 * s, 2 * s, 2, 1)
        eng.smoke_step_grad(s, 2 * s)
    gv0, gq0 = eng.smoke_get_grad(0)
    assert np.count_nonzero(gv0) > 0 and np.count_nonzero(gq0) > 0


def _check_scatter(f, name, s, variant, rng):
    """one call on frame s; the expected bits are before + D at the listed cells and `before` everywhere else"""
    import torch
    eng, qd = f['eng'], f['qd']
    cells = LISTS[name]
    n = len(cells)
    rv, rq = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, qd)).astype(np.float32)
    use_v, use_q = variant != 'gq-only', variant != 'gv-only'
    before, fields = _all_grads(eng), _all_fields(eng)
    if variant == 'dev':
        tv, tq = torch.from_numpy(rv).to('cuda:0'), torch.from_numpy(rq).to('cuda:0')
        eng.smoke_cells_add_grad(0, s, gv=tv, gq=tq)
        eng.sync()
    else:
        eng.smoke_cells_add_grad(0, s, gv=rv if use_v else None, gq=rq if use_q else None)
    after, fields_after = _all_grads(eng), _all_fields(eng)
    listed = np.zeros((RES,) * 3, bool)
    listed[cells[:, 0], cells[:, 1], cells[:, 2]] = True
    for t in range(RING + 1):
        for which, comps, rows, used in ((0, 3, rv, use_v), (1, qd, rq, use_q)):
            want = before[t][which].copy()
            if t == s and used:
                want[listed] = (before[t][which] + _dense(cells, rows, comps))[listed]
                assert not np.array_equal(_bits(want), _bits(before[t][which]))
            assert np.array_equal(_bits(after[t][which]), _bits(want)), (name, s, variant, t, which)
        for k in ('v', 'q'):
            assert np.array_equal(_bits(fields_after[t][k]), _bits(fields[t][k])), (name, s, variant, t, k)


@pytest.mark.parametrize('name', list(LISTS))
def test_scatter_adds_the_bits_of_the_dense_road(field, name):
    eng = field['eng']
    eng.smoke_cells_set(0, LISTS[name])
    rng = np.random.RandomState(len(name) + 3 * field['qd'])
    eng.smoke_reset_grad()
    for s in FRAMES:                                             # a cleared adjoint
        for variant in ('host', 'dev'):
            _check_scatter(field, name, s, variant, rng)
    _occupy(field)
    for s in FRAMES:                                             # an occupied one
        for variant in ('host', 'dev', 'gv-only', 'gq-only'):
            _check_scatter(field, name, s, variant, rng)
    # the dense road itself on the same rows: fe_smoke_add_grad of the field accumulated in list order adds the same bits everywhere
    cells, qd = LISTS[name], field['qd']
    rv, rq = rng.normal(size=(len(cells), 3)).astype(np.float32), rng.normal(size=(len(cells), qd)).astype(np.float32)
    eng.smoke_copy_grad(0, SCRATCH)
    eng.smoke_cells_add_grad(0, 0, gv=rv, gq=rq)
    eng.smoke_add_grad(SCRATCH, gv=_dense(cells, rv, 3), gq=_dense(cells, rq, qd))
    (gv_a, gq_a), (gv_b, gq_b) = eng.smoke_get_grad(0), eng.smoke_get_grad(SCRATCH)
    assert np.array_equal(gv_a, gv_b) and np.array_equal(gq_a, gq_b)          # (values: the dense add turns a -0 it passes into +0)
    listed = (cells[:, 0], cells[:, 1], cells[:, 2])
    assert np.array_equal(_bits(gv_a[listed]), _bits(gv_b[listed])) and np.array_equal(_bits(gq_a[listed]), _bits(gq_b[listed]))
    eng.smoke_cells_set(0, None)
    eng.smoke_reset_grad()


def test_host_and_device_variants_give_the_same_bits(field):
    import torch
    eng, qd = field['eng'], field['qd']
    cells = LISTS['n97']
    rng = np.random.RandomState(23)
    rv, rq = rng.normal(size=(97, 3)).astype(np.float32), rng.normal(size=(97, qd)).astype(np.float32)
    tv, tq = torch.from_numpy(rv).to('cuda:0'), torch.from_numpy(rq).to('cuda:0')
    _occupy(field)
    eng.smoke_cells_set(1, cells)
    for s in (0, RING):                                          # an occupied slot, a cleared one
        eng.smoke_copy_grad(s, SCRATCH)
        eng.smoke_cells_add_grad(1, s, gv=rv, gq=rq)
        eng.smoke_cells_add_grad(1, SCRATCH, gv=tv, gq=tq)
        eng.sync()
        (gv_h, gq_h), (gv_d, gq_d) = eng.smoke_get_grad(s), eng.smoke_get_grad(SCRATCH)
        assert np.array_equal(_bits(gv_h), _bits(gv_d)) and np.array_equal(_bits(gq_h), _bits(gq_d))
    # a new list under the same id: the grouping of the old one is gone
    eng.smoke_cells_set(1, LISTS['n300'])
    eng.smoke_reset_grad()
    r3 = rng.normal(size=(300, 3)).astype(np.float32)
    eng.smoke_cells_add_grad(1, 1, gv=r3)
    gv, gq = eng.smoke_get_grad(1)
    assert np.array_equal(_bits(gv), _bits(_dense(LISTS['n300'], r3, 3))) and not gq.any()
    eng.smoke_cells_add_grad(1, 1)                               # both NULL: succeeds, launches nothing
    assert np.array_equal(_bits(eng.smoke_get_grad(1)[0]), _bits(gv))
    eng.smoke_cells_set(1, None)
    eng.smoke_reset_grad()


def test_refusals_leave_the_adjoint_unchanged(field, hiplib):
    eng, qd = field['eng'], field['qd']
    _occupy(field)
    eng.smoke_cells_set(0, LISTS['n97'])
    rv, rq = np.ones((300, 3), np.float32), np.ones((300, qd), np.float32)
    pv, pq = rv.ctypes.data_as(C.c_void_p), rq.ctypes.data_as(C.c_void_p)
    import torch
    tv, tq = torch.ones((300, 3), dtype=torch.float32, device='cuda:0'), torch.ones((300, qd), dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    dv, dq = C.c_void_p(tv.data_ptr()), C.c_void_p(tq.data_ptr())
    before = _all_grads(eng)
    lib = eng.lib
    for fn, a, b in ((lib.fe_smoke_cells_add_grad, pv, pq), (lib.fe_smoke_cells_add_grad_dev, dv, dq)):
        for lid, s, what in ((2, 0, 'not set'), (_capi.FE_SMOKE_MAX_LISTS, 0, 'list id out of range'), (-1, 0, 'list id out of range'),
                             (0, -1, 'frame out of range'), (0, RING + 1, 'frame out of range')):
            assert fn(eng.h, lid, s, a, b) != 0, (lid, s)
            assert what in lib.fe_last_error(eng.h).decode(), (lid, s, lib.fe_last_error(eng.h).decode())
    with pytest.raises(_capi.FeEngineError, match='not set'):
        eng.smoke_cells_add_grad(2, 0, gv=np.zeros((0, 3), np.float32))
    with pytest.raises(_capi.FeEngineError, match='frame out of range'):
        eng.smoke_cells_add_grad(0, RING + 1, gv=rv[:97])
    after = _all_grads(eng)
    for (gv0, gq0), (gv1, gq1) in zip(before, after):
        assert np.array_equal(_bits(gv0), _bits(gv1)) and np.array_equal(_bits(gq0), _bits(gq1))
    eng.smoke_cells_set(0, None)
    eng.smoke_reset_grad()
    bare = S.make_engine(hiplib, S.water_block(n_grid=8, n_particles=8))
    for fn, a, b in ((bare.lib.fe_smoke_cells_add_grad, rv.ctypes.data_as(C.c_void_p), rq.ctypes.data_as(C.c_void_p)),
                     (bare.lib.fe_smoke_cells_add_grad_dev, dv, dq)):
        assert fn(bare.h, 0, 0, a, b) != 0
        assert 'no smoke field' in bare.lib.fe_last_error(bare.h).decode()
    bare.close()
