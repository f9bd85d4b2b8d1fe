"""GPU: target clouds of the HIP engine (fe_cloud_set / fe_cloud_query, the kernels of csrc/fe_nearest.h) and the FE_TERM_NEAREST_SQ /
FE_TERM_COVER_SQ terms of the loss-term programs against the all-pairs fp64 restatement (term_program.nearest_bruteforce /
eval_terms_numpy).

Bounds.  Indices and d2 are a function of the frame alone and must EQUAL the restatement, bit for bit, at every "nn_cells".  A term's value
is a sum of n fp64 numbers in another order than numpy's: within (n - 1) 2^-53 sum d2 (weight 1, so no further rounding).  The interpreter
forms the gradient with the engine's operations in the engine's order -- COVER in the same fixed point -- so on a cleared adjoint slot the
adjoint is np.float32(scale g) exactly, and on an occupied slot one fp32 addition away: one ulp per word."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd.fluidengine.losses.term_program import (AXIS_ALL, AXIS_X, AXIS_Y, AXIS_Z, COVER_SQ, L1_CONST, NEAREST_SQ, Sel, Term,  # noqa: E402
                                                          eval_terms_numpy, nearest_bruteforce)

pytestmark = pytest.mark.gpu
MASKS = [AXIS_ALL, AXIS_X | AXIS_Z, AXIS_Y]
N_BIG, F = 1500, 25


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _x_used(eng, f):
    x, used = np.zeros((eng.N, 3), np.float32), np.zeros((eng.N,), np.int32)
    eng.get_frame(f, x=x, used=used)
    return x, used


def _restate(x, used, mat, sel, cloud, mask):
    """what fe_cloud_query must return, from the all-pairs restatement"""
    N = len(x)
    ia = np.nonzero((Sel(0, N, -1, True) if sel is None else sel).mask(used, mat))[0]
    nn_p, d2_p = np.full(N, -1, np.int64), np.zeros(N)
    j, d = nearest_bruteforce(x[ia], cloud, mask)
    nn_p[ia], d2_p[ia] = j, d
    k, d2_c = nearest_bruteforce(cloud, x[ia], mask)
    nn_c = np.where(k >= 0, ia[np.maximum(k, 0)] if len(ia) else -1, -1)
    return nn_p, d2_p, nn_c, d2_c


def _check_query(eng, f, x, used, mat, sel, cloud, mask, tag):
    got = eng.cloud_query(f, 0, sel, mask)
    want = _restate(x, used, mat, sel, cloud, mask)
    for name, g, w in zip(('nn_of_particle', 'd2_of_particle', 'nn_of_point', 'd2_of_point'), got, want):
        if g.dtype == np.float64:
            bad = _bits(g) != _bits(w)
        else:
            bad = g.astype(np.int64) != w
        assert not bad.any(), f'{tag} mask {mask}: {name} differs at {np.nonzero(bad)[0][:8]}: got {g[bad][:4]!r} want {w[bad][:4]!r}'
    return got


@pytest.fixture(scope='module')
def engines(hiplib):
    made = {}

    def get(n):
        if n not in made:
            made[n] = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=n), max_substeps_local=4)
        return made[n]
    yield get
    for e in made.values():
        e.close()


@pytest.mark.parametrize('M', [1, 65, 1000])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 300])
def test_cloud_query_equals_the_restatement(engines, N, M):
    eng = engines(N)
    rs = np.random.RandomState(100 * N + M)
    mat = np.full(N, S.WATER, np.int32)
    x = (0.30 + 0.30 * rs.rand(N, 3)).astype(np.float32)
    used = np.ones(N, np.int32)
    if N >= 63:
        used[0] = 0                                             # an unused particle
        x[1] = [np.nan, 0.4, 0.4]                               # skipped: a non-finite word
        x[2] = [2.5, 0.4, 0.4]                                  # skipped where x is in the mask; a far query / candidate where it is not
        x[6] = [0.4, -7.0, 0.4]                                 # likewise for y
        x[5] = x[4]                                             # two particles in one place: the lower pid wins
        x[10:20] = (x[10:20] * 64).round() / 64                 # coarse positions: equal d2 to different points
    clouds = {'overlapping': (0.35 + 0.30 * rs.rand(M, 3)), 'disjoint and far': (0.35 + 0.30 * rs.rand(M, 3)) + [1.2, -0.9, 0.8],
              'on coarse positions': (rs.randint(16, 48, (M, 3)) / 64.0), 'one point M times': np.tile(0.35 + 0.30 * rs.rand(1, 3), (M, 1))}
    sels = [None, Sel(min(3, N - 1), N, -1, False)]
    for tag, cloud in clouds.items():
        cloud = cloud.astype(np.float32)
        if tag == 'overlapping':
            cloud[0] = x[min(3, N - 1)]                         # a particle on a cloud point: d2 = 0
            cloud[M - 1] = cloud[M // 2]                        # a duplicated cloud point: the lower index wins
        eng.set_frame(0, x=x, used=used)
        eng.cloud_set(0, cloud)
        for mask in MASKS:
            for sel in sels:
                got = _check_query(eng, 0, x, used, mat, sel, cloud, mask, f'N {N} M {M} {tag}')
        if tag == 'overlapping':                               # (got: mask y, the selection from particle min(3, N - 1) on)
            p3 = min(3, N - 1)
            assert got[1][p3] == 0.0 and got[0][p3] >= 0 and (N < 63 or (got[0][1] == -1 and got[0][6] == -1))
            if M > 2:
                assert not (got[0] == M - 1).any()
    # every candidate in one cell, no candidate at all
    xs = np.tile(x[min(3, N - 1)], (N, 1))
    eng.set_frame(0, x=xs, used=used)
    _check_query(eng, 0, xs, used, mat, None, cloud, AXIS_ALL, 'all particles in one place')
    none = np.zeros(N, np.int32)
    eng.set_frame(0, x=x, used=none)
    got = _check_query(eng, 0, x, none, mat, None, cloud, AXIS_ALL, 'no candidate')
    assert (got[0] == -1).all() and (got[2] == -1).all() and not got[3].any()
    eng.cloud_set(0, None)


class Case:
    """a stepped frame: water at frame 25, stored in a sorted order, a tenth of the particles unused"""

    def __init__(self, hiplib):
        self.sc = S.water_block(n_grid=16, n_particles=N_BIG, seed=3)
        self.sc['used'] = (np.random.RandomState(8).rand(N_BIG) > 0.1).astype(np.int32)
        self.eng = S.make_engine(hiplib, self.sc, max_substeps_local=32, options={'sort_interval': 10})
        self.eng.step(0, 0, F, 0)
        self.x, self.used = _x_used(self.eng, F)
        self.mat = self.sc['mat']
        rs = np.random.RandomState(5)
        lo, hi = self.x[self.used != 0].min(axis=0), self.x[self.used != 0].max(axis=0)
        self.cloud = (lo + (hi - lo) * (0.2 + 0.9 * rs.rand(777, 3))).astype(np.float32)        # overlaps the water and sticks out of it
        self.sel = Sel(100, 1400, -1, True)


@pytest.fixture(scope='module')
def case(hiplib):
    c = Case(hiplib)
    yield c
    c.eng.close()


def test_query_before_and_after_a_sort(case):
    eng = case.eng
    eng.cloud_set(0, case.cloud)
    for f in (0, 5, F):
        x, used = _x_used(eng, f)
        for mask in MASKS:
            _check_query(eng, f, x, used, case.mat, case.sel, case.cloud, mask, f'frame {f}')
    eng.cloud_set(0, None)


def _evaluate(eng, terms, scale):
    eng.task_loss_set_terms(terms)
    eng.task_loss_clear()
    eng.task_loss_step(0, F)
    sl, tl = eng.task_loss_get(1, terms=True)
    eng.reset_grad()
    eng.task_loss_step_grad(0, F, scale)
    return sl.copy(), tl.copy(), eng.get_grad(F)[0]


@pytest.mark.parametrize('mask', [AXIS_ALL, AXIS_X | AXIS_Z])
def test_values_adjoints_resolutions_and_repeats(case, mask):
    eng = case.eng
    eng.cloud_set(1, case.cloud)
    eng.task_loss_alloc(1)
    scale = 0.37
    clouds = {1: case.cloud}
    ia = case.sel.mask(case.used, case.mat)
    for kind, n in ((NEAREST_SQ, int(ia.sum())), (COVER_SQ, len(case.cloud))):
        # the value, weight 1: a re-ordered sum of n numbers
        one = [Term(kind, mask, case.sel, weight=1.0, cloud=1)]
        vals, _ = eval_terms_numpy(one, case.x, case.used, case.mat, None, False, clouds=clouds)
        sl, tl, _ = _evaluate(eng, one, scale)
        bound = (n - 1) * 2.0 ** -53 * vals[0]
        print(f'kind {kind} mask {mask}: step_loss {sl[0]!r} interpreter {vals[0]!r} err {abs(sl[0] - vals[0])!r} bound {bound!r}')
        assert vals[0] > 0 and abs(sl[0] - vals[0]) <= bound and tl[0, 0] == sl[0]
        # the adjoint on a cleared slot, one term: the interpreter's gradient rounded once
        one = [Term(kind, mask, case.sel, weight=0.7, cloud=1)]
        _, g = eval_terms_numpy(one, case.x, case.used, case.mat, None, True, clouds=clouds)
        want = (scale * g).astype(np.float32)
        out = {}
        for cells in (1, 3, 0, 0):
            eng.set_option('nn_cells', cells)
            assert eng.get_option('nn_cells') == cells
            res = _evaluate(eng, one, scale) + eng.cloud_query(F, 1, case.sel, mask)
            bad = _bits(res[2]) != _bits(want)
            assert not bad.any(), f'kind {kind} nn_cells {cells}: {int(bad.sum())} adjoint words differ, e.g. {res[2][bad][:4]!r} want {want[bad][:4]!r}'
            for prev in out.values():                             # every resolution, and a second evaluation: the same bits in every output
                for p, q in zip(prev, res):
                    assert np.array_equal(_bits(p), _bits(q))
            out[cells] = res
        moved = np.any(want != 0, axis=1)
        print(f'kind {kind} mask {mask}: {int(moved.sum())} of {int(ia.sum())} selected particles have a gradient, max |g| {np.abs(want).max()!r}')
        assert moved.sum() > (0.5 * ia.sum() if kind == NEAREST_SQ else 50) and not moved[~ia].any()
        for a in range(3):
            if not (mask >> a) & 1:
                assert not want[:, a].any()
    # both kinds and a separable term on an occupied slot: one fp32 addition of the once-rounded gradient
    terms = [Term(NEAREST_SQ, mask, case.sel, weight=0.7, cloud=1), Term(L1_CONST, AXIS_X, Sel(200, 1200, -1, True), c=(0.45, 0.0, 0.0), weight=1.3),
             Term(COVER_SQ, mask, Sel(0, 900, -1, True), weight=-0.3, cloud=1)]
    vals, g = eval_terms_numpy(terms, case.x, case.used, case.mat, None, True, clouds=clouds)
    cot = S.random_cotangent(N_BIG, seed=2)
    eng.task_loss_set_terms(terms)
    eng.reset_grad()
    eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    g0 = eng.get_grad(F)[0]
    eng.task_loss_step_grad(0, F, scale)
    g1 = eng.get_grad(F)[0]
    want = g0.astype(np.float64) + (scale * g).astype(np.float32).astype(np.float64)
    err = np.abs(g1.astype(np.float64) - want)
    ulp = np.spacing(np.maximum(np.abs(g1), np.abs(g0))).astype(np.float64)
    print(f'three terms on an occupied slot: max err / ulp {np.max(err / ulp)!r}; words changed {int((g1 != g0).sum())}')
    assert np.all(err <= ulp) and (g1 != g0).sum() > 1000 and vals[0] > 0 > vals[2]
    untouched = np.all(g == 0, axis=1)
    assert untouched.sum() > 50 and np.array_equal(g1[untouched], g0[untouched])
    eng.task_loss_set_terms(None)
    eng.cloud_set(1, None)


def test_the_calls_only_read(case, hiplib):
    eng = case.eng

    def frame_words(e, f):
        x, v, C_, u = np.zeros((N_BIG, 3), np.float32), np.zeros((N_BIG, 3), np.float32), np.zeros((N_BIG, 3, 3), np.float32), np.zeros(N_BIG, np.int32)
        e.get_frame(f, x, v, C_, None, u)
        return [_bits(a) for a in (x, v, C_)] + [u]

    terms = [Term(NEAREST_SQ, AXIS_ALL, case.sel, cloud=0), Term(COVER_SQ, AXIS_X | AXIS_Z, case.sel, cloud=0)]
    before = (frame_words(eng, F), frame_words(eng, F - 5), eng.get_work_stats(F), eng.get_options())
    eng.cloud_set(0, case.cloud)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.task_loss_step(0, F)
    eng.cloud_query(F, 0, case.sel, AXIS_Y)
    after = (frame_words(eng, F), frame_words(eng, F - 5), eng.get_work_stats(F), eng.get_options())
    for b, a in zip(before[:2], after[:2]):
        for p, q in zip(b, a):
            assert np.array_equal(p, q)
    assert before[2:] == after[2:]
    # a short rollout with the calls in it: the same substep launches as one without, none of the new kernels among them -- and, where
    # the substep itself repeats bit for bit between two engines, the same frames and work lists
    def rollout(with_calls):
        e = S.make_engine(hiplib, case.sc, max_substeps_local=32, options={'sort_interval': 10})
        e.profile_enable(True)
        if with_calls:
            e.cloud_set(0, case.cloud)
            e.task_loss_alloc(1)
            e.task_loss_set_terms(terms)
        for f0 in (0, 6, 12):
            e.step(f0, f0, 6, 0)
            if with_calls:
                e.task_loss_step(0, f0 + 6)
                e.cloud_query(f0 + 3, 0, None, AXIS_ALL)
        return e

    plain, plain2, withc = rollout(False), rollout(False), rollout(True)
    launches = [{k: n for k, (ms, n) in e.profile_read().items()} for e in (plain, withc)]
    assert launches[0] == launches[1] and sum(launches[0].values()) > 0, launches
    repeats = all(np.array_equal(p, q) for f in (9, 18) for p, q in zip(frame_words(plain, f), frame_words(plain2, f)))
    print(f'plain rollouts repeat bit for bit: {repeats}')
    if repeats:
        for f in (9, 18):
            for p, q in zip(frame_words(plain, f), frame_words(withc, f)):
                assert np.array_equal(p, q)
            assert plain.get_work_stats(f) == withc.get_work_stats(f)
    for e in (plain, plain2, withc):
        e.close()
    eng.task_loss_set_terms(None)
    eng.cloud_set(0, None)


def test_adjoint_in_another_order_and_refusal(hiplib):
    sc = S.water_block(n_grid=16, n_particles=N_BIG, seed=3)
    sc['used'] = (np.random.RandomState(8).rand(N_BIG) > 0.1).astype(np.int32)
    cot = S.random_cotangent(N_BIG, seed=2)
    sel = Sel(100, 1300, -1, True)
    cloud = (0.28 + 0.30 * np.random.RandomState(4).rand(500, 3)).astype(np.float32)
    terms = [Term(NEAREST_SQ, AXIS_ALL, sel, weight=0.6, cloud=2), Term(COVER_SQ, AXIS_X | AXIS_Z, sel, weight=0.9, cloud=2),
             Term(L1_CONST, AXIS_X, Sel(0, 400), c=(0.5, 0, 0), weight=0.2)]
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'sort_interval': 10, 'fuse_bwd': 1})
    eng.cloud_set(2, cloud)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.step(0, 0, F, 0)
    eng.reset_grad()
    eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(0, 0, F, 0)                                 # back to frame 0: its adjoint is left in the order the next call's first substep works in
    g0 = eng.get_grad(0)[0]
    assert np.abs(g0).max() > 0
    eng.task_loss_step_grad(0, 0, 0.37)
    g1 = eng.get_grad(0)[0]
    x, used = _x_used(eng, 0)
    _, g = eval_terms_numpy(terms, x, used, sc['mat'], None, True, clouds={2: cloud})
    want = g0.astype(np.float64) + (0.37 * g).astype(np.float32).astype(np.float64)
    err = np.abs(g1.astype(np.float64) - want)
    ulp = np.spacing(np.maximum(np.abs(g1), np.abs(g0))).astype(np.float64)
    print(f'adjoint in another order: max err / ulp {np.max(err / ulp)!r}; words changed {int((g1 != g0).sum())} of {int((g != 0).sum())} with a gradient')
    assert np.all(err <= ulp) and (g1 != g0).sum() > 0.5 * (g != 0).sum() and (g != 0).sum() > 2000
    untouched = np.all(g == 0, axis=1)
    assert untouched.sum() >= 100 and np.array_equal(g1[untouched], g0[untouched])
    eng.close()
    # a frame whose adjoint a fused fe_step_grad passed on in registers is refused
    eng = S.make_engine(hiplib, sc, options={'sort_interval': 10, 'fuse_bwd': 1})
    eng.cloud_set(2, cloud)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.step(0, 0, 6, 0)
    eng.reset_grad()
    eng.add_grad(6, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(2, 2, 4, 0)                                 # frames 5 ... 2: the slot of frame 3 is the incomplete one
    eng.task_loss_step_grad(0, 2, 1.0)                        # the call's first frame: defined
    with pytest.raises(Exception, match='registers'):
        eng.task_loss_step_grad(0, 3, 1.0)
    eng.close()


def test_refusals_leave_everything_in_place(case):
    import ctypes as C
    from fluidlab_amd import _capi
    eng = case.eng
    good = [Term(NEAREST_SQ, AXIS_ALL, case.sel, weight=0.5, cloud=0), Term(COVER_SQ, AXIS_X | AXIS_Z, case.sel, weight=2.0, cloud=0)]
    with pytest.raises(Exception, match='names a cloud that is not set'):
        eng.task_loss_set_terms(good)
    eng.cloud_set(0, case.cloud)
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(good)
    cot = S.random_cotangent(N_BIG, seed=9)

    def state():
        eng.task_loss_clear()
        eng.task_loss_step(0, F)
        eng.reset_grad()
        eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        adj0 = eng.get_grad(F)[0]
        return eng.task_loss_get(1, terms=True) + eng.cloud_query(F, 0, case.sel, AXIS_ALL) + (adj0,)

    before = state()
    vals, _ = eval_terms_numpy(good, case.x, case.used, case.mat, None, False, clouds={0: case.cloud})
    assert abs(before[0][0] - vals.sum()) <= 1e-12 * vals.sum() and vals.sum() > 0
    adj = eng.get_grad(F)[0]
    bad = case.cloud.copy()
    bad[17, 1] = np.nan
    far = case.cloud.copy()
    far[3, 2] = 2.0001
    for k, pts, msg in ((4, case.cloud, 'cloud id out of range'), (-1, case.cloud, 'cloud id out of range'), (0, bad, 'not finite or beyond'), (0, far, 'not finite or beyond')):
        with pytest.raises(Exception, match=msg):
            eng.cloud_set(k, pts)
    assert eng.lib.fe_cloud_set(eng.h, 0, case.cloud.ctypes.data_as(C.c_void_p), (1 << 20) + 1) != 0        # (refused on n alone: the points are not read)
    assert b'FE_CLOUD_MAX_POINTS' in eng.lib.fe_last_error(eng.h)
    with pytest.raises(Exception, match='names this cloud'):
        eng.cloud_set(0, None)
    sel = case.sel
    bad_terms = [([Term(NEAREST_SQ, AXIS_ALL, sel, cloud=1)], 'names a cloud that is not set'), ([Term(COVER_SQ, AXIS_ALL, sel, cloud=4)], 'cloud id out of range'),
                 ([Term(NEAREST_SQ, AXIS_ALL, sel, cloud=-1)], 'cloud id out of range'), ([Term(COVER_SQ, 0, sel, cloud=0)], 'axis_mask must name'),
                 (good + good[:1], 'nearest terms'), ([Term(NEAREST_SQ, AXIS_ALL, Sel(0, N_BIG + 1), cloud=0)], 'outside'), ([Term(7, AXIS_X, Sel(0, N_BIG))], 'unknown term kind')]
    for terms, msg in bad_terms:
        with pytest.raises(Exception, match=msg):
            eng.task_loss_set_terms(terms)
    packed = good[1].to_c()
    packed.b.require_used = 1
    arr = (_capi.FeLossTerm * 1)(packed)
    assert eng.lib.fe_task_loss_set_terms(eng.h, C.byref(arr), 1, C.sizeof(_capi.FeLossTerm)) != 0
    assert b'zeros in the rest of b' in eng.lib.fe_last_error(eng.h)
    for args, msg in (((F, 1, None, AXIS_ALL), 'not set'), ((F, 0, None, 0), 'axis_mask must name'), ((F, 0, Sel(0, N_BIG + 1), AXIS_ALL), 'outside'), ((999, 0, None, AXIS_ALL), 'frame index')):
        with pytest.raises(Exception, match=msg):
            eng.cloud_query(*args)
    with pytest.raises(Exception, match='nn_cells must be'):
        eng.set_option('nn_cells', -1)
    assert np.array_equal(_bits(eng.get_grad(F)[0]), _bits(adj))            # the adjoint the refused calls found is still there
    after = state()                                                         # the program and the cloud set before the refused calls still run
    for p, q in zip(before, after):
        assert np.array_equal(_bits(p), _bits(q))
    eng.task_loss_set_terms(None)
    eng.cloud_set(0, None)                                                  # no program names it any more
    with pytest.raises(Exception, match='not set'):
        eng.cloud_query(F, 0, None, AXIS_ALL)


def test_chamfer_matching_loss_device_against_the_host_path(hiplib):
    import test_host_env as H
    env = H._small('LatteArt-v0', None, horizon=6, horizon_action=6, loss_type='chamfer', n_pool=300)       # None = the HIP library
    te = env.taichi_env
    loss, sim = te.loss, te.simulator
    assert sim.engine.elib.backend == 'hip-gfx950' and loss.axis_mask == (AXIS_X | AXIS_Z) and type(loss).__name__ == 'ChamferMatchingLoss'
    rng = np.random.RandomState(5)
    loss.set_target_points(np.stack([rng.uniform(0.3, 0.7, 777), rng.uniform(0.5, 0.9, 777), rng.uniform(0.35, 0.65, 777)], axis=1))
    env.enable_device_loss()
    assert loss._device_loss
    pol = env.demo_policy()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    host, bounds, frames = [], [], []
    mat = sim.particles_i.mat.to_numpy()
    terms = loss.device_terms()
    for i in range(env.horizon):
        te.step(pol.get_action_v(i, agent=te.agent, update=True))
        s, f = sim.cur_step_global - 1, sim.cur_substep_local
        x, used = _x_used(sim.engine, f)
        vals, _ = eval_terms_numpy(terms, x, used, mat, None, False, clouds={0: loss.target})      # the interpreter on the same, still resident frame
        n = max(int(terms[0].a.mask(used, mat).sum()), len(loss.target))
        host.append(float(vals.sum()))
        bounds.append((n - 1) * 2.0 ** -53 * float(np.abs(vals).sum()) + 2.0 ** -52 * abs(host[-1]))      # two re-ordered sums and their addition
        frames.append((s, f, x, used))
    dev, host = np.array(loss.step_loss, np.float64), np.array(host)
    print(f'step_loss device {dev!r} host {host!r} err {np.abs(dev - host)!r} bound {np.array(bounds)!r}')
    assert np.all(host > 0) and np.all(np.abs(dev - host) <= np.array(bounds))
    assert abs(te.get_final_loss()['loss'] - host[-1]) <= bounds[-1]
    # the search as the host layers hand it out
    s, f, x, used = frames[-1]
    sel = terms[0].a
    got = te.nearest_in_cloud(f, 0, sel, AXIS_X | AXIS_Z)
    for g, w in zip(got, _restate(x, used, mat, sel, loss.target, AXIS_X | AXIS_Z)):
        assert np.array_equal(g, w)
    # the x-adjoint of the last frame against the host path: the same gradient rounded once
    eng = sim.engine
    eng.reset_grad()
    loss.compute_step_loss_grad(s, f)
    g_dev = eng.get_grad(f)[0]
    loss._device_loss = False                                 # the same loss object through the host path
    try:
        eng.reset_grad()
        loss.compute_step_loss_grad(s, f)
        g_host = eng.get_grad(f)[0]
    finally:
        loss._device_loss = True
    err = np.abs(g_dev.astype(np.float64) - g_host.astype(np.float64))
    print(f'x-adjoint of frame {f}: {int((g_host != 0).sum())} entries, max err / ulp {np.max(err / np.spacing(np.abs(g_host)).astype(np.float64))!r}')
    assert np.abs(g_host).max() > 0 and np.all(err <= np.spacing(np.abs(g_host)).astype(np.float64))


def test_latteart_env_with_the_chamfer_loss_steps_forward_and_backward(hiplib):
    import test_host_env as H
    rng = np.random.RandomState(3)
    target = np.stack([rng.uniform(0.3, 0.7, 400), np.full(400, 0.7), rng.uniform(0.35, 0.65, 400)], axis=1).astype(np.float32)
    env = H._small('LatteArt-v0', None, horizon=2, horizon_action=2, loss_type='chamfer', n_pool=200, target=target)      # (quality 0.5: the smallest this scene is run at)
    te = env.taichi_env
    assert np.array_equal(te.loss.target, target)
    env.enable_device_loss()
    pol = env.demo_policy()
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    for i in range(env.horizon):
        te.step(pol.get_action_v(i, agent=te.agent, update=True))
    info = te.get_final_loss()
    assert np.isfinite(info['loss']) and info['loss'] > 0
    te.reset_grad()
    te.get_final_loss_grad()
    for i in range(env.horizon - 1, -1, -1):
        te.step_grad(pol.get_action_v(i))
    g = te.simulator.engine.get_grad(0)[0]
    assert np.isfinite(g).all()
