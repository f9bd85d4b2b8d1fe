"""GPU: loss-term programs of the HIP engine (fe_task_loss_*, kernels k_task_sep_fwd / k_task_pair / k_task_merge / k_task_bwd) against
the fp64 numpy interpreter of the same semantics (term_program.eval_terms_numpy: pairs by brute force), and the five task losses with the
device loss on against their torch path.

Tolerances.  Sums: 1e-11 x sum |terms|, the bound tests/test_frame_summary_hip.py derives for re-ordered fp64 sums -- the engine adds the same
fp64 terms in another order.  For the 1,500 particles of the separable terms the worst case is (n - 1) 2^-53 ~ 2e-13 of sum |terms|.  A pair term
has up to 4e5 pair-axis terms, but neither side adds them in one chain: a thread of k_task_pair adds at most 3 x 300 of them, the rest is a tree
(wave, workgroup, k_task_merge), and numpy sums pairwise, so both stay within ~1e3 x 2^-53 ~ 1e-13 of the exact sum.  Positions on multiples
of 1/64: every difference and partial sum is a multiple of 2^-6 far below 2^53, any order gives the same number, so values and counts must be EQUAL.
Gradients: the engine rounds scale x (fp64 gradient) to fp32 once, so an entry is within one fp32 ulp of the interpreter's fp64 result rounded
to fp32."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd.fluidengine.losses.term_program import (AXIS_ALL, AXIS_X, AXIS_Y, AXIS_Z, L1_CONST, L1_REF, PAIR_L1, SQ_CONST, Sel, Term,  # noqa: E402
                                                          eval_terms_numpy)

pytestmark = pytest.mark.gpu
SUM_TOL = 1e-11
N = 1500


def _x_used(eng, f):
    x, used = np.zeros((eng.N, 3), np.float32), np.zeros((eng.N,), np.int32)
    eng.get_frame(f, x=x, used=used)
    return x, used


def _within_one_ulp(got32, want64, tag):
    want32 = want64.astype(np.float32)
    err = np.abs(got32.astype(np.float64) - want32.astype(np.float64))
    ulp = np.spacing(np.abs(want32)).astype(np.float64)
    print(f'{tag}: max |err| / ulp {np.max(err / ulp)!r}, entries != 0: {int((want32 != 0).sum())}')
    assert np.all(err <= ulp), tag


def _check_values(eng, s, terms, x, used, mat, ref, tag, times=1):
    vals, _ = eval_terms_numpy(terms, x, used, mat, ref)
    sl, tl = eng.task_loss_get(s + 1, terms=True)
    for t in range(len(terms)):
        print(f'{tag}: term {t} got {tl[t, s]!r} want {times * vals[t]!r} err {abs(tl[t, s] - times * vals[t])!r} bound {SUM_TOL * times * abs(vals[t])!r}')
        assert abs(tl[t, s] - times * vals[t]) <= SUM_TOL * times * abs(vals[t]), (tag, t)
    assert abs(sl[s] - times * vals.sum()) <= SUM_TOL * times * np.abs(vals).sum(), tag
    return vals, sl, tl


def test_separable_terms(hiplib):
    sc = S.mixed_materials(n_grid=16, n_particles=N)
    assert 0 < int(sc['used'].sum()) < N
    eng = S.make_engine(hiplib, sc, max_substeps_local=32)
    eng.step(0, 0, 25, 0)                                     # sorts at 0, 10, 20: frame 25 is stored in a sorted order
    terms = [Term(L1_CONST, AXIS_X, Sel(0, N, -1, True), c=(0.8, 0.0, 0.0), weight=1.3),
             Term(SQ_CONST, AXIS_X | AXIS_Z, Sel(0, N, S.WATER, True), c=(0.88, 0.0, 0.78), weight=0.7),
             Term(L1_REF, AXIS_ALL, Sel(0, N, S.MILK_VIS, True), weight=-0.4),
             Term(L1_CONST, AXIS_Y, Sel(200, 900), c=(0.0, 0.05, 0.0), weight=2.0),
             Term(SQ_CONST, AXIS_Y | AXIS_Z, Sel(100, 1400, S.ICECREAM, False), c=(0.0, 0.3, 0.4), weight=1e-3)]
    eng.task_loss_alloc(4)
    eng.task_loss_set_terms(terms)
    with pytest.raises(Exception, match='before fe_task_loss_set_ref'):
        eng.task_loss_step(1, 25)
    eng.task_loss_set_ref(0)
    eng.task_loss_step(1, 25)
    x, used = _x_used(eng, 25)
    ref, _ = _x_used(eng, 0)
    vals, sl, tl = _check_values(eng, 1, terms, x, used, sc['mat'], ref, 'separable')
    assert np.all(vals != 0) and sl[0] == 0 and np.all(tl[:, 0] == 0)
    eng.task_loss_step(1, 25)                                 # a second call doubles the entries (v + v is exact)
    sl2, tl2 = eng.task_loss_get(2, terms=True)
    assert sl2[1] == 2 * sl[1] and np.array_equal(tl2[:, 1], 2 * tl[:, 1])
    eng.task_loss_clear()
    sl3, tl3 = eng.task_loss_get(4, terms=True)
    assert np.all(sl3 == 0) and np.all(tl3 == 0)
    # the gradient of the separable kinds, into a reset adjoint
    eng.reset_grad()
    eng.task_loss_step_grad(1, 25, 0.37)
    _, g = eval_terms_numpy(terms, x, used, sc['mat'], ref, True)
    _within_one_ulp(eng.get_grad(25)[0], 0.37 * g, 'separable gradient')
    eng.close()


def test_errors_leave_the_program_in_place(hiplib):
    import ctypes as C
    from fluidlab_amd import _capi
    sc = S.water_block(n_grid=16, n_particles=N)
    eng = S.make_engine(hiplib, sc)
    with pytest.raises(Exception, match='no loss-term program'):
        eng.task_loss_step(0, 0)
    good = [Term(L1_CONST, AXIS_X, Sel(0, N), c=(0.8, 0, 0), weight=1.0)]
    eng.task_loss_set_terms(good)
    with pytest.raises(Exception, match='fe_task_loss_alloc first'):
        eng.task_loss_step(0, 0)
    eng.task_loss_alloc(3)
    pair = Term(PAIR_L1, AXIS_ALL, Sel(0, 10), Sel(20, 30))
    bad = [([Term(7, AXIS_X, Sel(0, N))], 'unknown term kind'), ([Term(L1_CONST, 0, Sel(0, N))], 'axis_mask'),
           ([Term(L1_CONST, AXIS_X, Sel(0, N + 1))], 'outside'), ([Term(L1_CONST, AXIS_X, Sel(-2, 5))], 'outside'),
           ([Term(PAIR_L1, AXIS_X, Sel(0, 10), Sel(5, N + 3))], 'outside'), (good * 9, 'n_terms'), ([pair] * 3, 'pair terms'),
           ([Term(PAIR_L1, AXIS_ALL, Sel(0, 100), Sel(99, 200))], 'overlap')]
    for terms, msg in bad:
        with pytest.raises(Exception, match=msg):
            eng.task_loss_set_terms(terms)
    arr = (_capi.FeLossTerm * 1)(good[0].to_c())
    assert eng.lib.fe_task_loss_set_terms(eng.h, C.byref(arr), 1, C.sizeof(_capi.FeLossTerm) - 8) != 0
    assert b'term_size' in eng.lib.fe_last_error(eng.h)
    for s in (-1, 3):
        with pytest.raises(Exception, match='loss step out of range'):
            eng.task_loss_step(s, 0)
        with pytest.raises(Exception, match='loss step out of range'):
            eng.task_loss_step_grad(s, 0, 1.0)
    eng.task_loss_step(2, 0)                                  # the program set before the refused ones is still the one that runs
    x, used = _x_used(eng, 0)
    _check_values(eng, 2, good, x, used, sc['mat'], None, 'after refusals')
    eng.task_loss_set_terms(None)
    with pytest.raises(Exception, match='no loss-term program'):
        eng.task_loss_step(0, 0)
    eng.close()


def _quantised_frame(eng, sc, f, seed):
    """positions on multiples of 1/64 in [0, 1) (many ties) and some of the first 700 particles unused, written into frame f"""
    rng = np.random.RandomState(seed)
    x = (rng.randint(0, 64, (N, 3)) / 64.0).astype(np.float32)
    used = np.ones(N, np.int32)
    used[rng.choice(700, 90, replace=False)] = 0
    eng.set_frame(f, x=x, used=used)
    return x, used


@pytest.mark.parametrize('chunk', [64, 0, 1024])
def test_pairs_exact(hiplib, chunk):
    sc = S.water_block(n_grid=16, n_particles=N)
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'task_pair_chunk': chunk})
    assert eng.get_option('task_pair_chunk') == chunk
    with pytest.raises(Exception, match='multiple of 64'):
        eng.set_option('task_pair_chunk', 100)
    eng.step(0, 0, 25, 0)
    x, used = _quantised_frame(eng, sc, 25, 6)
    terms = [Term(PAIR_L1, AXIS_ALL, Sel(0, 300), None, weight=1.0),
             Term(PAIR_L1, AXIS_ALL, Sel(0, 700, -1, True), Sel(1000, 1300), weight=1.0)]
    eng.task_loss_alloc(2)
    eng.task_loss_set_terms(terms)
    eng.task_loss_step(0, 25)
    vals, g = eval_terms_numpy(terms, x, used, sc['mat'], None, True)
    sl, tl = eng.task_loss_get(2, terms=True)
    d = x[:300, None, :].astype(np.float64) - x[None, :300, :].astype(np.float64)
    print(f'chunk {chunk}: self pairs {tl[0, 0]!r} want {vals[0]!r}; two sets {tl[1, 0]!r} want {vals[1]!r}; ties among the self pairs {np.mean(d == 0):.4f}')
    assert np.mean(d == 0) > 0.01
    assert tl[0, 0] == vals[0] and tl[1, 0] == vals[1] and sl[0] == vals[0] + vals[1] and vals[0] > 0 and vals[1] > 0
    eng.reset_grad()
    eng.task_loss_step_grad(0, 25, 1.0)
    gx = eng.get_grad(25)[0]
    assert np.array_equal(g, np.round(g)) and np.abs(g).max() < 2 ** 24      # integer counts, exact in fp32
    assert np.array_equal(gx, g.astype(np.float32))
    unused = np.nonzero(used[:700] == 0)[0]
    assert len(unused[unused >= 300]) > 0 and np.all(gx[unused[unused >= 300]] == 0)      # an unused particle of set a outside the self-pair set gets nothing
    assert np.abs(gx[1000:1300]).max() > 0 and np.all(gx[700:1000] == 0) and np.all(gx[1300:] == 0)
    # the two terms one at a time: the two-set term's counts alone, then the self-pair term's
    for t in (1, 0):
        eng.task_loss_set_terms([terms[t]])
        eng.reset_grad()
        eng.task_loss_step_grad(0, 25, 1.0)
        _, gt = eval_terms_numpy([terms[t]], x, used, sc['mat'], None, True)
        assert np.array_equal(eng.get_grad(25)[0], gt.astype(np.float32)), t
    eng.close()


@pytest.mark.parametrize('chunk', [64, 0, 1024])
def test_pairs_general(hiplib, chunk):
    sc = S.mixed_materials(n_grid=16, n_particles=N)
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'task_pair_chunk': chunk})
    eng.step(0, 0, 25, 0)
    w, scale = -1e-4 * 0.7, 0.37
    terms = [Term(PAIR_L1, AXIS_ALL, Sel(0, 300), None, weight=w),
             Term(PAIR_L1, AXIS_X | AXIS_Z, Sel(0, 700, -1, True), Sel(1000, 1300, S.WATER, True), weight=w)]
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.task_loss_step(0, 25)
    x, used = _x_used(eng, 25)
    _check_values(eng, 0, terms, x, used, sc['mat'], None, f'pairs general chunk {chunk}')
    eng.reset_grad()
    eng.task_loss_step_grad(0, 25, scale)
    _, g = eval_terms_numpy(terms, x, used, sc['mat'], None, True)
    _within_one_ulp(eng.get_grad(25)[0], scale * g, f'pairs general gradient chunk {chunk}')
    eng.close()


def _program():
    """separable and pair terms on sub-ranges: a gradient delivered in the wrong particle order cannot pass"""
    return [Term(L1_CONST, AXIS_X, Sel(100, 1200, -1, True), c=(0.8, 0.0, 0.0), weight=1.3),
            Term(SQ_CONST, AXIS_Y | AXIS_Z, Sel(0, 900), c=(0.0, 0.3, 0.4), weight=0.7),
            Term(PAIR_L1, AXIS_ALL, Sel(0, 400, -1, True), Sel(800, 1100), weight=1e-4)]


def test_adjoint_in_another_order_and_refusal(hiplib):
    sc = S.water_block(n_grid=16, n_particles=N, seed=3)
    sc['used'] = (np.random.RandomState(8).rand(N) > 0.1).astype(np.int32)
    cot = S.random_cotangent(N, seed=2)
    terms = _program()
    eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'sort_interval': 10, 'fuse_bwd': 1})
    eng.task_loss_alloc(1)
    eng.task_loss_set_terms(terms)
    eng.step(0, 0, 25, 0)
    eng.reset_grad()
    eng.add_grad(25, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(0, 0, 25, 0)                                # back to frame 0: its adjoint is left in the order the next call's first substep works in
    g0 = eng.get_grad(0)[0]
    assert np.abs(g0).max() > 0
    eng.task_loss_step_grad(0, 0, 0.37)
    g1 = eng.get_grad(0)[0]
    x, used = _x_used(eng, 0)
    _, g = eval_terms_numpy(terms, x, used, sc['mat'], None, True)
    want = g0.astype(np.float64) + (0.37 * g).astype(np.float32).astype(np.float64)       # one fp32 addition of the once-rounded gradient
    err = np.abs(g1.astype(np.float64) - want)
    ulp = np.spacing(np.maximum(np.abs(g1), np.abs(g0))).astype(np.float64)
    print(f'adjoint in another order: max |err| / ulp {np.max(err / ulp)!r}; entries changed {int((g1 != g0).sum())} of {int((g != 0).sum())} with a gradient')
    assert np.all(err <= ulp) and (g1 != g0).sum() > 0.5 * (g != 0).sum()
    untouched = np.all(g == 0, axis=1)
    assert untouched.sum() >= 300 and np.array_equal(g1[untouched], g0[untouched])      # particles no term selects keep their adjoint
    eng.close()
    # a frame whose adjoint a fused fe_step_grad passed on in registers is refused (the arrangement of test_incomplete_adjoint_slots_are_refused)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': 10, 'fuse_bwd': 1})
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def test_determinism_and_read_only(hiplib):
    sc = S.water_block(n_grid=16, n_particles=N, seed=3)
    sc['used'] = (np.random.RandomState(8).rand(N) > 0.1).astype(np.int32)
    terms = _program()
    n_sub = 12

    def rollout(with_loss, chunk=64):
        eng = S.make_engine(hiplib, sc, max_substeps_local=32, options={'task_pair_chunk': chunk})
        eng.profile_enable(True)
        if with_loss:
            eng.task_loss_alloc(n_sub)
            eng.task_loss_set_terms(terms)
        for f in range(n_sub):
            eng.step(f, f, 1, 0)
            if with_loss:
                eng.task_loss_step(f, f + 1)
        return eng

    def frame_words(eng, f):                                  # (no F: this download does not expand a compact one)
        x, v, C_, u = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32), np.zeros((N, 3, 3), np.float32), np.zeros(N, np.int32)
        eng.get_frame(f, x, v, C_, None, u)
        return [_bits(a) for a in (x, v, C_)] + [u]

    plain, plain2, a, b = rollout(False), rollout(False), rollout(True), rollout(True)
    launches = [{k: n for k, (ms, n) in e.profile_read().items()} for e in (plain, a)]
    assert launches[0] == launches[1] and sum(launches[0].values()) > 0, launches       # the same substep kernels, none of the new ones among them
    repeats = all(np.array_equal(p, q) for p, q in zip(frame_words(plain, n_sub), frame_words(plain2, n_sub)))
    print(f'plain rollouts repeat bit for bit: {repeats}')
    if repeats:
        for p, q in zip(frame_words(plain, n_sub), frame_words(a, n_sub)):       # a rollout with the loss calls in it ends in the same frame
            assert np.array_equal(p, q)
        sa, sb = a.task_loss_get(n_sub, terms=True), b.task_loss_get(n_sub, terms=True)
        assert np.array_equal(_bits(sa[0]), _bits(sb[0])) and np.array_equal(_bits(sa[1]), _bits(sb[1])) and np.all(sa[0] != 0)
        engines = (a, b)
    else:                                                     # the substep itself does not repeat: compare the loss calls on one engine's stored frames
        engines = (a, a)
    # the forward call only reads: every stored frame is what it was, two evaluations of a frame give the same bits
    before = [frame_words(a, f) for f in (n_sub // 2, n_sub)]
    a.task_loss_clear()
    for f in range(n_sub):
        a.task_loss_step(f, f + 1)
    first = a.task_loss_get(n_sub, terms=True)
    a.task_loss_clear()
    for f in range(n_sub):
        a.task_loss_step(f, f + 1)
    second = a.task_loss_get(n_sub, terms=True)
    assert np.array_equal(_bits(first[0]), _bits(second[0])) and np.array_equal(_bits(first[1]), _bits(second[1])) and np.all(first[0] != 0)
    for bf, f in zip(before, (n_sub // 2, n_sub)):
        for p, q in zip(bf, frame_words(a, f)):
            assert np.array_equal(p, q)
    # adjoints: bit-identical between the two engines (or two evaluations on one), multi-chunk integer atomics included
    grads = []
    for e in engines:
        e.reset_grad()
        e.task_loss_step_grad(0, n_sub, 0.37)
        grads.append(e.get_grad(n_sub)[0])
    assert np.array_equal(_bits(grads[0]), _bits(grads[1])) and np.abs(grads[0]).max() > 0
    for e in (plain, plain2, a, b):
        e.close()


ENV_CASES = ['gathering_easy', 'gathering_o', 'pouring', 'transporting', 'mixing']


@pytest.mark.parametrize('case', ENV_CASES)
def test_env_device_loss_matches_the_torch_path(hiplib, case):
    """step_loss of a rollout with the device loss on against the existing torch path evaluated on the same frames (1e-10 relative, the
    extra terms included), and the adjoint one loss step seeds into a reset adjoint (one fp32 ulp per entry; a frame in the middle of the
    rollout: on Pouring's last step the attraction is rounded separately from the program, two roundings against the torch path's one)."""
    import test_task_loss_terms as T
    env, pol, _ = T.build_env(case, None)                     # None = the HIP library
    te = env.taichi_env
    loss, sim = te.loss, te.simulator
    assert sim.engine.elib.backend == 'hip-gfx950' and not loss._device_loss
    env.enable_device_loss()
    assert loss._device_loss
    te.set_state(te.get_state()['state'], grad_enabled=True)
    te.apply_agent_action_p(pol.get_actions_p())
    host, frames = [], []
    for i in range(env.horizon):
        te.step(pol.get_action_v(i, agent=te.agent, update=True) if i < env.horizon_action else None)
        s, f = sim.cur_step_global - 1, sim.cur_substep_local
        host.append(float(loss.step_value(s, f, *loss.frame(f), False)[0]))     # the torch path on the same, still resident frame
        frames.append((s, f))
    dev = np.array(loss.step_loss, np.float64)
    host = np.array(host)
    rel = np.abs(dev[:len(host)] - host) / np.abs(host)
    print(f'{case}: step_loss device {dev[:3]!r} ... torch {host[:3]!r} ...; max relative difference {rel.max()!r}')
    assert np.all(host != 0) and np.all(rel <= 1e-10)
    assert abs(loss.cur_step_loss() - host[-1]) <= 1e-10 * abs(host[-1])
    info = te.get_final_loss()
    assert abs(info['loss'] - host.sum()) <= 1e-10 * np.abs(host).sum()
    s, f = frames[len(frames) // 2]
    eng = sim.engine
    eng.reset_grad()
    loss.compute_step_loss_grad(s, f)
    g_dev = eng.get_grad(f)[0]
    loss._device_loss = False                                 # the same loss object through today's path
    try:
        eng.reset_grad()
        loss.compute_step_loss_grad(s, f)
        g_host = eng.get_grad(f)[0]
    finally:
        loss._device_loss = True
    err = np.abs(g_dev.astype(np.float64) - g_host.astype(np.float64))
    ulp = np.spacing(np.abs(g_host)).astype(np.float64)
    print(f'{case}: seeded adjoint of frame {f}: {int((g_host != 0).sum())} entries, max |err| / ulp {np.max(err / ulp)!r}, bit-identical {np.array_equal(g_dev, g_host)}')
    assert np.abs(g_host).max() > 0 and np.all(err <= ulp)
    te.reset_grad()
    loss.clear_loss()
    assert np.all(np.asarray(loss.step_loss) == 0)


def test_transporting_end_to_end(hiplib):
    """Solver.forward_backward of reduced Transporting 'diff' with the device loss on against the same with it off: the bounds
    test_transporting_on_the_gpu asserts between two implementations of this scene."""
    import test_host_env as H
    import test_task_loss_terms as T
    out = []
    for on in (True, False):
        env, pol, cfg = T.build_env('transporting', None)
        if on:
            env.enable_device_loss()
        info, g, _ = H._solver_pass(env, 'configs/exp_transporting.yaml', T._prep_transporting)
        out.append((info, g))
    (ia, ga), (ib, gb) = out
    la, lb = ia['loss'], ib['loss']
    cols = [0, 5]
    print(f'MEASURED transporting device loss on vs off: loss {la!r} vs {lb!r} rel {abs(la - lb) / abs(lb):.2e} | grad cos {S.cosine(ga[:, cols], gb[:, cols]):.7f} '
          f'relL2 {S.rel_l2(ga[:, cols], gb[:, cols]):.3e} | dist {ia["dist_loss"]!r} vs {ib["dist_loss"]!r} attraction {ia["attraction_loss"]!r} vs {ib["attraction_loss"]!r}')
    assert abs(la - lb) <= 1e-5 * abs(lb)
    assert np.isfinite(ga).all() and S.cosine(ga[:, cols], gb[:, cols]) >= 0.99999 and S.rel_l2(ga[:, cols], gb[:, cols]) <= 2e-3
    assert ia['attraction_loss'] > 0 and abs(ia['dist_loss'] - ib['dist_loss']) <= 1e-5 * ib['dist_loss']
