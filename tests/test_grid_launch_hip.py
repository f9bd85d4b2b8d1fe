"""The separate grid kernels' launches follow the active list (fluidlab_amd/csrc/fe_grid_launch.h): the sort sends the list's length to a host-mapped word,
the host sizes k_grid / k_grid<true> / k_grid_grad from it without waiting, and the road (one entry per wave, or the strided walk) is still chosen on the device.
A 64^3 grid (16^3 blocks: the fixed launch is 1,024 workgroups, the smallest list-sized one 512) with droplets that sit in the corners of one block, eight to
a block, and leave it diagonally between two sorts, so that the list grows from 27 to 125 entries per block.  What get_work_stats reports about the launches, and the same trajectory with the
list-sized launch on, off, and with the length forced too small (the long-list road) and too large (surplus waves), against each other and the fp64 oracle."""
import numpy as np
import pytest

import scenarios as S

pytestmark = pytest.mark.gpu

N_SUB, SORT = 9, 3
FIXED, FLOOR, QUANTUM, ONE_CAP = 1024, 512, 128, 6144        # fe_grid_launch.h


def chooser(n, blocks=4096):
    """fe_grid_launch_wgs for an exact length, no explicit cap (tests/csrc/grid_launch_test.cpp checks the function itself)"""
    g = (n + 3) // 4
    if g > ONE_CAP:
        return min(FIXED, (blocks + 3) // 4)
    g = -(-max(g, FLOOR) // QUANTUM) * QUANTUM
    return min(g, (blocks + 3) // 4)


def scene():
    """27 blocks (every fifth per axis) with eight droplets of 8 particles each, one in every corner of the block: 0.1 ... 0.5 cells inside it on every axis, so
    that the droplets of a block share no grid node (a particle's nodes are base .. base + 2, base = floor(x n - 0.5); its block is base >> 2) and keep their
    own velocities: 14 per axis (0.18 cells per substep) outwards.  After six substeps every droplet is in the diagonal neighbour of its block: the 27 entries
    around the block have become the 125 around its eight neighbours."""
    rng = np.random.RandomState(41)
    n, per = 64, 8
    xs, vs = [], []
    for c in [(i, j, k) for i in (2, 7, 12) for j in (2, 7, 12) for k in (2, 7, 12)]:
        lo = 4.0 * np.array(c, np.float64) + 0.5                                # x n of the block's first base cell
        for corner in range(8):
            hi_side = (corner >> np.arange(3)) & 1
            off = rng.uniform(0.1, 0.5, (per, 3))
            xs.append((lo + np.where(hi_side, 4.0 - off, off)) / n)
            vs.append(np.where(hi_side, 14.0, -14.0) + rng.normal(0, 0.2, (per, 3)))
    x, v = S.f32(np.concatenate(xs)), S.f32(np.concatenate(vs))
    N = len(x)
    sc = dict(S.water_block(n_grid=n, n_particles=N, seed=7), x=x, v=v)
    return sc


@pytest.fixture(scope='module')
def sc():
    return scene()


@pytest.fixture(scope='module')
def cot(sc):
    return S.random_cotangent(sc['N'], seed=12)


@pytest.fixture(scope='module')
def oracle_run(oracle64, sc, cot):
    o = S.make_engine(oracle64, sc)
    r = S.run_forward_backward(o, N_SUB, {k: v.astype(np.float64) for k, v in cot.items()})
    o.close()
    return r


def check_against_oracle(run, ref, what):
    """the bounds of test_hip_parity.py::test_grid_kernels_long_list_road, for the same quantities"""
    (sa, ga), (sb, gb) = run, ref
    print('MEASURED', what, 'x max abs', np.abs(sa['x'] - sb['x']).max(), 'v rel', S.rel_l2(sa['v'], sb['v']),
          {k: (1.0 - S.cosine(ga[k], gb[k]), S.rel_l2(ga[k], gb[k])) for k in ('gx', 'gv', 'gC', 'gF')})
    assert np.abs(sa['x'] - sb['x']).max() <= 2e-6 and S.rel_l2(sa['v'], sb['v']) <= 1e-4, what
    for k in ('gx', 'gv', 'gC', 'gF'):
        assert S.cosine(ga[k], gb[k]) >= 0.99999 and S.rel_l2(ga[k], gb[k]) <= 1e-3, (what, k, S.rel_l2(ga[k], gb[k]))


def test_launches_follow_the_list(hiplib, sc, cot):
    """Forward with a synchronisation behind every sort (so that its length has reached the host when the next launch is sized), backward per substep:
    the forward launches are smaller than the fixed 1,024 workgroups while the list is short and larger once it has grown, the backward ones are
    sized from the exact length of each frame's own order."""
    g = S.make_engine(hiplib, sc, options={'sort_interval': SORT})
    for f in range(N_SUB):
        g.substep(f, f, 0)
        if f % SORT == 0:
            g.sync()
    g.reset_grad()
    g.add_grad(N_SUB, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    for f in reversed(range(N_SUB)):
        g.substep_grad(f, f, 0)
    g.sync()
    ws = [g.get_work_stats(f, launches=True) for f in range(N_SUB)]
    g.close()
    n_act = [w['n_active_blocks'] for w in ws]
    print('MEASURED active list', n_act, 'k_grid', [(w['grid_launch']['wgs'], w['grid_launch']['hint'], w['grid_launch']['kind']) for w in ws],
          'k_grid_grad', [(w['grid_grad_launch']['wgs'], w['grid_grad_launch']['hint'], w['grid_grad_launch']['kind']) for w in ws])
    assert 300 <= n_act[0] <= 4 * FLOOR and n_act[N_SUB - 1] > 4 * FLOOR + 4 * QUANTUM, n_act       # a few hundred entries per ... then more than the smallest launch covers
    for f in range(N_SUB):
        fw, bw = ws[f]['grid_launch'], ws[f]['grid_grad_launch']
        # backward: the frame's own list, exactly
        assert bw['kind'] == 'exact' and bw['hint'] == n_act[f] and bw['wgs'] == chooser(n_act[f]), (f, bw, n_act[f])
        if f % SORT != 0:                                  # (the launch of a sort's own substep is sized before that sort has run: from the one before, or not at all)
            assert fw['kind'] == 'exact' and fw['hint'] == n_act[f] and fw['wgs'] == chooser(n_act[f]), (f, fw, n_act[f])
        else:
            want = {'none': FIXED, 'lagged': chooser((fw['hint'] * 125 + 99) // 100), 'exact': chooser(max(fw['hint'], 0))}      # (FE_GL_MARGIN_PCT on a lagged length)
            assert fw['kind'] in want and fw['wgs'] == want[fw['kind']] and (f == 0 or fw['kind'] != 'none'), (f, fw)
        assert fw['wgs'] % QUANTUM == 0 and bw['wgs'] % QUANTUM == 0
    assert ws[1]['grid_launch']['wgs'] == FLOOR < FIXED                                            # the short list: half the fixed launch
    assert ws[N_SUB - 1]['grid_launch']['wgs'] > ws[1]['grid_launch']['wgs']                      # ... and more once it has grown
    assert 4 * ws[N_SUB - 1]['grid_launch']['wgs'] >= n_act[N_SUB - 1]                            # one entry per wave


def test_same_results_whatever_the_launch(hiplib, sc, cot, oracle_run):
    """List-sized launch off (twice: the run-to-run difference of the fixed geometry, from the slow path's fp32 atomics), on, on with the length forced to 1
    (the smallest launch: the long-list road once the list has grown past four times its workgroups) and to the number of blocks (every launch at the
    grid's 1,024 workgroups, most waves without an entry).  All agree with the fp64 oracle within test_grid_kernels_long_list_road's bounds and with
    each other within twice the fixed geometry's own run-to-run difference -- which is nothing in this scene (two fixed runs agree bit for bit),
    so the launches must agree bit for bit: neither the wave that handles an entry nor the road it takes enters the result.
    (Measured before node_velocity() spelled its fma out: the long-list road's copy of it was contracted differently, 8e-9 in x and 7e-6 in the adjoint of x.)"""
    runs, stats = {}, {}
    for name, opts in (('fixed', {'grid_list_launch': 0}), ('fixed again', {'grid_list_launch': 0}), ('list-sized', {}),
                       ('hint 1', {'grid_hint': 1}), ('hint 4096', {'grid_hint': 4096})):
        g = S.make_engine(hiplib, sc, options=dict(opts, sort_interval=SORT))
        runs[name] = S.run_forward_backward(g, N_SUB, cot)
        stats[name] = [g.get_work_stats(f, launches=True) for f in (1, N_SUB - 1)]
        g.close()
    for name in runs:
        check_against_oracle(runs[name], oracle_run, name)
    # the launches were what the names say
    assert all(w['grid_launch'] == {'wgs': FIXED, 'hint': -1, 'kind': 'none'} and w['grid_grad_launch']['wgs'] == FIXED for w in stats['fixed'])
    assert all(w['grid_launch'] == {'wgs': FLOOR, 'hint': 1, 'kind': 'forced'} and w['grid_grad_launch']['wgs'] == FLOOR for w in stats['hint 1'])
    assert stats['hint 1'][1]['n_active_blocks'] > 4 * FLOOR                                       # more entries than waves: the long-list road
    assert all(w['grid_launch'] == {'wgs': 1024, 'hint': 4096, 'kind': 'forced'} for w in stats['hint 4096'])
    assert stats['list-sized'][1]['grid_grad_launch']['kind'] == 'exact' and FLOOR < stats['list-sized'][1]['grid_grad_launch']['wgs'] < FIXED

    def diff(a, b):
        (sa, ga), (sb, gb) = a, b
        d = {k: S.rel_l2(sa[k], sb[k]) for k in ('x', 'v', 'C', 'F')}
        d.update({k: S.rel_l2(ga[k], gb[k]) for k in ('gx', 'gv', 'gC', 'gF')})
        return d
    noise = diff(runs['fixed again'], runs['fixed'])
    for name in ('list-sized', 'hint 1', 'hint 4096'):
        d = diff(runs[name], runs['fixed'])
        print('MEASURED', name, 'vs fixed', d, 'fixed vs fixed', noise)
        for k in d:
            assert d[k] <= 2.0 * noise[k], (name, k, d[k], noise[k])


def test_edited_frame_drops_the_hint(hiplib, oracle64, sc, cot):
    """fe_set_frame between two steps: the lengths the host holds describe what the frames held before the edit, so the launches go back to the fixed
    geometry until a later sort reports; the trajectory goes on from the edited frame and matches the oracle."""
    f_edit = 4
    res = []
    for lib in (hiplib, oracle64):
        g = S.make_engine(lib, sc, options={'sort_interval': SORT} if lib is hiplib else None)
        g.substep(0, 0, 0)
        g.sync()                                               # (the first sort's length has reached the host)
        st = S.run_forward(g, f_edit - 1, f0=1)
        if lib is hiplib:
            before = g.get_work_stats(2, launches=True)['grid_launch']
        v_new = (np.asarray(st['v'], np.float64) * 0.5 + [0.0, 1.0, 0.0]).astype(np.float32)
        g.set_frame(f_edit, v=v_new.astype(g.dtype))
        for f in range(f_edit, N_SUB):
            g.substep(f, f, 0)
        if lib is hiplib:
            after = [g.get_work_stats(f, launches=True)['grid_launch'] for f in range(f_edit, N_SUB)]
        sa = S.get_state(g, N_SUB)
        g.reset_grad()
        c = cot if lib is hiplib else {k: v.astype(np.float64) for k, v in cot.items()}
        g.add_grad(N_SUB, c['gx'], c['gv'], c['gC'], c['gF'])
        for f in reversed(range(N_SUB)):
            g.substep_grad(f, f, 0)
        gx, gv, gC, gF = g.get_grad(0)
        res.append((sa, dict(gx=gx, gv=gv, gC=gC, gF=gF)))
        g.close()
    print('MEASURED launches before the edit', before, 'after', after)
    assert before['kind'] == 'exact' and before['wgs'] == FLOOR
    assert after[0] == {'wgs': FIXED, 'hint': -1, 'kind': 'none'} and after[1] == after[0]         # frames 4 and 5: the order of the sort at frame 3, whose length was dropped
    assert all(a['kind'] in ('none', 'exact') for a in after[2:])                                  # from the sort at frame 6 on: its own length, once it has arrived
    check_against_oracle(res[0], res[1], 'edited frame')


def test_recompute_road(hiplib, sc, cot, oracle_run):
    """grid_store = 0: the backward pass recomputes every frame's grid (k_grid<true>), sized like k_grid_grad from the frame's exact length"""
    g = S.make_engine(hiplib, sc, options={'sort_interval': SORT, 'grid_store': 0})
    run = S.run_forward_backward(g, N_SUB, cot)
    ws = g.get_work_stats(N_SUB - 1, launches=True)
    g.close()
    assert ws['grid_grad_launch']['kind'] == 'exact' and ws['grid_grad_launch']['wgs'] == chooser(ws['n_active_blocks'])
    check_against_oracle(run, oracle_run, 'grid_store 0')
