"""GPU: observation fields of the HIP engine (fe_field_obs_*: kernels k_field_obs_scatter, k_field_obs_decode, k_field_obs_grad) against the host
restatement (term_program.field_obs_of_points / field_obs_grad_of_points) on the downloaded frame.

Scene: S.mixed_materials at 16^3 with 3,000 particles (four materials, 10 % unused, moving), sort_interval = 10, stepped to frame 25: frame 5
is stored in the identity order, frame 25 behind the sorts at 10 and 20.

Forward.  The words are integers, so the field must EQUAL the restatement bit for bit on both roads (LDS copies, global atomics), and channel
0 must equal fe_density_get.  Backward.  A word of the x or v adjoint changes by the fp64 sum rounded to fp32 once and added once: within one
fp32 ulp of the interpreter's fp64 value, plus one ulp of the word it was added to, plus 2^-50 times the sum of the absolute terms (the device
contracts multiply-adds, the interpreter does not).  Everything else in the adjoint is equal bit for bit.  Measured: the largest error is
0.995 of that bound on occupied slots (frames 25 .. 17 substep by substep, frames 20, 10 and 0 after ranged sweeps; the slots of 20 and 10 are
stored in another order than their frames) and 0 on cleared ones."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

from fluidlab_amd import _capi  # noqa: E402
from fluidlab_amd.fluidengine.losses.term_program import DensityField, Sel, density_stencil, field_obs_grad_of_points, field_obs_of_points  # noqa: E402

pytestmark = pytest.mark.gpu
N = 3000
F = 25
F_EARLY = 5
OPTS = {'sort_interval': 10}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _frame(eng, f):
    """x, v, C, used of frame f (no F: that download would expand a compactly stored one)"""
    x, v, C_, u = np.zeros((eng.N, 3), np.float32), np.zeros((eng.N, 3), np.float32), np.zeros((eng.N, 3, 3), np.float32), np.zeros(eng.N, np.int32)
    eng.get_frame(f, x, v, C_, None, u)
    return x, v, C_, u


def _box(x, n, lo_q=0.03, hi_q=0.97):
    """a field of n cells over the quantile box of the points x on every unprojected axis"""
    origin, cell = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    for a in range(3):
        if n[a] == 1:
            continue
        lo, hi = np.quantile(x[:, a].astype(np.float64), [lo_q, hi_q])
        cell[a] = float((hi - lo) / n[a])
        origin[a] = float(lo)
    return DensityField(tuple(origin), tuple(cell), tuple(n))


class Case:
    def __init__(self, hiplib):
        self.sc = S.mixed_materials(n_grid=16, n_particles=N)
        self.eng = S.make_engine(hiplib, self.sc, max_substeps_local=32, options=OPTS)
        self.eng.step(0, 0, F, 0)
        self.mat = self.sc['mat']
        self.frames = {f: _frame(self.eng, f) for f in (F_EARLY, F)}
        x, v, _, used = self.frames[F]
        assert 0 < int(used.sum()) < N and np.abs(v).max() > 0.1

    def ref(self, f, spec, sel, channels, drop=()):
        x, v, _, used = self.frames[f]
        m = sel.mask(used, self.mat)
        m[list(drop)] = False
        return field_obs_of_points(x[m], v[m], spec, channels, quantise=True), m


@pytest.fixture(scope='module')
def case(hiplib):
    c = Case(hiplib)
    yield c
    c.eng.close()


def _shapes(case):
    """name -> (spec, selection, channels, takes the LDS road when allowed)"""
    x, _, _, used = case.frames[F]
    xs = x[used != 0]
    full = Sel(0, N, -1, True)
    part = _box(xs, (8, 8, 8), 0.45, 0.97)                    # the lower half of the fluid along every axis lies outside
    return {'16x1x16 C=4': (_box(xs, (16, 1, 16)), full, 4, True),
            '8x8x8 C=1': (_box(xs, (8, 8, 8)), Sel(100, 2800, -1, True), 1, True),
            '8x8x8 C=4': (_box(xs, (8, 8, 8)), Sel(100, 2800, S.WATER, True), 4, True),
            'partly overlapping 8x8x8 C=4': (part, full, 4, True),
            '16x16x16 C=4 (LDS beyond 64 KiB)': (_box(xs, (16, 16, 16)), full, 4, True),
            '40x40x40 C=4 (global road only)': (_box(xs, (40, 40, 40)), full, 4, False)}


SHAPES = ['16x1x16 C=4', '8x8x8 C=1', '8x8x8 C=4', 'partly overlapping 8x8x8 C=4', '16x16x16 C=4 (LDS beyond 64 KiB)', '40x40x40 C=4 (global road only)']


@pytest.mark.parametrize('name', SHAPES)
def test_forward_equals_the_restatement_on_both_roads(case, name):
    import torch
    eng = case.eng
    spec, sel, channels, fits = _shapes(case)[name]
    assert (channels * 8 * int(np.prod(spec.n)) <= 160 * 1024) == fits
    eng.field_obs_set(1, spec, sel, channels)
    eng.density_set_field(0, spec)
    try:
        for f in (F_EARLY, F):                                # before and after the sorts: the particle order is irrelevant
            want, m = case.ref(f, spec, sel, channels)
            x = case.frames[f][0][m]
            ok, base, _, _ = density_stencil(x, spec)
            nn = np.array(spec.n)
            share = float((ok & np.all((base + 2 >= 0) & (base <= nn - 1), axis=1)).mean())
            got = {}
            for lds in (0, 1):
                eng.set_option('field_obs_lds', lds)
                got[lds] = eng.field_obs(f, 1)
                assert got[lds].shape == (channels,) + tuple(spec.n) and got[lds].dtype == np.float64
                bad = int((_bits(got[lds]) != _bits(want)).sum())
                print(f'{name} frame {f} field_obs_lds {lds}: {int(m.sum())} selected, {share:.3f} deposit; sum D {got[lds][0].sum()!r} restatement {want[0].sum()!r}; words that differ {bad}')
                assert bad == 0
            assert np.array_equal(_bits(got[0]), _bits(got[1]))
            assert want[0].sum() > 50 and (channels == 1 or np.abs(want[1:]).max() > 0.01)
            if name.startswith('partly'):
                assert 0.05 < share < 0.8
            # channel 0 is the density field of the same box and selection
            assert np.array_equal(_bits(got[1][0]), _bits(eng.density_field(f, 0, sel)))
            # the device form: float32 of the host form
            dev = eng.field_obs_dev(f, 1)
            assert dev.dtype == torch.float32 and dev.is_cuda and tuple(dev.shape) == got[1].shape
            assert np.array_equal(_bits(dev.cpu().numpy()), _bits(got[1].astype(np.float32)))
    finally:
        eng.set_option('field_obs_lds', -1)
        eng.field_obs_set(1, None)
        eng.density_set_field(0, None)


def test_guarded_particles_deposit_nothing(hiplib, case):
    """v_x = inf on one particle and v_y = 2049 on another: the field is the field of the frame without the two, in all channels"""
    eng = S.make_engine(hiplib, case.sc, max_substeps_local=32, options=OPTS)
    eng.step(0, 0, 12, 0)
    x, v, _, used = _frame(eng, 12)
    p, q = [int(i) for i in np.nonzero(used)[0][[40, 900]]]
    v[p, 0] = np.inf
    v[q, 1] = 2049.0
    eng.set_frame(12, v=v)
    x, v2, _, used = _frame(eng, 12)
    assert np.isinf(v2[p, 0]) and v2[q, 1] == 2049.0
    spec = _box(x[used != 0], (8, 8, 8))
    sel = Sel(0, N, -1, True)
    m = sel.mask(used, case.mat)
    with_them = field_obs_of_points(x[m], np.where(np.isfinite(v2), v2, 0.0)[m], spec, 1, quantise=True)
    m[[p, q]] = False
    for channels in (4, 1):
        want = field_obs_of_points(x[m], v2[m], spec, channels, quantise=True)
        eng.field_obs_set(0, spec, sel, channels)
        for lds in (0, 1):
            eng.set_option('field_obs_lds', lds)
            got = eng.field_obs(12, 0)
            assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want)), (channels, lds)
    assert not np.array_equal(with_them[0], want[0])          # the two would have been seen
    # ... and they get no gradient
    G = np.random.RandomState(3).uniform(-1, 1, (4,) + spec.shape).astype(np.float32)
    eng.field_obs_set(0, spec, sel, 4)
    eng.reset_grad()
    eng.field_obs_add_grad(12, 0, G)
    gx, gv = eng.get_grad(12)[:2]
    assert not gx[[p, q]].any() and not gv[[p, q]].any() and np.isfinite(gx).all() and np.isfinite(gv).all() and np.abs(gx).max() > 0
    eng.close()


def _check_add_grad(case_or_frame, eng, f, k, spec, sel, channels, G, dev, mat, what):
    """G1 = G0 + the interpreter's (gx, gv) within the bound in the x and v words of the selected particles; every other word equal"""
    import torch
    x, v, _, used = _frame(eng, f)
    G0 = eng.get_grad(f)
    eng.field_obs_add_grad(f, k, torch.as_tensor(G, device=f'cuda:{eng.device}') if dev else G)
    G1 = eng.get_grad(f)
    m = sel.mask(used, mat)
    gx, gv, ax, av = (np.zeros((eng.N, 3)) for _ in range(4))
    gx[m], gv[m], ax[m], av[m] = field_obs_grad_of_points(x[m], v[m], spec, G.astype(np.float64), terms=True)
    worst = 0.0
    for i, (g, a) in enumerate(((gx, ax), (gv, av))):
        add32 = g.astype(np.float32)
        want = G0[i].astype(np.float64) + add32.astype(np.float64)
        err = np.abs(G1[i].astype(np.float64) - want)
        bound = np.spacing(np.abs(add32)).astype(np.float64) + np.spacing(np.abs(G0[i])).astype(np.float64) + 2.0 ** -50 * a      # (the word added to is the one before the call)
        touched = a > 0
        assert np.all(err[touched] <= bound[touched]), (what, i, float(np.max(err[touched] / bound[touched])))
        assert np.array_equal(_bits(G1[i][~touched]), _bits(G0[i][~touched])), (what, i)      # unselected, guarded and out-of-field particles
        worst = max(worst, float(np.max(err[touched] / bound[touched])) if touched.any() else 0.0)
        assert (G1[i] != G0[i]).sum() >= 0.5 * (g != 0).sum()
    assert np.array_equal(_bits(G1[2]), _bits(G0[2])) and np.array_equal(_bits(G1[3]), _bits(G0[3])), what      # C and all of F's planes
    n_x, n_v = int((gx != 0).any(axis=1).sum()), int((gv != 0).any(axis=1).sum())
    print(f'{what}: {n_x} particles with an x gradient, {n_v} with a v gradient, of {int(m.sum())} selected; max err / bound {worst:.3f}')
    assert n_x > 200 and (channels == 1) == (n_v == 0) and (~m).sum() > 100
    return G1


@pytest.mark.parametrize('name', ['16x1x16 C=4', '8x8x8 C=1', 'partly overlapping 8x8x8 C=4', '40x40x40 C=4 (global road only)'])
def test_backward_cleared_slot(case, name):
    eng = case.eng
    spec, sel, channels, _ = _shapes(case)[name]
    G = np.random.RandomState(21).uniform(-1, 1, (channels,) + spec.shape).astype(np.float32)
    eng.field_obs_set(2, spec, sel, channels)
    out = []
    for dev in (False, True):
        eng.reset_grad()
        out.append(_check_add_grad(case, eng, F, 2, spec, sel, channels, G, dev, case.mat, f'{name}, cleared slot, dev={dev}'))
    for a, b in zip(out[0], out[1]):                          # host and _dev forms: the same bits
        assert np.array_equal(_bits(a), _bits(b))
    eng.reset_grad()
    eng.field_obs_set(2, None)


def test_backward_occupied_slots_across_sorts(case):
    """occupied slots, in the frame's own order and in another.  Substep by substep the engine leaves every adjoint in its frame's order
    (frames 25 .. 17, the sort at 20 included).  A ranged fe_step_grad that ends on a frame a sort made leaves that frame's adjoint in the
    order the next call's first substep works in, the order of the frame in front of the sort: there the slot comes from the adjoint's own
    slot_of_pid and not from the frame's.  Which is which is read from the engine (table_of_frame_<f>, table_of_grad_<f>) and both must occur."""
    eng = case.eng
    shapes = _shapes(case)
    cot = S.random_cotangent(N)
    names = ('16x1x16 C=4', '8x8x8 C=4')
    rng = np.random.RandomState(22)
    same_order, other_order = [], []

    def inject(f, what):
        assert np.abs(eng.get_grad(f)[0]).max() > 0
        tf, tg = eng.get_option(f'table_of_frame_{f}'), eng.get_option(f'table_of_grad_{f}')
        assert tf >= 0 and tg >= 0                            # (an occupied slot has an order of its own)
        (same_order if tf == tg else other_order).append(f)
        k = f % 2
        spec, sel, channels, _ = shapes[names[k]]
        G = (rng.uniform(-1, 1, (channels,) + spec.shape) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        _check_add_grad(case, eng, f, k, spec, sel, channels, G, f % 3 == 0, case.mat, f'{what}, frame {f} (frame order {int(tf)}, adjoint order {int(tg)})')
        assert eng.get_option(f'table_of_grad_{f}') == tg         # the call leaves the slot in its order

    try:
        for k, name in enumerate(names):
            spec, sel, channels, _ = shapes[name]
            eng.field_obs_set(k, spec, sel, channels)
        eng.reset_grad()
        eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        for f in range(F, 16, -1):                            # substep by substep: every position relative to the sort at 20
            if f < F:
                eng.substep_grad(f, f, 0)
            inject(f, 'substep by substep')
        assert eng.get_option(f'table_of_frame_{F}') != eng.get_option('table_of_frame_17')
        eng.reset_grad()
        assert eng.get_option(f'table_of_grad_{F}') == -1     # a cleared slot
        eng.add_grad(F, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        for f0, n in ((20, 5), (10, 10), (0, 10)):            # ranged calls that end on the frames the sorts made (and on frame 0)
            eng.step_grad(f0, f0, n, 0)
            inject(f0, f'after fe_step_grad({f0}, {n})')
        print(f'adjoint slot in its frame\'s order: frames {same_order}; in another order: frames {other_order}')
        assert len(same_order) >= 9 and other_order, (same_order, other_order)
        with pytest.raises(_capi.FeEngineError, match='out of range'):
            eng.get_option('table_of_grad_33')
    finally:
        eng.reset_grad()
        for k in (0, 1):
            eng.field_obs_set(k, None)


def test_compact_F_adjoint_and_refusals(hiplib):
    """an inviscid liquid: F's adjoint is stored as its trace inside a ranged fe_step_grad.  The cotangent goes into the x and v words of such
    a slot and F still expands to (trace / 3) I afterwards; a frame whose adjoint was passed on in registers is refused, like every other
    refusal without a changed word"""
    sc = S.water_block(n_grid=16, n_particles=1500, seed=3)
    sc['used'] = (np.random.RandomState(8).rand(1500) > 0.1).astype(np.int32)
    sc['v'] = S.f32(np.random.RandomState(9).normal(0, 0.5, (1500, 3)))
    cot = S.random_cotangent(1500)
    eng = S.make_engine(hiplib, sc, options={'sort_interval': 10, 'fuse_bwd': 1})
    assert eng.get_option('compact_F') == 1
    eng.step(0, 0, 6, 0)
    x, v, _, used = _frame(eng, 3)
    spec = _box(x[used != 0], (8, 1, 8))
    sel = Sel(50, 1400, -1, True)
    eng.field_obs_set(3, spec, sel, 4)
    G = np.random.RandomState(5).uniform(-1, 1, (4,) + spec.shape).astype(np.float32)
    eng.reset_grad()
    eng.add_grad(6, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(3, 3, 3, 0)                                 # frames 5, 4, 3: frame 4's x, v, C adjoint never reached memory; frame 3's F adjoint is compact

    def xvC(f):                                               # (no gF: handing it out would expand the compact planes)
        g = [np.zeros((1500, 3), np.float32), np.zeros((1500, 3), np.float32), np.zeros((1500, 3, 3), np.float32)]
        assert eng.lib.fe_get_grad(eng.h, f, *[a.ctypes.data_as(C.c_void_p) for a in g], None) == 0
        return g

    G0 = xvC(3)
    # (Frame 4's slot cannot be read back: fe_get_grad and fe_copy_grad refuse it for the same reason.  What can be seen of it is the order
    # the engine keeps for it, which an accepted call may set and a refused one must not; the neighbouring slot is compared word for word.)
    order4 = eng.get_option('table_of_grad_4')
    for call in (lambda: eng.field_obs_add_grad(4, 3, G), lambda: eng.field_obs_add_grad(4, 3, _dev(eng, G))):
        with pytest.raises(_capi.FeEngineError, match='registers'):
            call()
    assert b'registers' in eng.lib.fe_last_error(eng.h)
    ptr = G.ctypes.data_as(C.c_void_p)
    refused = [(lambda: eng.lib.fe_field_obs_add_grad(eng.h, 3, 4, ptr), b'out of range'), (lambda: eng.lib.fe_field_obs_add_grad(eng.h, 3, -1, ptr), b'out of range'),
               (lambda: eng.lib.fe_field_obs_add_grad(eng.h, 3, 2, ptr), b'not set'), (lambda: eng.lib.fe_field_obs_add_grad(eng.h, 3, 3, None), b'NULL'),
               (lambda: eng.lib.fe_field_obs_add_grad_dev(eng.h, 3, 3, None), b'NULL'), (lambda: eng.lib.fe_field_obs_add_grad(eng.h, -1, 3, ptr), b'out of range'),
               (lambda: eng.lib.fe_field_obs_add_grad(eng.h, 10 ** 6, 3, ptr), b'out of range')]
    for call, msg in refused:
        assert call() != 0 and msg in eng.lib.fe_last_error(eng.h), msg
    for a, b in zip(G0, xvC(3)):
        assert np.array_equal(_bits(a), _bits(b))
    assert eng.get_option('table_of_grad_4') == order4
    m = sel.mask(used, sc['mat'])

    def take(f):
        """the cotangent into frame f's slot, whose F is not downloaded before the call: x and v words within the bound, C's equal"""
        xf, vf, _, uf = _frame(eng, f)
        assert np.array_equal(uf, used)
        A0 = xvC(f)
        eng.field_obs_add_grad(f, 3, G)
        A1 = xvC(f)
        gx, gv, ax, av = (np.zeros((1500, 3)) for _ in range(4))
        gx[m], gv[m], ax[m], av[m] = field_obs_grad_of_points(xf[m], vf[m], spec, G.astype(np.float64), terms=True)
        for i, (g, a) in enumerate(((gx, ax), (gv, av))):
            changed = _bits(A1[i]) != _bits(A0[i])
            assert changed.sum() > 0.5 * (g != 0).sum() > 100 and not changed[a == 0].any()
            err = np.abs(A1[i].astype(np.float64) - (A0[i].astype(np.float64) + g.astype(np.float32)))
            assert np.all(err <= np.spacing(np.abs(g.astype(np.float32))) + np.spacing(np.abs(A0[i])) + 2.0 ** -50 * a)
        assert np.array_equal(_bits(A1[2]), _bits(A0[2]))

    take(3)                                                   # the call's first frame: defined, and taken
    # fuse_bwd = 0: every frame's adjoint reaches memory, and inside a ranged call the F adjoint of a liquid is stored as its trace alone.
    # Frame 4's slot is such a one; after the call its F still expands to (trace / 3) I for every used particle, bit for bit on the diagonal
    eng.set_option('fuse_bwd', 0)
    eng.reset_grad()
    eng.add_grad(6, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(3, 3, 3, 0)
    take(4)
    gF = eng.get_grad(4)[3][used != 0]
    assert np.abs(gF[:, 0, 0]).max() > 0 and np.array_equal(gF[:, 0, 0], gF[:, 1, 1]) and np.array_equal(gF[:, 0, 0], gF[:, 2, 2])
    assert not gF[:, 0, 1].any() and not gF[:, 1, 0].any() and not gF[:, 0, 2].any() and not gF[:, 2, 0].any() and not gF[:, 1, 2].any() and not gF[:, 2, 1].any()
    eng.close()


def _dev(eng, a):
    import torch
    return torch.as_tensor(a, device=f'cuda:{eng.device}')


def test_set_refusals_leave_the_field_in_place(case):
    eng = case.eng
    spec, sel, channels, _ = _shapes(case)['8x8x8 C=4']
    eng.field_obs_set(0, spec, sel, channels)
    want, _ = case.ref(F, spec, sel, channels)
    assert np.array_equal(_bits(eng.field_obs(F, 0)), _bits(want))
    D = DensityField
    nan, inf = float('nan'), float('inf')
    bad = [(4, spec, sel, 4, 'field id out of range'), (-1, spec, sel, 4, 'field id out of range'),
           (0, D(spec.origin, spec.cell, (8, 0, 8)), sel, 4, r'n\[a\] must be >= 1'), (0, D(spec.origin, spec.cell, (128, 129, 128)), sel, 4, 'more than FE_DENSITY_MAX_CELLS'),
           (0, D(spec.origin, spec.cell, (1 << 22, 1, 1)), sel, 4, 'more than FE_DENSITY_MAX_CELLS'), (0, D(spec.origin, (0.1, 0.0, 0.1), (8, 8, 8)), sel, 4, 'cell must be finite and positive'),
           (0, D(spec.origin, (0.1, nan, 0.1), (8, 8, 8)), sel, 4, 'cell must be finite and positive'), (0, D(spec.origin, (0.1, 0.1, inf), (8, 8, 8)), sel, 4, 'cell must be finite and positive'),
           (0, D((0.0, -inf, 0.0), spec.cell, (8, 8, 8)), sel, 4, 'origin must be finite'), (0, spec, sel, 2, 'channels must be 1'), (0, spec, sel, 0, 'channels must be 1'),
           (0, spec, Sel(0, N + 1), 4, 'outside'), (0, spec, Sel(-1, N), 4, 'outside')]
    for k, sp, se, ch, msg in bad:
        with pytest.raises(_capi.FeEngineError, match=msg):
            eng.field_obs_set(k, sp, se, ch)
    c = spec.to_c()
    assert eng.lib.fe_field_obs_set(eng.h, 0, C.byref(c), C.sizeof(_capi.FeDensitySpec) - 8, None, 4) != 0 and b'spec_size' in eng.lib.fe_last_error(eng.h)
    out = np.zeros(want.size + 1)
    for n_values, ptr, msg in ((want.size - 1, out.ctypes.data_as(C.c_void_p), b'n_values'), (want.size // 4, out.ctypes.data_as(C.c_void_p), b'n_values'), (want.size, None, b'null output')):
        assert eng.lib.fe_field_obs_get(eng.h, F, 0, ptr, C.c_longlong(n_values)) != 0 and msg in eng.lib.fe_last_error(eng.h)
    assert eng.lib.fe_field_obs_get_dev(eng.h, F, 0, None) != 0 and b'null output' in eng.lib.fe_last_error(eng.h)
    assert eng.lib.fe_field_obs_get_dev(eng.h, F, 1, None) != 0 and b'not set' in eng.lib.fe_last_error(eng.h)
    assert not out.any()
    with pytest.raises(_capi.FeEngineError, match='field_obs_lds must be'):
        eng.set_option('field_obs_lds', 2)
    assert eng.get_option('field_obs_lds') == -1
    assert np.array_equal(_bits(eng.field_obs(F, 0)), _bits(want))      # the field set before the refused calls is still the one read
    with pytest.raises(_capi.FeEngineError, match='must be a contiguous'):
        eng.field_obs_add_grad(F, 0, _dev(eng, np.zeros((4, 8, 8), np.float32)))
    eng.field_obs_set(0, None)
    with pytest.raises(_capi.FeEngineError, match='not set'):
        eng.field_obs(F, 0)


def test_read_only_and_lifetime(hiplib, case):
    sc = case.sc
    a = S.make_engine(hiplib, sc, max_substeps_local=32, options=OPTS)
    out = np.zeros(64)
    ptr = out.ctypes.data_as(C.c_void_p)
    g32 = np.zeros(64, np.float32).ctypes.data_as(C.c_void_p)
    # entries before any set-up fail cleanly
    for call in (lambda: a.lib.fe_field_obs_get(a.h, 0, 0, ptr, C.c_longlong(64)), lambda: a.lib.fe_field_obs_get_dev(a.h, 0, 0, ptr),
                 lambda: a.lib.fe_field_obs_add_grad(a.h, 0, 0, g32), lambda: a.lib.fe_field_obs_add_grad_dev(a.h, 0, 0, g32)):
        assert call() != 0 and b'not set' in a.lib.fe_last_error(a.h)
    assert a.lib.fe_field_obs_set(a.h, 0, None, 0, None, 4) == 0      # removing a field that was never set
    with pytest.raises(_capi.FeEngineError, match='not set'):
        a.field_obs(0, 0)
    # a rollout with the calls in it against a plain engine: every frame is only read, and the launches are those of the plain rollout
    plain = S.make_engine(hiplib, sc, max_substeps_local=32, options=OPTS)
    for en in (a, plain):
        en.profile_enable(True)
    small = DensityField((0.2, 0.0, 0.2), (0.15, 1.0, 0.15), (4, 1, 4))
    a.field_obs_set(0, small, None, 1)
    G_small = np.random.RandomState(1).uniform(-1, 1, (1, 4, 1, 4)).astype(np.float32)
    for s in range(3):
        for en in (a, plain):
            en.step(s * 8, s * 8, 8, 0)
        before = [_frame(a, f) for f in range(0, (s + 1) * 8 + 1)]
        d1, d2 = a.field_obs((s + 1) * 8, 0), a.field_obs((s + 1) * 8, 0)
        a.field_obs_dev(s * 8 + 3, 0)
        a.field_obs_add_grad((s + 1) * 8, 0, G_small)
        assert d1.tobytes() == d2.tobytes() and d1.sum() > 100
        for f, fa in enumerate(before):
            assert all(p.tobytes() == q.tobytes() for p, q in zip(fa, _frame(a, f))), f
        for f in range(0, (s + 1) * 8 + 1):                   # (the other engine's host does the same downloads)
            _frame(plain, f)
    launches = [{k: n for k, (ms, n) in en.profile_read().items()} for en in (a, plain)]
    assert launches[0] == launches[1] and sum(launches[0].values()) > 0, launches
    plain.close()
    # a field re-set to a larger size grows its buffers
    x, v, _, used = _frame(a, 24)
    big = _box(x[used != 0], (40, 40, 40))
    a.field_obs_set(0, big, None, 4)
    want = field_obs_of_points(x[used != 0], v[used != 0], big, 4)
    assert np.array_equal(_bits(a.field_obs(24, 0)), _bits(want)) and a.field_obs_dev(24, 0).shape == (4, 40, 40, 40)
    a.reset_grad()
    a.field_obs_add_grad(24, 0, np.ones((4, 40, 40, 40), np.float32))
    assert np.abs(a.get_grad(24)[1]).max() > 0
    a.field_obs_set(0, small, None, 1)                        # ... and back to the small one
    assert np.array_equal(_bits(a.field_obs(24, 0)), _bits(field_obs_of_points(x[used != 0], v[used != 0], small, 1)))
    a.close()
    # a second engine after the first was destroyed
    b = S.make_engine(hiplib, sc, max_substeps_local=32, options=OPTS)
    b.step(0, 0, 4, 0)
    x, v, _, used = _frame(b, 4)
    b.field_obs_set(3, small, None, 4)
    assert np.array_equal(_bits(b.field_obs(4, 3)), _bits(field_obs_of_points(x[used != 0], v[used != 0], small, 4)))
    b.close()
