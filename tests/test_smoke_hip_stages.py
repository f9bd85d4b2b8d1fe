"""The HIP smoke solver (fluidlab_amd/csrc/fe_smoke.h) against the oracle stage by stage, on the edge cases of tests/smoke_cases.py:
q_dim 1..3, slabs at and beyond the domain walls, slabs of one layer and of none, grids smaller than a wave, cavities with no or one
free neighbour, back-traces that leave the grid on every face, frames that already hold data, and the frame ring as the host drives it.

Bounds.  u = 2^-24.  A stencil stage is compared with the fp64 stage applied to the device's own input; its per-cell bound is
2 m u sum|terms| for an expression of m floating-point operations (the 2 covers either choice of fused-multiply-add contraction).
Advection and every adjoint have no such closed bound (chained trilinear samples, expf, sqrtf, atomics): there the yardstick is
err32, the error of the fp32 oracle against the fp64 oracle on the same fp32 inputs, and the device may be 4 err32 off the fp64 oracle
in max-norm (floor 4 u max|field|): the fp32 oracle and the kernel do the same operations in another order and with other contraction
(two maxima over a few thousand cells of one error distribution differ by about 2) and the device's expf, sqrtf and division are 1-2
ulp where glibc's are half an ulp (another factor of about 2).

The action gradient is the exception to "err32 as measured once".  Each of its components is one number: the sum over all free cells
of per-cell terms of either sign, which k_smoke_advect_grad adds up through a 64-lane shuffle tree, one LDS float atomic per wave and
one global float atomic per block, and the oracle in a loop.  The rounding error of such a sum is relative to sum|term|, not to the
|sum| that is left after cancellation, and for a group of one to three numbers err32 is one to three draws from that error's
distribution, not a maximum over thousands of cells: a single draw is below a tenth of the distribution's width one time in
thirteen, and then no kernel can stay within 4 of it.  So for the action groups, and for them only, err32 is the largest of DRAWS = 8
draws: the error of the fp32 oracle against the fp64 oracle for the test's cotangent and for seven more of the same pattern and
size, which differ in nothing but the random signs and sizes the rounding errors meet.  (The largest of 8 draws of |N(0, s)| is below
0.67 s with probability 2^-8.)  The margin stays 4, and the device is run on the test's cotangent only.

With FE_SMOKE_PARITY_OUT set, every measured ratio `device error / err32` is appended to that file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import smoke_cases as SC  # noqa: E402
import smoke_numpy  # noqa: E402  (smoke_cases puts oracle/ on the path)

pytestmark = pytest.mark.gpu
U, MARGIN = SC.U, 4.0
PATTERNS = ('dense', 'v-at-walls', 'q-only')
GROUPS = (('translation', slice(0, 3)), ('rotation', slice(3, 6)), ('strength', slice(6, 7)), ('radius', slice(7, 8)))
DRAWS = 8                            # err32 draws behind the yardstick of an action-gradient group (module docstring)
_cache = {}


def _record(test, case, field, err, err32, bound):
    path = os.environ.get('FE_SMOKE_PARITY_OUT')
    if path:
        ratio = err / err32 if err32 > 0 else (0.0 if err == 0 else float('inf'))
        with open(path, 'a') as fh:
            fh.write(f'{test:9s} {case:13s} {field:24s} err {err:.3e} err32 {err32:.3e} ratio {ratio:7.3f} bound {bound:.3e}\n')


def _yardstick(test, case, field, dev, o32, o64, failures):
    """max|dev - o64| <= max(4 max|o32 - o64|, 4 u max|o64|); collects a failure instead of raising so that every field is recorded"""
    err, err32 = float(np.abs(dev - o64).max(initial=0.0)), float(np.abs(o32 - o64).max(initial=0.0))
    bound = max(MARGIN * err32, MARGIN * U * float(np.abs(o64).max(initial=0.0)))
    _record(test, case, field, err, err32, bound)
    if not err <= bound:
        failures.append((case, field, 'err', err, 'err32', err32, 'bound', bound))


def _free(name):
    if ('free', name) not in _cache:
        _cache['free', name] = SC.free_mask(SC.CASES[name])
    return _cache['free', name]


def _cots(name, draws=1):
    """the three patterns of the test's cotangent, then those of the further draws"""
    out = []
    for k in range(draws):
        c = SC.cotangents(SC.CASES[name], _free(name), seed=3 + 10 * k)
        out += [c[p] for p in PATTERNS]
    return out


def _one_step(lib, tag, name):
    """one step forward and the adjoints (the device: the test's three cotangents; the oracles: all DRAWS of them), computed once per
    (engine, case) and shared; never modified"""
    if (tag, name) not in _cache:
        _cache[tag, name] = SC.one_step(lib, SC.CASES[name], _cots(name, 1 if tag == 'hip' else DRAWS))
    return _cache[tag, name]


def _yardstick_drawn(test, case, field, dev, o32s, o64s, failures):
    """_yardstick with err32 the largest over the draws (o32s[0], o64s[0] belong to the cotangent the device ran)"""
    err = float(np.abs(dev - o64s[0]).max())
    err32 = max(float(np.abs(a - b).max()) for a, b in zip(o32s, o64s))
    bound = max(MARGIN * err32, MARGIN * U * float(np.abs(o64s[0]).max()))
    _record(test, case, field, err, err32, bound)
    if not err <= bound:
        failures.append((case, field, 'err', err, 'err32', err32, 'bound', bound))


def _abs_nb_sum(free, field):
    """sum over the six compute_location neighbours of |field|"""
    return sum(np.abs(smoke_numpy._nb(free, field, ax, sh)[0]) for ax in range(3) for sh in (-1, 1))


@pytest.mark.parametrize('name', SC.NAMES)
def test_smoke_hip_stages_forward(hiplib, oracle64, oracle32, name):
    """One step.  The free mask and what non-free cells hold, exactly; divergence (m = 6), the Jacobi sweeps (m = 7 per sweep; the
    averaging is non-expansive in max-norm, so the sweeps' bounds add up) and the gradient subtraction (m = 3) against the fp64 stage
    applied to the device's own input; advection (v_tmp and each column of q) against the fp64 oracle with the err32 yardstick."""
    case, free = SC.CASES[name], _free(name)
    d, o64, o32 = _one_step(hiplib, 'hip', name), _one_step(oracle64, 'o64', name), _one_step(oracle32, 'o32', name)
    v0, q0, p0 = SC.inputs(case)
    nf = ~free
    # ---- exact facts
    assert ((d['v_tmp'] != 0).any(-1) == free).all()
    assert (d['v_tmp'][nf] == 0).all() and (d['v1'][nf] == 0).all()
    assert (d['q1'][nf] == q0[nf]).all()
    assert (d['p1'][nf] == 0).all()                                  # frame 1 was zero before the step and non-free cells are not written
    assert (d['div'][nf] == 0).all()
    if name == 'empty':
        for k in ('v_tmp', 'div', 'v1', 'q1', 'p1'):
            assert (d[k] == o64[k]).all() and (d[k] == o32[k]).all(), k
    # ---- divergence from the device's v_tmp: 0.5 (sum of six +-values), m = 6
    lo_hi = 0.0
    for ax in range(3):
        for sh in (-1, 1):
            val, isfree = smoke_numpy._nb(free, d['v_tmp'], ax, sh)
            lo_hi = lo_hi + np.abs(np.where(isfree, val[..., ax], d['v_tmp'][..., ax]))
    ref = smoke_numpy.divergence(d['v_tmp'], free)
    bound = 2 * 6 * U * 0.5 * lo_hi
    assert (np.abs(d['div'] - ref)[free] <= bound[free]).all(), ('div', np.abs(d['div'] - ref).max(), bound.max())
    # ---- the sweeps from the device's div and p[0]: (sum of six - div) / 6, m = 7 per sweep
    cur, total = np.where(free, p0, 0.0), 0.0
    for _ in range(case['iters']):
        total += (2 * 7 * U * (_abs_nb_sum(free, cur) + np.abs(d['div'])) / 6.0)[free].max(initial=0.0)
        cur = smoke_numpy.jacobi(cur, d['div'], free, 1)
    assert np.abs(d['p1'] - cur)[free].max(initial=0.0) <= total, ('p', np.abs(d['p1'] - cur)[free].max(), total)
    # ---- subtraction from the device's v_tmp and p[1]: v_tmp - 0.5 (p_hi - p_lo), m = 3
    ref = smoke_numpy.subtract(d['v_tmp'], d['p1'], free)
    terms = np.stack([np.abs(d['v_tmp'][..., ax]) + 0.5 * (np.abs(smoke_numpy._nb(free, d['p1'], ax, 1)[0]) + np.abs(smoke_numpy._nb(free, d['p1'], ax, -1)[0]))
                      for ax in range(3)], -1)
    assert (np.abs(d['v1'] - ref) <= 2 * 3 * U * terms).all(), ('v', np.abs(d['v1'] - ref).max())
    # ---- advection against the fp64 oracle
    failures = []
    _yardstick('stages', name, 'v_tmp', d['v_tmp'], o32['v_tmp'], o64['v_tmp'], failures)
    for c in range(case['q_dim']):
        _yardstick('stages', name, f'q[1][{c}]', d['q1'][..., c], o32['q1'][..., c], o64['q1'][..., c], failures)
    assert not failures, failures


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('name', SC.NAMES)
def test_smoke_hip_adjoint_one_step(hiplib, oracle64, oracle32, name, pattern):
    """The adjoint of one step against the fp64 oracle with the err32 yardstick, per field: v.grad[0], each column of q.grad[0], and the
    action gradient per component group, each against its own magnitude.  Three cotangents so that no term hides behind a larger
    one: dense; v only, on the cells at walls, at obstacles and outside the slab; q only.  `no-sweeps` has nothing flowing through
    div (subtract and advect adjoints alone), `q2-one-sweep` one transposed Jacobi sweep."""
    case = SC.CASES[name]
    i = PATTERNS.index(pattern)
    d = _one_step(hiplib, 'hip', name)['grads'][i]
    o64s, o32s = (_one_step(lib, tag, name)['grads'][i::len(PATTERNS)] for lib, tag in ((oracle64, 'o64'), (oracle32, 'o32')))
    o64, o32 = o64s[0], o32s[0]
    failures = []
    tag = f'adj/{pattern[0]}'
    _yardstick(tag, name, 'gv[0]', d['gv0'], o32['gv0'], o64['gv0'], failures)
    for c in range(case['q_dim']):
        _yardstick(tag, name, f'gq[0][{c}]', d['gq0'][..., c], o32['gq0'][..., c], o64['gq0'][..., c], failures)
    for gname, sl in GROUPS:
        _yardstick_drawn(tag, name, f'action {gname}', d['action'][sl], [o['action'][sl] for o in o32s], [o['action'][sl] for o in o64s], failures)
    if _free(name).any():                                            # q depends on the AirCon's place and radius only
        live = GROUPS if pattern != 'q-only' else (GROUPS[0], GROUPS[3])
        assert all(np.abs(o64['action'][sl]).max() > 0 for _, sl in live)
    assert not failures, failures


@pytest.mark.parametrize('name', ['q3', 'walls', 'pocket', 'fast-walls'])
def test_smoke_hip_three_steps(hiplib, oracle64, oracle32, name):
    """three steps end to end with a moving, turning AirCon: v, q (per column) and p of the last frame, err32 yardstick"""
    case = SC.CASES[name]
    acts = SC.actions(3)
    d, o64, o32 = (SC.run_steps(lib, case, acts)['final'] for lib in (hiplib, oracle64, oracle32))
    failures = []
    for k in ('v', 'p'):
        _yardstick('3 steps', name, k, d[k], o32[k], o64[k], failures)
    for c in range(case['q_dim']):
        _yardstick('3 steps', name, f'q[{c}]', d['q'][..., c], o32['q'][..., c], o64['q'][..., c], failures)
    assert not failures, failures


SENTINEL = 7.25


def _sentinel_step(lib, case):
    eng, e = SC.make_engine(lib, case, action_steps=1, set_inputs=False)
    n, qd = case['res'], case['q_dim']
    full = dict(v=np.full((n, n, n, 3), SENTINEL), v_tmp=np.full((n, n, n, 3), SENTINEL), div=np.full((n, n, n), SENTINEL),
                p=np.full((n, n, n), SENTINEL), q=np.full((n, n, n, qd), SENTINEL))
    eng.smoke_set_frame(0, **full)
    eng.smoke_set_frame(1, **full)
    v0, q0, p0 = SC.inputs(case)
    eng.smoke_set_frame(0, v=v0, q=q0, p=p0)
    eng.eff_set_action(e, 0, 0, 2, SC.actions(1)[0])
    eng.step(0, 0, 1, 1)
    eng.smoke_step(0, 1)
    f0, f1 = SC.as64(eng.smoke_get_frame(0, ('v_tmp', 'div'))), SC.as64(eng.smoke_get_frame(1, ('v', 'q', 'p')))
    eng.close()
    return {'v_tmp[0]': f0['v_tmp'], 'div[0]': f0['div'], 'v[1]': f1['v'], 'q[1]': f1['q'], 'p[1]': f1['p']}


@pytest.mark.parametrize('name', ['base', 'beyond', 'empty'])
def test_smoke_hip_step_writes_what_the_oracle_writes(hiplib, oracle64, oracle32, name):
    """Frames that already hold data (set_state at s > 0, a reused ring slot): with every field of frames 0 and 1 filled with a
    sentinel, one step must overwrite the same cells per field on the device as on the oracle -- v_tmp[s] and v[s+1] are written
    (with 0) on every cell outside the free space, q[s+1] everywhere, div[s] and p[s+1] on free cells only -- with the same values."""
    case = SC.CASES[name]
    d, o64, o32 = (_sentinel_step(lib, case) for lib in (hiplib, oracle64, oracle32))
    failures = []
    for k in d:
        wd, wo = d[k] != SENTINEL, o64[k] != SENTINEL
        if not (wd == wo).all():
            failures.append((k, 'cells written on the device only', int((wd & ~wo).sum()), 'on the oracle only', int((wo & ~wd).sum())))
            continue
        _yardstick('writes', name, k, d[k][wo], o32[k][wo], o64[k][wo], failures)
    assert not failures, failures


def _ring(lib, case, cot_v, cot_q):
    """Four steps through a smoke ring of two frames, forward and backward, in the host's order (MPMSimulator.memory_to_cache /
    memory_from_cache): after the chunk's last step copy_frame(S, 0); backward, copy_frame(0, S), copy_grad(0, S),
    reset_grad_till_frame(S), frame 0 restored from the checkpoint and the earlier chunk stepped again.  The effector's and the
    particles' rings hold all four steps: the smoke ring alone is under test."""
    S_, G = 2, 4
    eng, e = SC.make_engine(lib, case, action_steps=G, max_steps_local=S_)
    acts = SC.actions(G)
    ckpt = eng.smoke_get_frame(0, SC.FIELDS)
    fields = []
    for g in range(G):
        s = g % S_
        if g and s == 0:
            eng.smoke_copy_frame(S_, 0)
        eng.eff_set_action(e, g, g, 2, acts[g])
        eng.smoke_step(s, 2 * g)
        eng.step(2 * g, 2 * g, 2, 1)
        fields.append(SC.as64(eng.smoke_get_frame(s + 1, ('v', 'q', 'p'))))
    eng.reset_grad()
    eng.smoke_add_grad(S_, gv=cot_v, gq=cot_q)
    for g in reversed(range(G)):
        s = g % S_
        if s == S_ - 1 and g != G - 1:
            eng.smoke_copy_frame(0, S_)
            eng.smoke_copy_grad(0, S_)
            eng.smoke_reset_grad_till_frame(S_)
            eng.smoke_set_frame(0, **ckpt)
            for g2 in range(g - S_ + 1, g + 1):
                eng.smoke_step(g2 % S_, 2 * g2)
        eng.step_grad(2 * g, 2 * g, 2, 1)
        eng.smoke_step_grad(s, 2 * g)
        eng.eff_set_action_grad(e, g, g, 2)
    gv0, gq0 = eng.smoke_get_grad(0)
    out = dict(fields=fields, gv0=gv0.astype(np.float64), gq0=gq0.astype(np.float64), action=eng.eff_get_action_grad(e, 0, G, 8)[:G].astype(np.float64))
    eng.close()
    return out


@pytest.mark.parametrize('name', ['base', 'q3'])
def test_smoke_hip_frame_ring(hiplib, oracle64, oracle32, name):
    """stepping into frames that already hold data, and the adjoint carried across the chunk boundary by copy_grad and
    reset_grad_till_frame: fields after each of four steps, adjoints at the start and the action gradient per step and group"""
    case = SC.CASES[name]
    cots = [SC.cotangents(case, _free(name), seed=3 + 10 * k)['dense'] for k in range(DRAWS)]
    d = _ring(hiplib, case, *cots[0])
    o64s, o32s = ([_ring(lib, case, *c) for c in cots] for lib in (oracle64, oracle32))
    o64, o32 = o64s[0], o32s[0]
    failures = []
    for g in range(4):
        for k in ('v', 'p'):
            _yardstick('ring', name, f'step {g} {k}', d['fields'][g][k], o32['fields'][g][k], o64['fields'][g][k], failures)
        for c in range(case['q_dim']):
            _yardstick('ring', name, f'step {g} q[{c}]', d['fields'][g]['q'][..., c], o32['fields'][g]['q'][..., c], o64['fields'][g]['q'][..., c], failures)
    _yardstick('ring', name, 'gv[0]', d['gv0'], o32['gv0'], o64['gv0'], failures)
    for c in range(case['q_dim']):
        _yardstick('ring', name, f'gq[0][{c}]', d['gq0'][..., c], o32['gq0'][..., c], o64['gq0'][..., c], failures)
    for g in range(4):
        for gname, sl in GROUPS:
            _yardstick_drawn('ring', name, f'action {g} {gname}', d['action'][g, sl], [o['action'][g, sl] for o in o32s],
                             [o['action'][g, sl] for o in o64s], failures)
    assert np.abs(o64['action']).min(0).max() > 0 and np.abs(o64['gv0']).max() > 0
    assert not failures, failures
