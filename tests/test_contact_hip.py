"""fe_contact_wrench on the GPU (include/fluidengine_ext.h, fluidlab_amd/csrc/fe_contact.h): what the replay reports against what the forward
pass did -- twin runs with the colliders switched off, the momentum identity of the B-spline gather, the fp64 restatement tests/contact_ref.py --
and the call's contract.  Every test asserts valid == 1 on the frames it judges.

Bounds.  The twin tests use the derived bound of the issue: the kernel's gather may sum its 27 products in another order than g2p, so a
contact's velocities differ by at most 27 * 2^-23 * max |v_out| per axis; summed over the contacts with their masses (times |r| for the angular
part).  max |v_out| comes from the restatement.  The restatement tests use a tolerance measured once on an MI355X
(profiles/contact_wrench_parity.txt) and asserted at four times the measured value."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_ref as R  # noqa: E402
import scenarios as S  # noqa: E402

from fluidlab_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

VARIANTS = dict(friction=dict(friction=0.5, softness=0.0), soft=dict(friction=0.1, softness=60.0), sticky=dict(friction=20.0, softness=0.0))
GATHER = 27 * 2.0 ** -23                      # relative rounding of a 27-term fp32 sum of products, either order
# Measured on an MI355X (profiles/contact_wrench_parity.txt, written by the two restatement tests with FE_CONTACT_PARITY_OUT set): the largest
# |engine - restatement| / sum |m dv| over the records of the two statics of water_on_obstacles, impulse and angular impulse alike, and over the
# effector's record of frame 1 of the re-sorted stirrer: 8.973e-07 and 8.984e-07 in two runs (static 0's impulse; two rollouts of this engine
# differ in their last bits, test_contract).  Asserted at four times the larger.
MEASURED_REL = 8.984e-07
PARITY_TOL = 4 * MEASURED_REL


def mass64(sc):
    """the engine's fp32 mass p_vol * rho per particle, widened"""
    rho = np.array([S.MATERIALS[int(m)][2] for m in sc['mat']], np.float64)
    return S.f32((0.5 / sc['n_grid']) ** 2 * rho).astype(np.float64)


def lam64(sc):
    return S.f32([S.MATERIALS[int(m)][1] for m in sc['mat']]).astype(np.float64)


def rigid_engine(hiplib, sc, options=None):
    """make_engine + the Rigid effector of run_rigid, actions of step 0 set; returns (engine, effector)"""
    eng = S.make_engine(hiplib, sc, options=options)
    r = sc['rigid']
    e = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=r['action_dim'], action_scale_v=r['action_scale_v'], action_scale_p=r['action_scale_p'],
                         boundary=hiplib.make_boundary(**r['boundary']))
    eng.eff_set_mesh(e, r['voxels'], r['T'], friction=r['friction'], softness=r['softness'])
    if 'collide_type' in sc:
        eng.set_option('collide_type', sc['collide_type'])
    st0 = eng.eff_get_state(e, 0)
    st0[:7] = r['init_state']
    eng.eff_set_state(e, 0, st0)
    eng.eff_apply_action_p(e, sc['action_p'])
    return eng, e


def run_steps(eng, e, sc, n_steps):
    ns = sc['n_substeps']
    for s in range(n_steps):
        eng.eff_set_action(e, s, s, ns, sc['actions'][s])
        eng.step(s * ns, s * ns, ns, 1)


def first_substep(eng, e, sc):
    eng.eff_set_action(e, 0, 0, sc['n_substeps'], sc['actions'][0])
    eng.step(0, 0, 1, 1)


def dyn_of(sc, eng, e, f):
    """the effector's collider in substep f as contact_ref takes it"""
    r, p0, p1 = sc['rigid'], eng.eff_get_state(e, f).astype(np.float64), eng.eff_get_state(e, f + 1).astype(np.float64)
    return dict(voxels=r['voxels'].astype(np.float64), T=r['T'], friction=float(np.float32(r['friction'])), softness=float(np.float32(r['softness'])),
                pos0=p0[:3], quat0=p0[3:7], pos1=p1[:3], quat1=p1[3:7])


def reference(sc, st, dynamics=(), collide_type=1, statics=()):
    """contact_ref on a downloaded frame (fp32 words, widened)"""
    return R.contact_ref(*[st[k].astype(np.float64) for k in 'xvCF'], st['used'], mass64(sc), lam64(sc), sc['n_grid'], sc['dt'], (0.5 / sc['n_grid']) ** 2,
                         S.f32(sc['gravity']).astype(np.float64), sc['boundary'], statics=statics, dynamics=dynamics, collide_type=collide_type)


def twin_momentum(sc, a, b):
    """sum_p m_p (v1_with - v1_free) and its moment about the origin at x_p + dt v1_free_p, fp64; the differing particles"""
    m = mass64(sc)
    dv = a['v'].astype(np.float64) - b['v'].astype(np.float64)
    diff = (dv != 0).any(1) & (a['used'] != 0)
    J = m[:, None] * dv
    r = b['x0'].astype(np.float64) + sc['dt'] * b['v'].astype(np.float64)
    return J[diff].sum(0), np.cross(r[diff], J[diff]).sum(0), diff, r, J


def one_record(eng, f=0):
    rec = eng.contact_wrench(f, 1)
    assert rec.shape[0] == 1 and (rec['valid'] == 1).all(), rec['valid']
    return rec[0]


@pytest.mark.parametrize('variant', ['friction', 'soft', 'sticky', 'two_materials'])
def test_twin_run_particle_level(hiplib, variant):
    sc = S.stirrer_mini(shape='sphere', **VARIANTS['friction' if variant == 'two_materials' else variant])
    sc['collide_type'] = 1
    if variant == 'two_materials':                                # water and milk (half the density): the mass comes from the particle's own record
        sc['mat'] = np.where(np.arange(sc['N']) % 2 == 0, S.WATER, S.MILK).astype(np.int32)
    out = []
    for opts in ({}, {'collide_min_y': 1e30}):
        eng, e = rigid_engine(hiplib, sc, options=opts)
        st0 = S.get_state(eng, 0)
        first_substep(eng, e, sc)
        st1 = S.get_state(eng, 1)
        st1['x0'] = st0['x']
        if not opts:
            rec = one_record(eng)[0]
            dyn = dyn_of(sc, eng, e, 0)
        eng.close()
        out.append(st1)
        st_first = st0
    a, b = out
    _, _, diff, r, Jp = twin_momentum(sc, a, b)
    m = mass64(sc)
    # max |v_out| from the restatement of frame 0 (collide_type 1: the colliders do not touch the grid)
    _, info = reference(sc, st_first)
    vmax = np.abs(info['v_out']).max()
    per = m * GATHER * vmax                                     # per contact and axis
    # The contacts.  Two rollouts of this engine do not run the same substep to the same bits (test_contract), so nearly every particle
    # "differs" between the twins by rounding; the sums and the bound run over the contacts only: the particles whose difference is above
    # the per-contact bound, and those the restatement puts into the contact branch (a separating contact changes nothing, or an ulp).
    big = diff & (np.abs(Jp).max(1) > per)
    pos = st_first['x'].astype(np.float64) + sc['dt'] * b['v'].astype(np.float64)
    hit, _ = R.dynamic_hit(dyn, pos)
    contacts = (big | hit) & (a['used'] != 0)
    J, L = Jp[contacts].sum(0), np.cross(r[contacts], Jp[contacts]).sum(0)
    bound = per[contacts].sum()                                 # sum over contacts of m_p * 27 * 2^-23 * max |v_out|
    bound_ang = (per[contacts] * np.linalg.norm(r[contacts], axis=1)).sum()
    err, err_ang = np.abs(rec['impulse'] - J).max(), np.abs(rec['ang_impulse'] - L).max()
    print(f'\n[{variant}] differing {int(diff.sum())} contacts {int(contacts.sum())} n_particles {int(rec["n_particles"])} |dJ| {err:.3e} (bound {bound:.3e}) '
          f'|dL| {err_ang:.3e} (bound {bound_ang:.3e})')
    assert rec['kind'] == 0 and rec['n_nodes'] == 0
    assert err <= bound and err_ang <= bound_ang
    # the count: every particle whose difference is above the bound is a contact; beyond those only particles that the restatement puts
    # into the contact branch can be counted
    assert big.sum() > 20 and big.sum() <= rec['n_particles'] <= contacts.sum(), (big.sum(), contacts.sum(), rec['n_particles'])
    assert np.array_equal(rec['ref'], dyn['pos0'])                # the effector's position words at frame 0


def _stencils_inside_boundary(sc, x):
    """every particle's 27 nodes lie where boundary_v multiplies by one: strictly inside the cube boundary"""
    n = sc['n_grid']
    base = (x.astype(np.float64) * n - 0.5).astype(int)
    lo, hi = base.min(0) / n, (base.max(0) + 2) / n
    assert (lo > np.asarray(sc['boundary']['lower'])).all() and (hi < np.asarray(sc['boundary']['upper'])).all(), (lo, hi)


def test_momentum_identity_statics(hiplib):
    sc = S.water_on_obstacles()
    free = dict(sc); free.pop('statics')
    out = []
    for s in (sc, free):
        eng = S.make_engine(hiplib, s)
        st0 = S.get_state(eng, 0)
        eng.step(0, 0, 1, 0)
        st1 = S.get_state(eng, 1)
        st1['x0'] = st0['x']
        if s is sc:
            rec = one_record(eng)
            assert eng.contact_count() == 2
        else:
            assert eng.contact_count() == 0
        eng.close()
        out.append(st1)
    _stencils_inside_boundary(sc, st0['x'])
    a, b = out
    m = mass64(sc)
    J = (m[:, None] * (a['v'].astype(np.float64) - b['v'].astype(np.float64))).sum(0)
    _, info = reference(sc, st0, statics=sc['statics'])
    _, info_free = reference(sc, st0)
    vmax = max(np.abs(info['v_out']).max(), np.abs(info_free['v_out']).max())
    bound = (m * GATHER * vmax).sum()                           # every particle counted
    got = rec['impulse'].sum(0)
    print(f'\n[statics] n_nodes {rec["n_nodes"]} |sum impulse - dp| {np.abs(got - J).max():.3e} (bound {bound:.3e}) |dp| {np.abs(J).max():.3e}')
    assert (rec['kind'] == 1).all() and (rec['n_nodes'] > 0).all() and (rec['n_particles'] == 0).all() and not rec['ref'].any()
    assert np.abs(got - J).max() <= bound


@pytest.mark.parametrize('collide_type', [2, 3])
def test_momentum_identity_effector_at_nodes(hiplib, collide_type):
    sc = S.stirrer_mini(shape='sphere', friction=0.5, softness=0.0)
    sc['collide_type'] = collide_type
    out = []
    for opts in ({}, {'collide_min_y': 1e30}):                    # (switches both levels off)
        eng, e = rigid_engine(hiplib, sc, options=opts)
        st0 = S.get_state(eng, 0)
        first_substep(eng, e, sc)
        st1 = S.get_state(eng, 1)
        if not opts:
            rec = one_record(eng)[0]
            dyn = dyn_of(sc, eng, e, 0)
        eng.close()
        out.append(st1)
    _stencils_inside_boundary(sc, st0['x'])
    a, b = out
    m = mass64(sc)
    J = (m[:, None] * (a['v'].astype(np.float64) - b['v'].astype(np.float64))).sum(0)
    _, info = reference(sc, st0, dynamics=[dyn], collide_type=collide_type)
    _, info_free = reference(sc, st0)
    vmax = max(np.abs(info['v_out']).max(), np.abs(info_free['v_out']).max())
    bound = (m * GATHER * vmax).sum()
    print(f'\n[collide_type {collide_type}] n_particles {rec["n_particles"]} n_nodes {rec["n_nodes"]} |impulse - dp| {np.abs(rec["impulse"] - J).max():.3e} '
          f'(bound {bound:.3e}) |dp| {np.abs(J).max():.3e}')
    assert rec['n_nodes'] > 0 and (rec['n_particles'] > 0) == (collide_type == 3)
    assert np.abs(rec['impulse'] - J).max() <= bound


def _rel_errors(rec, ref):
    den = ref['abs_impulse']
    return np.abs(rec['impulse'] - ref['impulse']).max() / den, np.abs(rec['ang_impulse'] - ref['ang_impulse']).max() / den


def test_statics_separately_against_the_restatement(hiplib):
    sc = S.water_on_obstacles()
    eng = S.make_engine(hiplib, sc)
    st0 = S.get_state(eng, 0)
    eng.step(0, 0, 1, 0)
    rec = one_record(eng)
    eng.close()
    refs, info = reference(sc, st0, statics=sc['statics'])
    lines = []
    for s, (st, ref) in enumerate(zip(sc['statics'], refs)):
        # no node with mass within 1e-4 voxels of the surface: fp32 cannot put it on the other branch
        sd_vox = np.abs(R.static_sd(st, info['node_x'])) * np.asarray(st['T'])[0, 0]
        assert sd_vox.min() >= 1e-4, (s, sd_vox.min())
        ej, el = _rel_errors(rec[s], ref)
        lines.append(f'static {s}: n_nodes {int(rec["n_nodes"][s])} (restatement {ref["n_nodes"]}) impulse rel err {ej:.3e} ang_impulse rel err {el:.3e} sum|m dv| {ref["abs_impulse"]:.3e}')
        assert rec['n_nodes'][s] == ref['n_nodes'] > 0
    print('\n' + '\n'.join(lines))
    if os.environ.get('FE_CONTACT_PARITY_OUT'):
        with open(os.environ['FE_CONTACT_PARITY_OUT'], 'a') as f:
            f.write('water_on_obstacles, substep 0, |engine - restatement| / sum |m dv| per record\n' + '\n'.join(lines) + '\n')
    for s, ref in enumerate(refs):
        ej, el = _rel_errors(rec[s], ref)
        assert ej <= PARITY_TOL and el <= PARITY_TOL, (s, ej, el)


def test_frame_in_an_older_particle_order(hiplib):
    sc = S.stirrer_mini(shape='sphere', friction=0.5, softness=0.0)
    eng, e = rigid_engine(hiplib, sc, options={'sort_interval': 3})
    run_steps(eng, e, sc, 2)                                      # 8 substeps: sorts at 0, 3, 6 -- frame 1's table is not the current one
    whole = eng.contact_wrench(1, 7)
    single = np.concatenate([eng.contact_wrench(f, 1) for f in range(1, 8)])
    assert whole.shape == (7, 1) and whole.tobytes() == single.tobytes()
    assert whole['valid'][0, 0] == 1 and whole['valid'][6, 0] == 1, whole['valid'].ravel()
    assert whole['n_particles'][0, 0] > 20 and whole['n_particles'][6, 0] > 20
    st1 = S.get_state(eng, 1)
    dyn = dyn_of(sc, eng, e, 1)
    assert np.array_equal(whole['ref'][0, 0], eng.eff_get_state(e, 1)[:3].astype(np.float64))
    eng.close()
    refs, _ = reference(sc, st1, dynamics=[dyn], collide_type=1)
    ej, el = _rel_errors(whole[0, 0], refs[0])
    line = (f'stirrer_mini sort_interval 3, frame 1: n_particles {int(whole["n_particles"][0, 0])} (restatement {refs[0]["n_particles"]}) '
            f'impulse rel err {ej:.3e} ang_impulse rel err {el:.3e} nearest particle to the surface {refs[0]["min_abs_sd"]:.3e}')
    print('\n' + line)
    if os.environ.get('FE_CONTACT_PARITY_OUT'):
        with open(os.environ['FE_CONTACT_PARITY_OUT'], 'a') as f:
            f.write(line + '\n')
    assert ej <= PARITY_TOL and el <= PARITY_TOL, (ej, el)


def _xvC(eng, f):
    """x, v, C and used of frame f (no F: that download would expand a compactly stored one)"""
    N = eng.N
    x, v, C_, u = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32), np.zeros((N, 3, 3), np.float32), np.zeros(N, np.int32)
    eng.get_frame(f, x, v, C_, None, u)
    return x, v, C_, u


N_PLAIN = 4                                                  # plain rollouts whose pairwise distances are the measure of the engine's own noise
NOISE_ULPS = {'x': 5e-7, 'v': 4e-6, 'C': 8e-5, 'F': 4e-6}     # what tests/test_hip_parity.py allows one pair of runs beyond the measured noise (of the field's range)


def _rollout(hiplib, sc, with_calls, n_steps=3):
    """every frame of n_steps steps of the stirrer scene, downloaded at the end; with_calls: a wrench call after every step"""
    eng, e = rigid_engine(hiplib, sc)
    ns = sc['n_substeps']
    for s in range(n_steps):
        eng.eff_set_action(e, s, s, ns, sc['actions'][s])
        eng.step(s * ns, s * ns, ns, 1)
        if with_calls:
            rec = eng.contact_wrench(s * ns, ns)
            assert (rec['valid'] == 1).all() and rec['n_particles'].sum() > 0 and rec['n_nodes'].sum() > 0
    frames = [S.get_state(eng, f) for f in range(n_steps * ns + 1)]
    eng.close()
    return frames


def _first_difference(a, b):
    """(frame, text) of the first word in which two rollouts differ, or (len, None)"""
    for f, (p, q) in enumerate(zip(a, b)):
        for k in ('x', 'v', 'C', 'F', 'used'):
            n = int((p[k].view(np.uint32) != q[k].view(np.uint32)).sum())
            if n:
                return f, f'frame {f} {k}: {n} words'
    return len(a), None


def _apart(a, b, k, u):
    """largest difference of field k over the used particles of one frame, relative to the field's range (as tests/test_hip_parity.py measures it)"""
    p, q = a[k][u].astype(np.float64), b[k][u].astype(np.float64)
    return float(np.abs(p - q).max()) / max(1.0, float(np.abs(q).max()))


def test_rollout_with_calls_against_rollouts_without(hiplib):
    """The issue's check: a rollout with a wrench call after every step ends in the same frames as one without.  The engine itself is not
    bit-reproducible from run to run (tests/test_hip_parity.py, tests/test_render_hip.py; profiles/contact_wrench_parity.txt: two rollouts of
    this scene without any contact call differ in the velocity words of 1,230 of 1,500 particles after one substep).  So, as
    tests/test_render_hip.py does for the pictures, the plain rollout runs several times (N_PLAIN) and between the rollout with calls and the plain one there is
    always an assertion:
      - every frame up to the first one in which two plain runs differ is equal word for word (where they agree throughout, every frame);
      - beyond that, `used` is equal in every frame and x, v, C, F lie no farther from the first plain run than 4 x what the farthest two
        plain runs lie apart in that frame (in a scene with contact a particle that falls on the other side of a surface is a jump, not an
        ulp: one pair of runs is too small a sample of that -- measured, 1.3e-6 of the range of v between one pair and 1.1e-5 between another), plus the few ulp of the field's range test_hip_parity.py allows for one pair of runs being a small sample of
        the noise (NOISE_ULPS).  A call that disturbed a store word, a working grid, a stamp or a sort key shows in the later frames."""
    sc = S.stirrer_mini(shape='sphere', friction=0.5, softness=0.0)
    sc['collide_type'] = 3
    with_calls = _rollout(hiplib, sc, True)
    plains = [_rollout(hiplib, sc, False) for _ in range(N_PLAIN)]
    plain = plains[0]
    n = len(plain)
    assert len(with_calls) == n == 13 and all(len(q) == n for q in plains)
    f_noise, noise = min((_first_difference(plain, q) for q in plains[1:]), key=lambda t: t[0])
    f_diff, diff = _first_difference(plain, with_calls)
    print(f'\nplain against plain: first difference {noise}; plain against the rollout with calls: first difference {diff}')
    assert f_noise >= 1, noise                                    # the frame both start from
    assert f_diff >= f_noise, (diff, noise)                       # equal wherever the plain runs are equal
    worst, env = {k: 0.0 for k in 'xvCF'}, {k: 0.0 for k in 'xvCF'}
    for f in range(f_noise, n):
        r, p = with_calls[f], plain[f]
        assert all(np.array_equal(q[f]['used'], p['used']) for q in plains[1:] + [with_calls]), f
        u = p['used'] != 0
        for k in 'xvCF':
            d = _apart(r, p, k, u)
            nz = max(_apart(plains[i][f], plains[j][f], k, u) for i in range(N_PLAIN) for j in range(i))
            worst[k], env[k] = max(worst[k], d), max(env[k], nz)
            assert d <= 4.0 * nz + NOISE_ULPS[k], (f, k, d, nz)
    print('with calls against plain, largest relative difference', {k: float(f'{v:.2g}') for k, v in worst.items()}, 'plain against plain', {k: float(f'{v:.2g}') for k, v in env.items()})


def test_contract(hiplib):
    """The rest of the contract.  Beside the comparison of whole rollouts (test_rollout_with_calls_against_rollouts_without): two evaluations
    give the same bytes; the call leaves every frame of the window as it was, bit for bit (x, v, C, used; F is not downloaded, that would
    expand a compact one); the rollout goes on with the launches of one without calls (the engine's per-kernel launch counts); which frames
    are valid; the error cases; an engine without colliders."""
    sc = S.stirrer_mini(shape='sphere', friction=0.5, softness=0.0)
    sc['collide_type'] = 3
    ns = sc['n_substeps']
    eng, e = rigid_engine(hiplib, sc)
    plain, e_plain = rigid_engine(hiplib, sc)
    L = sc['max_substeps_local']
    for en in (eng, plain):
        en.profile_enable(True)
    for s in range(3):
        for en, ef in ((eng, e), (plain, e_plain)):
            en.eff_set_action(ef, s, s, ns, sc['actions'][s])
            en.step(s * ns, s * ns, ns, 1)
        before = [_xvC(eng, f) for f in range(L + 1)]
        r1, r2 = eng.contact_wrench(s * ns, ns), eng.contact_wrench(s * ns, ns)
        # two evaluations give the same bytes
        assert r1.tobytes() == r2.tobytes() and (r1['valid'] == 1).all() and r1['n_particles'].sum() > 0 and r1['n_nodes'].sum() > 0
        for f, fa in enumerate(before):                           # every frame of the window was only read
            assert all(p.tobytes() == q.tobytes() for p, q in zip(fa, _xvC(eng, f))), f
        for f in range(L + 1):                                    # (the other engine's host does the same downloads)
            _xvC(plain, f)
    launches = [{k: n for k, (ms, n) in en.profile_read().items()} for en in (eng, plain)]
    assert launches[0] == launches[1] and sum(launches[0].values()) > 0, launches
    plain.close()
    # fe_set_frame on frame f makes that frame valid == 0, and no other
    eng.set_frame(5, x=S.get_state(eng, 5)['x'])
    v = eng.contact_wrench(4, 3)['valid'].ravel()
    assert list(v) == [1, 0, 1], v
    zero = eng.contact_wrench(5, 1)[0, 0]
    assert not zero['impulse'].any() and not zero['ang_impulse'].any() and not zero['ref'].any() and zero['n_particles'] == 0 == zero['n_nodes'] and zero['kind'] == 0
    # every error case returns non-zero and leaves `out` untouched
    out = np.full((2, 1), 7, _capi.CONTACT_DTYPE)
    keep = out.tobytes()
    size = _capi.CONTACT_DTYPE.itemsize
    for args in ((-1, 1, 1, size), (0, 0, 1, size), (L - 1, 2, 1, size), (0, 1, 1, size - 8), (0, 1, 0, size), (L, 1, 1, size)):
        rc = eng.lib.fe_contact_wrench(eng.h, args[0], args[1], out.ctypes.data_as(ctypes.c_void_p), args[2], args[3])
        assert rc != 0 and eng.lib.fe_last_error(eng.h) and out.tobytes() == keep, args
    assert eng.lib.fe_contact_wrench(eng.h, L - 1, 1, out.ctypes.data_as(ctypes.c_void_p), 1, size) == 0      # (the last substep of the window is a legal one)
    assert out['valid'][0, 0] == 0                                # ... that was never computed
    eng.close()
    # grid_store = 0: valid == 0 and zeros
    eng, e = rigid_engine(hiplib, sc, options={'grid_store': 0})
    run_steps(eng, e, sc, 1)
    rec = eng.contact_wrench(0, sc['n_substeps'])
    assert (rec['valid'] == 0).all() and not rec['impulse'].any() and not rec['ang_impulse'].any() and (rec['n_particles'] == 0).all() and (rec['n_nodes'] == 0).all()
    eng.close()
    # no effector and no static: the count is 0 and the call succeeds writing nothing
    eng = S.make_engine(hiplib, S.water_block(n_grid=16, n_particles=500))
    eng.step(0, 0, 2, 0)
    assert eng.contact_count() == 0 and eng.contact_wrench(0, 2).shape == (2, 0)
    out = np.full((2,), 7, _capi.CONTACT_DTYPE)
    keep = out.tobytes()
    assert eng.lib.fe_contact_wrench(eng.h, 0, 2, out.ctypes.data_as(ctypes.c_void_p), 1, _capi.CONTACT_DTYPE.itemsize) == 0 and out.tobytes() == keep
    eng.close()


def _tool_env(renderer=None):
    """a mini Rigid scene: water at rest on the floor region of a 16^3 grid, an analytic cylinder driven through it"""
    from fluidlab_amd.configs.macros import STIRRER, WATER
    from fluidlab_amd.envs.fluid_env import FluidEnv
    from fluidlab_amd.fluidengine.meshes import sdf_cylinder
    from fluidlab_amd.utils.config import CfgNode

    class ToolEnv(FluidEnv):
        def __init__(self):
            super().__init__(loss=False, seed=0, dim=3, quality=0.25, particle_density=4e4, horizon=6, gravity=(0.0, -10.0, 0.0), max_substeps_local=None)

        def setup_agent(self):
            self.taichi_env.setup_agent(CfgNode(dict(type='AgentRigid', effectors=[dict(
                type='Rigid', params=dict(init_pos=(0.5, 0.32, 0.5), init_euler=(0.0, 0.0, 0.0), action_dim=6, action_scale_p=(1.0,) * 6, action_scale_v=(0.02,) * 6),
                mesh=dict(file='stirrer.obj', material=STIRRER, softness=0.0, sdf=sdf_cylinder(0.25, 0.5), sdf_res=40, scale=(0.3, 0.4, 0.3), euler=(0.0, 0.0, 0.0)),
                boundary=dict(type='cube', lower=(0.05, 0.05, 0.05), upper=(0.95, 0.95, 0.95)))])))

        def setup_boundary(self):
            self.taichi_env.setup_boundary(type='cube', lower=(0.05, 0.05, 0.05), upper=(0.95, 0.95, 0.95))

        def setup_bodies(self):
            self.taichi_env.add_body(type='cube', lower=(0.3, 0.1, 0.3), upper=(0.7, 0.3, 0.7), material=WATER)

        def _get_reward(self):
            return 0.0

    return ToolEnv()


def test_through_the_environment(hiplib):
    action = np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.0])             # the tool moves along +x, 0.02 per step
    env = _tool_env()
    assert env.taichi_env.n_particles <= 1500 and env.taichi_env.simulator.n_grid == 16
    plain = [env.step(action) for _ in range(2)]
    assert all('contact' not in info for _, _, _, info in plain)  # off by default
    w = env.taichi_env.contact_wrench()
    assert len(w) == 1 and w[0]['kind'] == 'effector' and w[0]['index'] == 0 and w[0]['coverage'] == 1.0 and w[0]['n_contacts'] > 0
    print(f'\n[env] force {w[0]["force"]} torque {w[0]["torque"]} contacts {w[0]["n_contacts"]}')
    assert w[0]['force'][0] < 0                                   # the water at rest resists the tool
    plain2 = _tool_env()                                          # a second run without the option: what two runs lie apart anyway
    noise = [np.abs(plain2.step(action)[0] - o_plain).max() for o_plain, _, _, _ in plain]
    env2 = _tool_env()
    env2.enable_contact_info()
    for (o_plain, _, _, _), nz in zip(plain, noise):
        o, _, _, info = env2.step(action)
        # the observation vector is unchanged: the same entries, as far from the run without the option as 4 x what two runs without it lie
        # apart (two rollouts agree to rounding, not to the bit: test_rollout_with_calls_against_rollouts_without), plus the ulps of the
        # velocities' range that test allows
        assert o.shape == o_plain.shape and o.dtype == o_plain.dtype
        d = np.abs(o - o_plain).max()
        print(f'[env] observation with the option against without {d:.3e}; without against without {nz:.3e}')
        assert d <= 4.0 * nz + NOISE_ULPS['v'] * max(1.0, np.abs(o_plain).max()), (d, nz)
        c = info['contact']
        assert len(c) == 1 and set(c[0]) == {'kind', 'index', 'force', 'torque', 'coverage', 'n_contacts'}
        again = env2.taichi_env.contact_wrench()                  # info['contact'] is TaichiEnv.contact_wrench() of the step just taken
        assert all(np.array_equal(c[0][k], again[0][k]) for k in ('force', 'torque')) and c[0]['n_contacts'] == again[0]['n_contacts']
    assert c[0]['coverage'] == 1.0 and c[0]['force'][0] < 0
