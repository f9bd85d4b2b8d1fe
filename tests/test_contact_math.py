"""Host build of the contact wrench's shared math -- one collider's step at a particle and at a node, the chains, the fixed-order merge and
the final record of fluidlab_amd/csrc/fe_contact.h, the functions k_contact_particles, k_contact_nodes and k_contact_merge run on the device --
against tests/contact_ref.py, the fp64 numpy restatement on oracle/mpm_numpy.py.  tests/csrc/contact_test.cpp reads a case this file writes and
returns its partial and merged records.  Built once plain and once with AddressSanitizer and UBSan on the host code, stand-alone.  No GPU.

Tolerance.  The engine's contact law is fp32, the restatement fp64.  The largest fp32 error is the normal: central differences of the trilinear
sample over 2e-2 voxels.  A sample is a sum of eight products of magnitude <= 0.3 (the lattices hold world distances), so it carries a few
2^-24 * 0.3 ~ 2e-8 of rounding, and the difference of two of them is divided by 2e-2 * (lattice value per voxel ~ 0.02 .. 0.04) ~ 6e-4: up to
~1e-4 per component of the normal, and the velocity change of a contact is linear in the normal.  TOL = 1e-3 of sum |m dv| (|r| times that
for the angular part) leaves one order of magnitude over that estimate; the contacts counted must agree exactly, which the cases make sure of
by asserting that no point lies within 1e-5 of a surface or of the soft branch's threshold.  The bound is the worst case of every contact of a
record erring the same way; the records of these cases (12 to 423 contacts) come out at 2e-7 to 3.5e-6, which is recorded here and not asserted."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_ref as R  # noqa: E402
import scenarios as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'contact_test.cpp')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')
SLOTS, MAX_EFF = 8, 4
TOL = 1e-3
ACC = np.dtype([('J', np.float64, 3), ('L', np.float64, 3), ('np', np.int64), ('nn', np.int64)])
REC = np.dtype([('impulse', np.float64, 3), ('ang_impulse', np.float64, 3), ('ref', np.float64, 3), ('n_particles', np.int64),
                ('n_nodes', np.int64), ('valid', np.int32), ('kind', np.int32)])


def _hipcc():
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if hipcc is None:
        pytest.skip('hipcc not available')
    os.makedirs(OUT, exist_ok=True)
    return hipcc


@pytest.fixture(scope='module')
def exe():
    hipcc = _hipcc()
    path = os.path.join(OUT, 'contact_test')
    subprocess.check_call([hipcc, '--offload-host-only', '-O2', '-std=c++17', '-x', 'hip', SRC, '-o', path])
    return path


def _sdf_words(c):
    T = np.asarray(c['T'], np.float64)
    return [np.int32(c['voxels'].shape[0])], [S.f32(T[:3].ravel()), S.f32(np.linalg.inv(T[:3, :3]).ravel()), S.f32([c['friction'], c.get('softness', 0.0)])]


def write_case(path, case):
    n_eff = len(case['dynamics'])
    with open(path, 'wb') as f:
        np.array([len(case['statics']), n_eff, case['node_dyn'], len(case['ijk']), len(case['px']), case['n_split']], np.int32).tofile(f)
        S.f32([case['dt'], 1.0 / case['n_grid'], *case['gravity'], case['collide_min_y']]).tofile(f)
        for st in case['statics']:
            i, fl = _sdf_words(st)
            for a in i + fl + [S.f32(st['voxels']).ravel()]:
                np.asarray(a).tofile(f)
        for d in case['dynamics']:
            mesh = d if d is not None else case['no_mesh']
            i, fl = _sdf_words(mesh)
            for a in [np.int32(d is not None)] + i + fl + [S.f32(mesh[k]) for k in ('pos0', 'quat0', 'pos1', 'quat1')] + [S.f32(mesh['voxels']).ravel()]:
                np.asarray(a).tofile(f)
        np.asarray(case['ijk'], np.int32).tofile(f)
        S.f32(np.concatenate([case['g_p'][tuple(case['ijk'].T)], case['g_m'][tuple(case['ijk'].T)][:, None]], 1)).tofile(f)
        S.f32(np.concatenate([case['px'], case['pm'][:, None], case['pnv']], 1)).tofile(f)


def read_result(path, n_split):
    raw = open(path, 'rb').read()
    o = 0
    out = {}
    for name, dt, n in (('node_partial', ACC, n_split * SLOTS), ('node_merged', ACC, SLOTS), ('part_partial', ACC, n_split * SLOTS),
                        ('part_merged', ACC, SLOTS), ('rec', REC, SLOTS), ('rec0', REC, SLOTS)):
        out[name] = np.frombuffer(raw, dt, n, o)
        o += n * dt.itemsize
    assert o == len(raw)
    return out


def make_case(kind, seed=8):           # (a seed at which no point lies within 1e-5 of a surface or of the soft threshold: check())
    """statics: two spheres in sequence, nodes only.  friction / soft / sticky: effector 0 a posed sphere mesh in that branch, effector 1 without a
    mesh, effector 2 a second, sticky mesh behind it; particles and nodes; collide_min_y cuts through the particles."""
    rng = np.random.RandomState(seed)
    n = 16
    case = dict(n_grid=n, dt=2e-4, gravity=(3.0, -10.0, 1.0), statics=[], dynamics=[], node_dyn=0, collide_min_y=-1e30, n_split=150)
    # every node of the box 2..12 per axis; a quarter of them without mass (0, or below FE_EPS)
    ijk = np.stack(np.meshgrid(*[np.arange(2, 13)] * 3, indexing='ij'), -1).reshape(-1, 3)
    g_m = np.zeros((n, n, n)); g_p = np.zeros((n, n, n, 3))
    m = S.f32(rng.uniform(1e-4, 4e-4, len(ijk)))
    m[rng.uniform(size=len(ijk)) < 0.15] = 0.0
    m[rng.uniform(size=len(ijk)) < 0.10] = np.float32(1e-13)
    g_m[tuple(ijk.T)] = m
    g_p[tuple(ijk.T)] = S.f32(m[:, None] * (rng.normal(0, 0.6, (len(ijk), 3)) + [0.5, -1.0, 0.2]))
    case.update(ijk=ijk, g_m=g_m, g_p=g_p)
    if kind == 'statics':
        v1, T1 = S.sphere_sdf((0.42, 0.30, 0.45), 0.12)
        v2, T2 = S.sphere_sdf((0.62, 0.40, 0.50), 0.10, res=20, lo=0.2, hi=0.9)
        v3, T3 = S.sphere_sdf((0.44, 0.35, 0.46), 0.13, res=20, lo=0.1, hi=0.9)      # overlaps the first: nodes that meet two statics in sequence
        case['statics'] = [dict(voxels=v1, T=T1, friction=0.5), dict(voxels=v2, T=T2, friction=0.0), dict(voxels=v3, T=T3, friction=2.0)]
        case.update(px=np.zeros((0, 3)), pm=np.zeros(0), pnv=np.zeros((0, 3)))
        return case
    vox, T = S.offset_sphere_sdf_mesh()
    pose = dict(pos0=S.f32([0.45, 0.47, 0.46]), quat0=S.f32([0.9238795, 0.0, 0.3826834, 0.0]), pos1=S.f32([0.452, 0.469, 0.461]),
                quat1=S.f32([0.9205049, 0.01, 0.3905, 0.005]))
    a = dict(voxels=vox, T=T, friction=dict(friction=0.5, soft=0.5, sticky=20.0)[kind], softness=60.0 if kind == 'soft' else 0.0, **pose)
    vox_b, T_b = S.offset_sphere_sdf_mesh(center=(-0.04, 0.03, 0.0), r=0.09)
    b = dict(voxels=vox_b, T=T_b, friction=20.0, softness=0.0, pos0=S.f32([0.5, 0.5, 0.5]), quat0=S.f32([1.0, 0.0, 0.0, 0.0]), pos1=S.f32([0.5, 0.501, 0.5]),
             quat1=S.f32([0.9999875, 0.0, 0.0, 0.005]))
    N = 1500
    case.update(dynamics=[a, None, b], no_mesh=a, node_dyn=1, collide_min_y=0.42,
                px=S.f32(rng.uniform(0.3, 0.62, (N, 3))), pm=S.f32(np.full(N, (0.5 / n) ** 2)), pnv=S.f32(rng.normal(0, 0.5, (N, 3))))
    return case


def reference(case):
    """contact_ref on the case's fp32 words, widened: the node chain on the listed nodes, the particle chain on the given gathered velocities"""
    recs_eff = [R.new_record() for _ in case['dynamics']]
    recs_st = [R.new_record() for _ in case['statics']]
    R.node_chain(case['g_p'], case['g_m'], case['n_grid'], case['dt'], S.f32(case['gravity']).astype(np.float64), None, case['statics'], case['dynamics'],
                 bool(case['node_dyn']), float(np.float32(case['collide_min_y'])), recs_eff, recs_st, eps=float(np.float32(1e-12)))
    if len(case['px']):
        R.dynamic_chain(case['dynamics'], float(np.float32(case['collide_min_y'])), case['dt'], case['pm'].astype(np.float64), case['px'].astype(np.float64),
                        case['pnv'].astype(np.float64), recs_eff, False)
    return recs_eff, recs_st


def run_case(exe, case, tmp_path):
    write_case(tmp_path / 'case.bin', case)
    r = subprocess.run([exe, str(tmp_path / 'case.bin'), str(tmp_path / 'res.bin')], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and '0 failures' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return read_result(tmp_path / 'res.bin', case['n_split'])


def merge_like_the_kernel(part):
    """[n, 8 words] -> the record k_contact_merge forms: lane l adds the partials l, l + 64, ... in order, then r[l] += r[l ^ o], o = 32 .. 1"""
    v = np.zeros((64,), ACC)
    for i in range(len(part)):
        for k in ACC.names:
            v[k][i % 64] = v[k][i % 64] + part[k][i]
    o = 32
    while o:
        w = v.copy()
        for k in ACC.names:
            w[k] = v[k] + v[k][np.arange(64) ^ o]
        v, o = w, o >> 1
    return v[0]


def check(res, case, recs_eff, recs_st):
    dt = case['dt']
    for c, ref in [(e, r) for e, r in enumerate(recs_eff)] + [(MAX_EFF + s, r) for s, r in enumerate(recs_st)]:
        got_J = res['node_merged']['J'][c] + res['part_merged']['J'][c]
        got_L = res['node_merged']['L'][c] + res['part_merged']['L'][c]
        assert res['node_merged']['nn'][c] == ref['n_nodes'] and res['part_merged']['np'][c] == ref['n_particles'], (c, ref['n_nodes'], ref['n_particles'])
        assert res['node_merged']['np'][c] == 0 and res['part_merged']['nn'][c] == 0
        assert np.abs(got_J - ref['impulse']).max() <= TOL * ref['abs_impulse'] + 1e-300, (c, got_J, ref['impulse'], ref['abs_impulse'])
        assert np.abs(got_L - ref['ang_impulse']).max() <= 2.0 * TOL * ref['abs_impulse'] + 1e-300, (c, got_L, ref['ang_impulse'])      # (r x dJ)_a <= |r_b| |dJ_c| + |r_c| |dJ_b|, |r_a| < 1
        assert ref['min_abs_sd'] > 1e-5, (c, ref['min_abs_sd'])                # no point within rounding of a surface or of the soft threshold: the counts are meaningful
    return dt


def test_two_statics_in_sequence_and_massless_nodes(exe, tmp_path):
    case = make_case('statics')
    res = run_case(exe, case, tmp_path)
    recs_eff, recs_st = reference(case)
    check(res, case, recs_eff, recs_st)
    assert all(r['n_nodes'] > 10 for r in recs_st), [r['n_nodes'] for r in recs_st]
    # nodes inside both overlapping spheres met the first and the third static in sequence
    inside = [R.static_sd(st, case['ijk'] / case['n_grid']) <= 0 for st in case['statics']]
    has_mass = case['g_m'][tuple(case['ijk'].T)] > np.float32(1e-12)
    assert (inside[0] & inside[2] & has_mass).sum() > 5
    # a node with m <= FE_EPS inside a static meets no collider: the counts above already exclude them, and some exist
    assert (inside[0] & ~has_mass).sum() > 0
    assert (res['part_merged']['np'] == 0).all() and (res['node_merged']['nn'][:MAX_EFF] == 0).all()


@pytest.mark.parametrize('kind', ['friction', 'soft', 'sticky'])
def test_effector_branches_chain_and_collide_min_y(exe, tmp_path, kind):
    case = make_case(kind)
    res = run_case(exe, case, tmp_path)
    recs_eff, recs_st = reference(case)
    check(res, case, recs_eff, recs_st)
    a, none, b = recs_eff
    assert a['n_particles'] > 20 and a['n_nodes'] > 5 and b['n_particles'] > 5, (a['n_particles'], a['n_nodes'], b['n_particles'], b['n_nodes'])
    assert none['n_particles'] == 0 and none['n_nodes'] == 0 and not none['impulse'].any()
    # particles that end below collide_min_y lie inside the first mesh as well, and are not counted
    pos = case['px'].astype(np.float64) + case['dt'] * case['pnv'].astype(np.float64)
    hit, sd = R.dynamic_hit(case['dynamics'][0], pos)
    below = pos[:, 1] <= np.float32(case['collide_min_y'])
    assert (hit & below).sum() > 5 and a['n_particles'] == (hit & ~below).sum()
    if kind == 'soft':                                            # the soft branch reaches outside the surface
        assert (hit & (sd > 0)).sum() > 5
    # the records handed out: sums of both parts, the effector's position words, kind; valid = 0 zeroes everything but kind
    for c in range(SLOTS):
        assert np.array_equal(res['rec']['impulse'][c], res['node_merged']['J'][c] + res['part_merged']['J'][c])
        assert res['rec']['n_particles'][c] == res['part_merged']['np'][c] and res['rec']['n_nodes'][c] == res['node_merged']['nn'][c]
        assert res['rec']['valid'][c] == 1 and res['rec']['kind'][c] == (0 if c < MAX_EFF else 1) == res['rec0']['kind'][c]
        assert res['rec0']['valid'][c] == 0 and not res['rec0']['impulse'][c].any() and not res['rec0']['ang_impulse'][c].any() and not res['rec0']['ref'][c].any()
        assert res['rec0']['n_particles'][c] == 0 and res['rec0']['n_nodes'][c] == 0
    for e, d in enumerate(case['dynamics']):
        assert np.array_equal(res['rec']['ref'][e], (d or case['no_mesh'])['pos0'].astype(np.float64))
    assert not res['rec']['ref'][len(case['dynamics']):].any()


def test_merge_order_is_the_kernels(exe, tmp_path):
    case = make_case('friction')
    res = run_case(exe, case, tmp_path)
    n_split = case['n_split']
    assert n_split > 64                                           # (lanes that add more than one partial)
    for name in ('node', 'part'):
        part = res[name + '_partial'].reshape(n_split, SLOTS)
        for c in range(SLOTS):
            want = merge_like_the_kernel(part[:, c])
            got = res[name + '_merged'][c]
            assert got.tobytes() == want.tobytes(), (name, c, got, want)
        assert any(part['J'][:, c].any() for c in range(SLOTS))
    # ... and differs from the plain left-to-right sum only by fp64 rounding
    part = res['part_partial'].reshape(n_split, SLOTS)
    plain = part['J'][:, 0].sum(0)
    assert np.abs(plain - res['part_merged']['J'][0]).max() <= n_split * 2.0 ** -53 * np.abs(part['J'][:, 0]).sum()


def test_contact_math_host_sanitized(tmp_path):
    hipcc = _hipcc()
    path = os.path.join(OUT, 'contact_test_san')
    subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                           '-Xarch_host', '-fno-sanitize-recover=undefined', '-x', 'hip', SRC, '-o', path])
    for kind in ('statics', 'sticky'):
        case = make_case(kind)
        case['n_split'] = 7
        run_case(path, case, tmp_path)
