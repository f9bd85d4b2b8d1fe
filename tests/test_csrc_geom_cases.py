"""The geometry and contact half of fluidlab_amd/csrc/fe_math.h per function, the part that needs no GPU (tests/geom_cases.py holds the cases and
references): the fp64 build of the header against references that are not the header -- oracle/mpm_numpy.py for values, central differences for the 20
columns of t_dynamic_collide<Dual>, the 7 of t_move_quat<Dual>, the contact-law and static-collide pull-backs and the boundary_x Jacobian -- the three
closed forms collide_chain_grad_row relies on, and the host fp32 build against fp64 under a measured cap, class by class, so that the GPU test
(tests/test_csrc_geom_hip.py), which bounds the device relative to the host fp32 build, is not relative to something that is itself wrong."""
import numpy as np
import pytest

import geom_cases as G

pytestmark = pytest.mark.skipif(G.M.hipcc() is None, reason='hipcc not available')

FD_TOL = 1e-6               # of the Jacobian's largest entry: tests/csrc/math_test.cpp's bound for the constitutive adjoint

# Host fp32 against host fp64 on the moving collider: class maximum of |out - out64| / (|out64| + 1) and of |J - J64| / max|J64|.  MEASURED is what this
# deterministic CPU run gives (the x86-64 half of the device library: the engine's flags, no FMA contraction); the cap asserted is 3 x MEASURED.
MEASURED = {
    ('thin', 0): (1.47e-4, 6.50e-4), ('thin', 1): (1.63e-4, 1.72e-3), ('thin', 2): (2.42e-4, 9.45e-4), ('thin', 3): (1.58e-4, 4.88e-7),
    ('thick', 0): (2.32e-4, 7.90e-4), ('thick', 1): (1.78e-4, 2.06e-3), ('thick', 2): (4.37e-4, 5.31e-4), ('thick', 3): (2.53e-4, 4.72e-7),
    ('sphere', 0): (1.65e-4, 5.26e-4), ('sphere', 1): (1.34e-4, 3.30e-3), ('sphere', 2): (1.72e-4, 2.89e-4), ('sphere', 3): (1.83e-4, 4.98e-7),
    ('odd', 0): (2.08e-4, 4.78e-4), ('odd', 1): (1.47e-4, 2.39e-3), ('odd', 2): (2.70e-4, 3.27e-4), ('odd', 3): (2.11e-4, 5.32e-7),
    ('scaled', 0): (1.29e-4, 1.33e-3), ('scaled', 1): (1.47e-4, 2.25e-3), ('scaled', 2): (1.60e-4, 2.81e-4), ('scaled', 3): (1.96e-4, 4.73e-7),
}
# (out: the collider's velocity (pn + p1 - pos) / dt loses 6e-8 x 0.5 / dt = 1.5e-4 in fp32 whatever the contact branch, sticky included;
#  J at softness 60: d infl / d sd = 60 infl multiplies the error of the sampled field.)


def _col(key):
    return G.colliders()[key[0]]


def test_libraries_cross_compile():
    import os
    lib = G.build_device_lib()
    with open(lib, 'rb') as f:
        blob = f.read()
    for k in (b'k_geom', b'gfx950'):
        assert k in blob, k
    d, f = G.device_lib(), G.f64_lib()
    assert d.real is np.float32 and f.real is np.float64 and d.has_device and not f.has_device
    assert d.widths == f.widths
    x = G.collide_class('thin', 0)
    assert f.run('classify', [x['x'][:4], x['fs'][:4]], collider=_col(('thin', 0)))[0] == 0
    assert d.run('classify', [x['x'][:4], x['fs'][:4]], collider=_col(('thin', 0)))[0] == -1          # the fp64 build only
    assert os.path.getsize(lib) > 0


def test_generators_fill_their_classes():
    """rejection below one half everywhere, every class at its size, every branch with at least 1,000 cases over the classes"""
    tot, soft_out = np.zeros(len(G.BRANCHES), int), 0
    for key in G.CLASS_KEYS:
        cs = G.collide_class(*key)
        assert len(cs['x']) == 2000 and cs['rejected'] < 0.5 * cs['drawn'], (key, cs['rejected'], cs['drawn'])
        assert np.array_equal(cs['x'], G.w32(cs['x']))                                  # float32 words
        qn = np.linalg.norm(cs['x'][:, G.Q0], axis=1)
        assert qn.min() < 0.9995 and qn.max() > 1.0005                                  # unnormalised q0
        assert np.abs(cs['x'][:, G.P1] - cs['x'][:, G.P0]).max() > 1e-4 and np.abs(cs['x'][:, G.Q1] - cs['x'][:, G.Q0]).max() > 1e-4
        c, hit = G.classify(_col(key), cs['x'], cs['fs'])
        sure, flat, branch = G.verdict(_col(key), c, hit, cs['fs'])
        assert sure.all() and not flat.any() and np.array_equal(branch, cs['branch'])
        res = _col(key)['res']
        assert ((c[:, G.C_PV] < 0) | (c[:, G.C_PV] > res - 1)).any()                    # positions outside the voxel box
        tot += np.bincount(cs['branch'], minlength=len(G.BRANCHES)); soft_out += int(cs['soft_outside'].sum())
    print('MEASURED branch counts', dict(zip(G.BRANCHES, tot.tolist())), 'soft-outside', soft_out)
    assert (tot >= 1000).all() and soft_out >= 1000
    flat = sum(len(G.collide_class(c, v)['flat']['x']) for c in ('thin', 'scaled') for v in (0, 1, 2))
    assert flat >= 100, flat


@pytest.mark.parametrize('key', G.CLASS_KEYS, ids=lambda k: f'{k[0]}-{k[1]}')
def test_collide_fp64_against_numpy_and_differences(key):
    """value and hit flag against oracle/mpm_numpy.py (given the exact inverse of T, as numpy takes it); all 20 Dual columns against central differences
    of the fp64 value; and the closed forms of the engine's adjoint: J_p1 = (I - J_mv) / dt, J_pos = -J_p0 - (I - J_mv) / dt, J_q1 = J_p1 d rot(pm, q1) / d q1,
    at the absolute scale 1 / dt (|I - J_mv| is 0 on the separating branch)."""
    col, cs, f = _col(key), G.collide_class(*key), G.f64_lib()
    x, fs = cs['x'], cs['fs']
    ref = G.numpy_collide(col, x, fs, cs['group'])
    oe = G.run_collide(f, col, x, fs, rinv=col['Rinv_exact'])
    moved = np.abs(ref - x[:, G.MV]).max(axis=1) > 0
    assert np.array_equal(oe['hit'].astype(bool), cs['hit']) and (moved <= cs['hit']).all()
    e_np = np.abs(oe['out'] - ref).max()
    o = G.run_collide(f, col, x, fs)
    Jfd = G.fd_jacobian(lambda y: G.run_collide(f, col, y, fs)['out'], x, G.FD_STEP)
    big = np.abs(o['J']).max(axis=(1, 2))
    e_fd = (np.abs(Jfd - o['J']).max(axis=(1, 2)) / big).max()
    I, Jmv = np.eye(3), o['J'][:, :, G.MV]
    Jcv = (I - Jmv) / G.DT
    pm = G.qrot(x[:, G.POS] - x[:, G.P0], G.qconj_n(x[:, G.Q0]))
    e_id = max(np.abs(o['J'][:, :, G.P1] - Jcv).max(), np.abs(o['J'][:, :, G.POS] + o['J'][:, :, G.P0] + Jcv).max(),
               np.abs(o['J'][:, :, G.Q1] - Jcv @ G.qrot_dq(pm, x[:, G.Q1])).max()) * G.DT
    print(f'MEASURED {key}: fp64 vs numpy {e_np:.3g}, Dual vs differences {e_fd:.3g} of the largest entry, closed forms {e_id:.3g} / dt')
    assert e_np <= 1e-10                        # two fp64 evaluations of velocities of O(1) formed through 1 / dt = 5000
    assert (big[~cs['hit']] == 1.0).all()       # a miss passes mv through
    assert e_fd <= FD_TOL
    assert e_id <= 1e-12                        # the same fp64 products in another order, relative to 1 / dt


@pytest.mark.parametrize('key', G.CLASS_KEYS, ids=lambda k: f'{k[0]}-{k[1]}')
def test_collide_host_fp32_against_fp64(key):
    col, cs = _col(key), G.collide_class(*key)
    o32, o64 = G.run_collide(G.device_lib(), col, cs['x'], cs['fs']), G.run_collide(G.f64_lib(), col, cs['x'], cs['fs'])
    e = G.collide_errors(o32, o64)
    print(f'MEASURED {key}: host fp32 vs fp64 out {e["out"]:.3g} J {e["J"]:.3g}')
    assert np.array_equal(o32['hit'], o64['hit'])
    assert e['out'] <= 3 * MEASURED[key][0] and e['J'] <= 3 * MEASURED[key][1]


def test_collide_ties_on_the_host():
    """sd exactly 0, infl exactly at its cap, and either side of both and of the soft edge: the hit select of both host builds is the expected one, and the
    values agree (the field is a plane: the normal is well conditioned on the tie itself)"""
    col = G.tie_collider()
    x, fs, hit = G.collide_ties()
    c, chit = G.classify(col, x, fs)
    assert np.array_equal(c[:8, G.C_SD], x[:8, G.POS][:, 1])                                # sd = pos_y without rounding
    assert c[3, G.C_INFL] == 1.0 and c[4, G.C_INFL] == 1.0 and c[5, G.C_INFL] < 1.0         # at the cap, capped, just below it
    assert np.array_equal(chit, hit)
    o64, o32 = G.run_collide(G.f64_lib(), col, x, fs), G.run_collide(G.device_lib(), col, x, fs)
    assert np.array_equal(o64['hit'].astype(bool), hit) and np.array_equal(o32['hit'].astype(bool), hit)
    assert np.array_equal(o64['out'][~hit], x[~hit][:, G.MV])
    sticky = hit & (fs[:, 0] > 10)
    assert (o64['out'][sticky] == 0).all()                                                  # cv = 0 exactly
    e = np.abs(o32['out'] - o64['out']).max()
    print(f'MEASURED collide ties host fp32 vs fp64 out {e:.3g}')
    assert e <= 3e-6                                                                        # MEASURED 6.9e-8: one float32 step of a velocity below 1


def flat_cell_properties(o, x, fs, cls_cols, branch, label, own_branch):
    """What holds in the flat cell layer whatever the normal is (shared with the GPU test).  With n a vector of length at most 1 and rel = mv - cv:
    separating (nc >= 0): a = 0, vt = rel, out = cv + rel (infl + 1 - infl) = mv.  Otherwise vt = rel - nc n is rel with a part of its n-component removed
    (|n| <= 1: |vt| <= |rel|), scaled by a factor in [0, 1]; out - cv = infl vt' + (1 - infl) rel is a convex combination of two vectors no longer than rel."""
    out = o['out'].astype(np.float64)
    assert np.isfinite(out).all() and np.isfinite(o['J']).all(), label
    cv, mv = cls_cols[:, G.C_CV], x[:, G.MV]
    rel = np.linalg.norm(mv - cv, axis=1)
    # `branch` is the fp64 build's (its difference is exactly 0, so n = 0, nc = 0: separating); another build's noise normal picks its own branch
    sep = (branch == 2) if own_branch else np.zeros(len(x), bool)
    scale = np.abs(mv).max(axis=1) + np.abs(cv).max(axis=1)          # out is formed as cv + (mv - cv): the rounding is relative to the larger of the two
    assert (np.abs(out - mv).max(axis=1)[sep] <= 1e-5 * scale[sep]).all(), label
    # cv and rel here are the fp64 build's.  An fp32 build forms its own cv = (pn + p1 - pos) / dt from three numbers below 1 in all: it is off by up to
    # 3 x 6e-8 / dt = 9e-4 in out and in rel alike; the bound is the issue's |out - cv| <= |rel| (1 + 1e-5) with that much room for the other build's cv.
    slack = 0.0 if own_branch else 2 * 3 * 6e-8 / G.DT
    excess = np.linalg.norm(out - cv, axis=1) - rel * (1 + 1e-5) - 1e-5 * scale
    print(f'MEASURED flat cell {label}: n = {len(x)}, largest |out - cv| - |rel| (1 + 1e-5) = {excess.max():.3g} (room {slack:.3g})')
    assert (excess <= slack).all(), label


@pytest.mark.parametrize('cname', ['thin', 'scaled'])
def test_flat_cell_layer_on_the_host(cname):
    """The hits whose central difference is below 1e-3 of the nominal gradient: an even res puts a layer of cells across the box's mid-plane whose corner
    values are equal on both sides; the trilinear field is flat there, the fp64 difference is exactly 0 and the fp32 one is rounding noise normalised into an
    arbitrary direction.  fp32 and fp64 then differ by O(|rel|) with nothing wrong, so nothing is asserted about their agreement -- only what holds for ANY
    normal of length at most 1 (flat_cell_properties), on both builds."""
    col = G.colliders()[cname]
    for vi in (0, 1, 2):
        fl = G.collide_class(cname, vi)['flat']
        c, hit = G.classify(col, fl['x'], fl['fs'])
        assert hit.all() and len(fl['x']) >= 20
        for lib, label in ((G.f64_lib(), 'fp64'), (G.device_lib(), 'host fp32')):
            rc, (_, _, nrm), _ = lib.run('sdf', [c[:, G.C_PV]], collider=col)                  # sdf_normal in the layer: any direction, never longer than 1
            assert rc == 0 and np.isfinite(nrm).all() and (np.linalg.norm(nrm.astype(np.float64), axis=1) <= 1 + 1e-6).all(), (cname, vi, label)
            flat_cell_properties(G.run_collide(lib, col, fl['x'], fl['fs']), fl['x'], fl['fs'], c, fl['branch'], (cname, vi, label), label == 'fp64')


def test_sdf_against_numpy_and_edges():
    f, d = G.f64_lib(), G.device_lib()
    for cname in ('thin', 'odd', 'sphere', 'scaled'):
        col = G.colliders()[cname]
        vox = col['vox'].reshape((col['res'],) * 3)
        for pv, exact in ((G.sdf_points(cname), False), (G.sdf_edge_points(col), True)):
            rc, (sd, sdt, nrm), _ = f.run('sdf', [pv], collider=col, rinv=col['Rinv_exact'])
            assert rc == 0
            ref = G.NP._sdf_sample(vox, pv)
            assert np.abs(sd[:, 0] - ref).max() <= 1e-14 and (np.array_equal(sd, sdt) or np.abs(sd - sdt).max() <= 1e-15)
            if exact:
                assert np.array_equal(sd[:, 0] == 1.0, ref == 1.0)
            assert (np.linalg.norm(nrm, axis=1) <= 1 + 1e-12).all()
            rc, (s32, st32, n32), _ = d.run('sdf', [pv], collider=col)
            assert rc == 0 and np.abs(s32[:, 0] - ref).max() <= 2.5e-7 and np.abs(st32[:, 0] - ref).max() <= 2.5e-7          # 3 x MEASURED 8.2e-8 (thin, scaled; sphere 5.6e-8)
            if exact:                                                                   # outside / inside decided alike on every hand-written edge
                assert np.array_equal(s32[:, 0] == 1.0, ref == 1.0), cname
        # the normal against numpy's: static_collide with friction 0 on a unit inward velocity is not needed -- restate the five lines
        pv = G.sdf_points(cname)
        g = np.stack([(G.NP._sdf_sample(vox, pv + e) - G.NP._sdf_sample(vox, pv - e)) / 2e-2 for e in 1e-2 * np.eye(3)], axis=1)
        g /= np.sqrt((g ** 2).sum(1) + G.EPS)[:, None]
        n = g @ col['Rinv_exact'].T
        n /= np.sqrt((n ** 2).sum(1) + G.EPS)[:, None]
        rc, (_, _, nrm), _ = f.run('sdf', [pv], collider=col, rinv=col['Rinv_exact'])
        assert np.abs(nrm - n).max() <= 1e-9, cname                                     # (1e-16 / 2e-2 / the gradient's 2e-2, normalised)


def test_contact_law_and_static_collide():
    """values against numpy's static_collide / its contact law, pull-backs against central differences of the fp64 value (normal held fixed)"""
    f = G.f64_lib()
    n, rv, g, fr = G.contact_law_cases()
    rc, (out, gb), _ = f.run('contact_law', [n, rv, g, fr])
    assert rc == 0
    assert np.abs(out - G.numpy_contact_law(n, rv, fr[:, 0])).max() <= 1e-14
    J = G.fd_jacobian(lambda y: f.run('contact_law', [n, y, g, fr])[1][0], rv, np.full(3, 1e-6))
    e = np.abs(np.einsum('ni,nij->nj', g, J) - gb).max(axis=1) / np.maximum(np.abs(J).max(axis=(1, 2)) * np.abs(g).max(axis=1), 1e-300)
    print(f'MEASURED contact_law pull-back vs differences {e.max():.3g}')
    assert e.max() <= FD_TOL
    nc = (rv * n).sum(1)
    assert min((nc >= 0).sum(), ((nc < 0) & (np.linalg.norm(out, axis=1) == 0)).sum(), ((nc < 0) & (np.linalg.norm(out, axis=1) > 0)).sum()) >= 300
    rc, (o32, g32), _ = G.device_lib().run('contact_law', [n, rv, g, fr])
    assert np.abs(o32 - out).max() <= 7e-7 and np.abs(g32 - gb).max() <= 3.3e-7 * np.abs(gb).max()          # 3 x MEASURED 2.24e-7, 1.07e-7
    # static_collide on the sphere and the scaled plate, friction 0.5: cases of the moving collider's class with the pose taken out
    for cname in ('sphere', 'scaled'):
        col, cs = G.colliders()[cname], G.collide_class(cname, 0)
        c, hit = G.classify(col, cs['x'], cs['fs'])
        pos = G.w32(G.qrot(cs['x'][:, G.POS] - cs['x'][:, G.P0], G.qconj_n(cs['x'][:, G.Q0])))          # the mesh-frame point as a world position
        x = np.concatenate([np.zeros((len(pos), 3)), np.tile([1.0, 0, 0, 0], (len(pos), 1)), np.zeros((len(pos), 3)), np.tile([1.0, 0, 0, 0], (len(pos), 1)), pos,
                            cs['x'][:, G.MV]], axis=1)
        fs = cs['fs']
        c, hit = G.classify(col, x, fs, dt=1e30)                                        # cv = 0: the static collider's margins
        sure, _, _ = G.verdict(col, c, hit, fs)
        pos, v, gg, ff = pos[sure], x[sure][:, G.MV], g[:sure.sum()], fs[sure][:, :1]
        assert sure.sum() >= 1500 and hit[sure].sum() >= 100
        rc, (vo, gb), _ = f.run('static_collide', [pos, v, gg, ff], collider=col, rinv=col['Rinv_exact'])
        st = dict(voxels=col['vox'].reshape((col['res'],) * 3), T=np.vstack([col['T'][:3], [0, 0, 0, 1.0]]), friction=float(ff[0, 0]))
        assert np.abs(vo - G.NP.static_collide(st, pos, v)).max() <= 1e-12, cname
        J = G.fd_jacobian(lambda y: f.run('static_collide', [pos, y, gg, ff], collider=col, rinv=col['Rinv_exact'])[1][0], v, np.full(3, 1e-6))
        e = np.abs(np.einsum('ni,nij->nj', gg, J) - gb).max(axis=1) / np.maximum(np.abs(J).max(axis=(1, 2)) * np.abs(gg).max(axis=1), 1e-300)
        assert e.max() <= FD_TOL, (cname, e.max())


def test_move_quat_and_quaternions():
    f, d = G.f64_lib(), G.device_lib()
    wq, hand = G.move_quat_cases()
    for cases in (wq, hand):
        rc, (q, J), _ = f.run('move_quat', [cases])
        assert rc == 0 and np.isfinite(q).all() and np.isfinite(J).all()
        assert np.abs(q - G.numpy_move_quat(cases)).max() <= 1e-14
        assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-14
        rc, (q32, J32), _ = d.run('move_quat', [cases])
        assert np.isfinite(q32).all() and np.isfinite(J32).all() and np.abs(q32 - q).max() <= 4.5e-7
        assert np.abs(J32 - J).max() <= 9e-7 * np.abs(J).max()                # host fp32 vs fp64, 3 x MEASURED: q 1.5e-7, J 2.85e-7 of its largest entry
    rc, (q, J), _ = f.run('move_quat', [wq])
    Jfd = G.fd_jacobian(lambda y: f.run('move_quat', [y])[1][0], wq, np.full(7, 1e-6))
    e = np.abs(Jfd - J.reshape(-1, 4, 7)).max(axis=(1, 2)) / np.abs(J).max(axis=1)
    print(f'MEASURED t_move_quat<Dual> vs differences {e.max():.3g}')
    assert e.max() <= FD_TOL
    # quat_mul, quat_from_w, quat_rotate against numpy
    rng = np.random.RandomState(3)
    n = 2000
    qa, qb, aa, v = G.w32(G.unit_quats(rng, n)), G.w32(G.unit_quats(rng, n)), G.w32(rng.normal(size=(n, 3))), G.w32(rng.normal(size=(n, 3)))
    aa[:3] = [[0, 0, 0], [1e-7, 0, 0], [0, 0, -1e-7]]
    rc, (mul, fw, rot), _ = f.run('quat', [qa, qb, aa, v])
    m = G.qmul_ref(qa, qb)
    wn = np.sqrt((aa ** 2).sum(1, keepdims=True) + G.EPS)
    assert np.abs(mul - m / np.linalg.norm(m, axis=1, keepdims=True)).max() <= 1e-14
    assert np.abs(fw - np.concatenate([np.cos(wn / 2), aa / wn * np.sin(wn / 2)], axis=1)).max() <= 1e-14 and np.isfinite(fw).all()
    assert np.abs(rot - G.qrot(v, qa)).max() <= 1e-14
    rc, (m32, f32_, r32), _ = d.run('quat', [qa, qb, aa, v])
    # 3 x MEASURED 1.47e-7 (quat_mul), 1.16e-7 (quat_from_w), 5.4e-7 (quat_rotate of vectors up to 4 long)
    assert np.abs(m32 - mul).max() <= 4.5e-7 and np.abs(f32_ - fw).max() <= 3.5e-7 and np.abs(r32 - rot).max() <= 1.7e-6 and np.isfinite(f32_).all()


def boundary_ties(b):
    """hand-written: x on a face with v = 0, > 0, < 0 (the cube's >= / <= against the cylinder's > / <), on both faces, and a cylinder point on its axis"""
    lo, up = (np.array(b['lower']), np.array(b['upper'])) if b['type'] == 'cube' else (np.array([0.0, b['y_range'][0], 0.0]), np.array([1.0, b['y_range'][1], 1.0]))
    X, V = [], []
    for face in (lo, up):
        for d in range(3):
            for vv in (0.0, 0.7, -0.7):
                x = np.array([0.5, 0.5 * (lo[1] + up[1]), 0.45]); x[d] = face[d]
                v = np.array([0.3, -0.2, 0.1]); v[d] = vv
                X.append(x); V.append(v)
    if b['type'] != 'cube':
        c, r = b['xz_center'], b['xz_radius']
        for rr in (float(np.nextafter(G.f32(r), G.f32(0))), r, float(np.nextafter(G.f32(r), G.f32(9)))):          # nrm within one ulp of the radius
            X.append([c[0] + rr, 0.5, c[1]]); V.append([0.3, 0.2, 0.1])
        X.append([c[0], 0.5, c[1]]); V.append([0.3, 0.2, 0.1])                                                   # on the axis: nrm = sqrt(FE_EPS)
    return G.w32(X), G.w32(V)


def radial_ties(b, n):
    """rows of boundary_ties whose verdict hangs on nrm against the radius: FE_EPS under the root is below half an ulp of rx^2 in fp32 and not in fp64, so
    within an ulp of the wall the two precisions decide differently and both are right; the fp32 builds are held equal to each other there (GPU test)"""
    m = np.zeros(n, bool)
    if b['type'] != 'cube':
        m[-4:-1] = True
    return m


@pytest.mark.parametrize('bname', sorted(G.BOUNDARIES))
def test_boundaries_against_numpy(bname):
    f, d = G.f64_lib(), G.device_lib()
    b, x, v = G.boundary_cases(bname)
    tx, tv = boundary_ties(b)
    for xx, vv, tie in ((x, v, False), (tx, tv, True)):
        rc, (vo, k, xn, J), (is_out,) = f.run('boundary', [xx, vv], bnd=b)
        assert rc == 0
        rv, rxn, rout = G.numpy_boundary(b, xx, vv)
        assert np.array_equal(vo, rv) or np.abs(vo - rv).max() <= 1e-16
        assert np.abs(xn - rxn).max() <= 1e-15 and np.array_equal(is_out[:, 0].astype(bool), rout)
        rc, (vo32, k32, xn32, J32), (out32,) = d.run('boundary', [xx, vv], bnd=b)
        if tie:
            keep = ~radial_ties(b, len(xx))
            vo, k, xn, J, is_out, vo32, k32, xn32, J32, out32 = (a[keep] for a in (vo, k, xn, J, is_out, vo32, k32, xn32, J32, out32))
        assert np.array_equal(k32, k) and np.array_equal(out32, is_out) and np.abs(xn32 - xn).max() <= 1.9e-7 and np.abs(vo32 - vo).max() <= 6e-8
        unit = (J == 0) | (J == 1)
        # host fp32 vs fp64, 3 x MEASURED: xn 6.3e-8 (cylinder; cube 0), v' 0 (one float32 step allowed), J 1.9e-7
        assert np.array_equal(J32[unit], J[unit]) and np.abs(J32 - J).max() <= 6e-7
        if not tie:
            Jfd = G.fd_jacobian(lambda y: f.run('boundary', [y, vv], bnd=b)[1][2], xx, np.full(3, 1e-7)).reshape(-1, 9)
            assert np.abs(Jfd - J).max() <= FD_TOL, bname
    if b['type'] == 'cube' and b['lower'][1] == b['upper'][1]:
        assert (J.reshape(-1, 3, 3)[:, 1, 1] == 0).all() and (xn[:, 1] == b['lower'][1]).all()                   # lower == upper: pinned, no gradient
    if b.get('lock_dims'):
        assert (vo[:, list(b['lock_dims'])] == 0).all()


def test_stencil_against_numpy():
    f, d = G.f64_lib(), G.device_lib()
    for x, tie in ((G.stencil_cases(), False), (G.stencil_ties(), True)):
        base, fx, w, dw, inside = G.stencil_reference(x, 16)
        assert tie or np.array_equal(base, G.stencil_reference(x, 16, np.float32)[0])          # away from the ties both precisions truncate alike
        if not tie:
            b0, _, w0 = G.NP.weights(x, 16.0)                                            # mpm_numpy's own, where it is defined alike (any sign: astype truncates)
            assert np.array_equal(b0, base) and np.abs(np.moveaxis(w0, 0, 1) - w).max() <= 1e-15
        for lib, tol in ((f, 1e-14), (d, 9e-7)):          # host fp32 vs fp64: 3 x MEASURED 2.95e-7 (w; fx 0, dw 1.2e-7)
            base, fx, w, dw, inside = G.stencil_reference(x, 16, lib.real)
            rc, (gfx, gw, gdw), (gb, gin) = lib.run('stencil', [x], inv_dx=16.0, n_grid=16)
            assert rc == 0 and np.array_equal(gb, base) and np.array_equal(gin[:, 0].astype(bool), inside)
            assert np.abs(gfx - fx).max() <= tol and np.abs(gw.reshape(-1, 3, 3) - w).max() <= tol and np.abs(gdw.reshape(-1, 3, 3) - dw).max() <= tol
    for wild in G.STENCIL_WILD:                                                          # the host's cast of these is its own business; inside must be false
        x = np.full((3, 3), 0.53125); x[np.arange(3), np.arange(3)] = wild
        rc, _, (gb, gin) = d.run('stencil', [x], inv_dx=16.0, n_grid=16)
        assert rc == 0 and not gin.any(), wild
