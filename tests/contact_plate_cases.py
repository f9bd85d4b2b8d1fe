"""The engine's collide adjoint on a box, one substep, particle by particle (tests/test_contact_plate_hip.py on the GPU, tests/test_contact_plate_cases.py
on the CPU).  Scene: stirrer_mini's water block with the thin plate tilted 45 degrees and a 6-dof action that moves and turns it; ONE substep forward and
backward, so no trajectory amplifies anything.  Every used particle's gathered velocity and position come from the fp64 restatement (tests/contact_ref.py:
p2g_liquid, node_chain, gather) and go through the `classify` entry of tests/csrc/geom_device_test.hip; a particle is *sure* when it respects the margins
of tests/geom_cases.py (verdict) and *unsure* (flat cell / near an edge) otherwise.  The cotangent on frame 1 is zero on the unsure particles: the
particle-level collide acts after the gather, so that removes their contact Jacobian from the whole adjoint, and what remains can be compared per particle."""
import numpy as np

import contact_ref as R
import geom_cases as G
import scenarios as S
from test_contact_hip import dyn_of, first_substep, lam64, mass64, rigid_engine

VARIANTS = ((0.5, 0.0), (0.1, 60.0), (2.0, 0.0))          # (friction, softness) at collide_type = 1
MIN_SURE, MIN_BRANCH, MAX_UNSURE = 100, 20, 0.15          # conditions on the scene, not measurements


def plate_scene(vi):
    friction, softness = VARIANTS[vi]
    # seed 14: of the seeds 11 ... 22 one of those whose fp64 classification meets check_conditions in all three variants with the smallest unsure share
    return S.stirrer_mini(horizon=1, n_substeps=4, friction=friction, softness=softness, shape='box', seed=14)


def classify_scene(sc, eng, e):
    """after the first substep of `eng` (the fp64 oracle): -> dict contact, sure, branch per particle (unused particles: no contact, sure)"""
    st0 = S.get_state(eng, 0)
    x, v, C, F = (st0[k].astype(np.float64) for k in 'xvCF')
    used = st0['used'].astype(bool)
    dyn = dyn_of(sc, eng, e, 0)
    n, dt = sc['n_grid'], sc['dt']
    g_p, g_m = R.p2g_liquid(x, v, C, F, st0['used'], mass64(sc), lam64(sc), n, dt, (0.5 / n) ** 2)
    v_out, _, _ = R.node_chain(g_p, g_m, n, dt, S.f32(sc['gravity']).astype(np.float64), sc['boundary'], (), (dyn,), False, -1e30, [R.new_record()], [])
    nv = R.gather(x[used], v_out, n)
    pos = x[used] + dt * nv
    col = G.colliders()['thin']
    assert np.array_equal(col['vox'].reshape(-1), np.asarray(sc['rigid']['voxels'], np.float64).reshape(-1))          # the plate of stirrer_mini
    k = len(pos)
    cases = np.concatenate([np.tile(np.concatenate([dyn['pos0'], dyn['quat0'], dyn['pos1'], dyn['quat1']]), (k, 1)), pos, nv], axis=1)
    fs = np.tile([dyn['friction'], dyn['softness']], (k, 1))
    c, hit = G.classify(col, cases, fs, dt=dt)
    sure_u, _, branch_u = G.verdict(col, c, hit, fs)
    N = len(x)
    contact, sure, branch = np.zeros(N, bool), np.ones(N, bool), np.zeros(N, int)
    contact[used], sure[used], branch[used] = hit, sure_u, branch_u
    return dict(contact=contact, sure=sure, branch=branch, v1_ref=M_collide(dyn, pos, nv, dt, used, N))


def M_collide(dyn, pos, nv, dt, used, N):
    out = np.zeros((N, 3))
    out[used] = R.M.dynamic_collide(dyn, pos, nv, dt)
    return out


def cotangent(sc, sure):
    cot = S.random_cotangent(sc['N'], seed=9)
    for k in cot:
        cot[k] = np.ascontiguousarray(np.where(sure.reshape((-1,) + (1,) * (cot[k].ndim - 1)), cot[k], 0).astype(np.float32))
    return cot


def forward_frame(lib, sc, options=None, mesh=True):
    """frame 1 of the scene as the engine holds it (its own words: for comparisons bit by bit), with engine options and with or without the plate's mesh"""
    if mesh:
        eng, e = rigid_engine(lib, sc, options=options)
    else:                                                 # rigid_engine without eff_set_mesh: the effector moves, nothing collides
        eng = S.make_engine(lib, sc, options=options)
        r = sc['rigid']
        e = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=r['action_dim'], action_scale_v=r['action_scale_v'], action_scale_p=r['action_scale_p'],
                             boundary=lib.make_boundary(**r['boundary']))
        st0 = eng.eff_get_state(e, 0)
        st0[:7] = r['init_state']
        eng.eff_set_state(e, 0, st0)
        eng.eff_apply_action_p(e, sc['action_p'])
    first_substep(eng, e, sc)
    f1 = S.get_state(eng, 1)
    eng.close()
    return f1


def run_plate(lib, sc, sure=None, classify=False, device=0):
    """one substep forward; with `sure` also backward from the masked cotangent.  -> dict v1, used, cls (if classify), gx, gv, action_grad"""
    eng, e = rigid_engine(lib, sc)
    first_substep(eng, e, sc)
    f1 = S.get_state(eng, 1)
    out = dict(v1=f1['v'].astype(np.float64), x1=f1['x'].astype(np.float64), used=f1['used'].astype(bool))
    if classify:
        out['cls'] = classify_scene(sc, eng, e)
        sure = out['cls']['sure'] if sure is None else sure
    if sure is not None:
        cot = cotangent(sc, sure)
        eng.reset_grad()
        eng.add_grad(1, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        eng.step_grad(0, 0, 1, 1)
        eng.eff_set_action_grad(e, 0, 0, sc['n_substeps'])
        eng.eff_apply_action_p_grad(e)
        g = eng.get_grad(0)
        out.update(gx=g[0].astype(np.float64), gv=g[1].astype(np.float64),
                   action_grad=np.asarray(eng.eff_get_action_grad(e, 0, sc['horizon'], sc['rigid']['action_dim']), np.float64))
    eng.close()
    return out


def check_conditions(cls, vi):
    """the conditions of the scene (asserted on the CPU from the fp64 reference alone) -> the counts, for printing"""
    sc_ = cls['contact'] & cls['sure']
    counts = {b: int((sc_ & (cls['branch'] == i)).sum()) for i, b in enumerate(G.BRANCHES) if i >= 2}
    unsure = float((cls['contact'] & ~cls['sure']).sum()) / max(int(cls['contact'].sum()), 1)
    assert sc_.sum() >= MIN_SURE, (vi, int(sc_.sum()))
    assert counts['slide'] >= MIN_BRANCH and counts['separating'] >= MIN_BRANCH, (vi, counts)
    if VARIANTS[vi][0] == 2.0:
        assert counts['stick'] >= MIN_BRANCH, (vi, counts)
    assert unsure <= MAX_UNSURE, (vi, unsure)
    return dict(sure_contacts=int(sc_.sum()), unsure_share=unsure, **counts)


def errors(a, ref, cls):
    """max norms against `ref`: forward v' over the sure contact particles, gx and gv over ALL particles, the action gradient"""
    m = cls['contact'] & cls['sure']
    return dict(v1=float(np.abs(a['v1'] - ref['v1'])[m].max()), gx=float(np.abs(a['gx'] - ref['gx']).max()), gv=float(np.abs(a['gv'] - ref['gv']).max()),
                action_grad=float(np.abs(a['action_grad'] - ref['action_grad']).max()))


def floors(ref, cls):
    """a few float32 steps of each field's range: 4 x 6e-8 x max |field|"""
    m = cls['contact'] & cls['sure']
    return dict(v1=2.4e-7 * np.abs(ref['v1'][m]).max(), gx=2.4e-7 * np.abs(ref['gx']).max(), gv=2.4e-7 * np.abs(ref['gv']).max(),
                action_grad=2.4e-7 * np.abs(ref['action_grad']).max())


def flat_cell_share(engine, effector, frames, dt):
    """Of the particles in contact with `effector`'s mesh in the substeps `frames` of a finished rollout: the share whose central difference of the SDF is
    below 1e-3 of the median one over the contacts (the flat cell layer).  Position and pose decide both; the position is x[f] + dt v[f + 1], which is the one
    the collide saw up to dt |v' - v_gathered|.  A printed figure for test_gathering_easy_on_the_gpu, not a classification anything is asserted on.
    -> (flat, contacts)"""
    mesh = effector.mesh
    vox = np.asarray(mesh.sdf_voxels_np, np.float64)
    T = np.asarray(mesh.T_mesh_to_voxels_np, np.float64)
    col = dict(vox=vox, res=vox.shape[0], T=T, Rinv=np.linalg.inv(T[:3, :3]))
    N = engine.N
    flat = contacts = 0
    for f in frames:
        x, v, used = np.zeros((N, 3), engine.dtype), np.zeros((N, 3), engine.dtype), np.zeros((N,), np.int32)
        engine.get_frame(f, x=x, used=used)
        engine.get_frame(f + 1, v=v)
        p0, p1 = (engine.eff_get_state(effector.index, g).astype(np.float64) for g in (f, f + 1))
        u = used.astype(bool)
        pos = x[u].astype(np.float64) + dt * v[u].astype(np.float64)
        cases = np.concatenate([np.tile(np.concatenate([p0[:7], p1[:7]]), (len(pos), 1)), pos, v[u].astype(np.float64)], axis=1)
        fs = np.tile([min(float(mesh.friction), 10.0), float(mesh.softness)], (len(pos), 1))
        c, hit = G.classify(col, cases, fs, dt=dt)
        if hit.any():
            g = c[hit, G.C_G]
            flat += int((g < G.FLAT * np.median(g)).sum()); contacts += int(hit.sum())
    return flat, contacts


# ------------------------------------------------------------------------------------------------------------------------------------
# collide_type = 3: the sphere and the plate as two meshed effectors of one agent, colliding at the grid nodes and at the particles
# ------------------------------------------------------------------------------------------------------------------------------------
# of 14 poses tried on the fp64 oracle (the first the plate scene's, the rest drawn within 0.03 of it) the first with NO unsure massy node: node positions are a
# lattice, so that is a property of the pose.  10 nodes and 86 sure particles hit both colliders there.
TWO_POSE = dict(sphere=[0.447, 0.448, 0.449, 1.0, 0.0, 0.0, 0.0], plate=[0.477, 0.471, 0.455, 0.9238795, 0.0, 0.3826834, 0.0])
MIN_BOTH = 20


def two_tool_scene(pose=None):
    """plate_scene(0) with a second effector in front of the plate in the agent's chain: the offset sphere (friction 0.3), overlapping the plate, each with its
    own 6-dof action.  Effector 0 is the sphere, effector 1 the plate: a particle inside both runs the chain twice, and the adjoint walks it backwards."""
    pose = pose or TWO_POSE
    sc = plate_scene(0)
    sc['collide_type'] = 3
    rng = np.random.RandomState(5)
    vox, T = S.offset_sphere_sdf_mesh()
    plate = dict(sc['rigid'], init_state=list(pose['plate']), col='thin')
    sphere = dict(sc['rigid'], voxels=vox, T=T, friction=0.3, softness=0.0, init_state=list(pose['sphere']), col='sphere')
    sc['tools'] = [dict(sphere, action_p=S.f32(list(pose['sphere'][:3]) + [0, 0, 0]),
                        action=S.f32(np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.3, 0.3, 3)]))),
                   dict(plate, action_p=S.f32(list(pose['plate'][:3]) + [0, 0, 0]), action=sc['actions'][0])]
    return sc


def two_tool_engine(lib, sc):
    eng = S.make_engine(lib, sc)
    effs = []
    for r in sc['tools']:
        e = eng.add_effector(type=S.FE_EFF_PLAIN, action_dim=r['action_dim'], action_scale_v=r['action_scale_v'], action_scale_p=r['action_scale_p'],
                             boundary=lib.make_boundary(**r['boundary']))
        eng.eff_set_mesh(e, r['voxels'], r['T'], friction=r['friction'], softness=r['softness'])
        effs.append(e)
    eng.set_option('collide_type', sc['collide_type'])
    for e, r in zip(effs, sc['tools']):
        st0 = eng.eff_get_state(e, 0)
        st0[:7] = r['init_state']
        eng.eff_set_state(e, 0, st0)
        eng.eff_apply_action_p(e, r['action_p'])
    return eng, effs


def _chain_classify(dyns, cols, x, nv, dt, node):
    """the colliders in order, as contact_ref.dynamic_chain runs them, each input classified -> (sure, hit count per row, velocity behind the chain).
    A miss is sure when sd keeps the margin to its branch edges: it samples no normal, and across a cell face the trilinear field is continuous."""
    sure, hits, nv = np.ones(len(x), bool), np.zeros(len(x), int), nv.copy()
    for dyn, col in zip(dyns, cols):
        pos = x if node else x + dt * nv
        cases = np.concatenate([np.tile(np.concatenate([dyn['pos0'], dyn['quat0'], dyn['pos1'], dyn['quat1']]), (len(x), 1)), pos, nv], axis=1)
        fs = np.tile([dyn['friction'], dyn['softness']], (len(x), 1))
        c, hit = G.classify(col, cases, fs, dt=dt)
        s, _, _ = G.verdict(col, c, hit, fs)
        sd = c[:, G.C_SD]
        edge_ok = (np.abs(sd) >= G.MARGIN) & ((dyn['softness'] <= 0) | (np.abs(sd - np.log(10.0) / max(dyn['softness'], 1e-30)) >= G.MARGIN))
        sure &= np.where(hit, s, edge_ok)
        hits += hit
        nv = R.M.dynamic_collide(dyn, pos, nv, dt)
    return sure, hits, nv


def classify_two(sc, eng, effs):
    """after the first substep of the fp64 oracle: node level (every massy node through both colliders) and particle level (the gathered velocity through both)"""
    st0 = S.get_state(eng, 0)
    x, v, C, F = (st0[k].astype(np.float64) for k in 'xvCF')
    used = st0['used'].astype(bool)
    n, dt = sc['n_grid'], sc['dt']
    dyns, cols = [], []
    for e, r in zip(effs, sc['tools']):
        p0, p1 = eng.eff_get_state(e, 0).astype(np.float64), eng.eff_get_state(e, 1).astype(np.float64)
        dyns.append(dict(voxels=np.asarray(r['voxels'], np.float64), T=r['T'], friction=float(np.float32(r['friction'])), softness=float(np.float32(r['softness'])),
                         pos0=p0[:3], quat0=p0[3:7], pos1=p1[:3], quat1=p1[3:7]))
        cols.append(G.colliders()[r['col']])
    g_p, g_m = R.p2g_liquid(x, v, C, F, st0['used'], mass64(sc), lam64(sc), n, dt, (0.5 / n) ** 2)
    occ = g_m > R.EPS
    xn = np.stack(np.nonzero(occ), 1) / float(n)
    vo = g_p[occ] / g_m[occ][:, None] + dt * S.f32(sc['gravity']).astype(np.float64)
    node_sure, node_hits, _ = _chain_classify(dyns, cols, xn, vo, dt, True)
    v_out, _, _ = R.node_chain(g_p, g_m, n, dt, S.f32(sc['gravity']).astype(np.float64), sc['boundary'], (), dyns, True, -1e30, [R.new_record() for _ in dyns], [])
    nv = R.gather(x[used], v_out, n)
    sure_u, hits_u, v1_u = _chain_classify(dyns, cols, x[used], nv, dt, False)
    N = len(x)
    sure, hits, v1 = np.ones(N, bool), np.zeros(N, int), np.zeros((N, 3))
    sure[used], hits[used], v1[used] = sure_u, hits_u, v1_u
    return dict(sure=sure, contact=hits > 0, both=hits == 2, v1_ref=v1, node_unsure=int((~node_sure).sum()), node_hits=int((node_hits > 0).sum()),
                node_both=int((node_hits == 2).sum()), branch=np.zeros(N, int))


def run_two(lib, sc, sure=None, classify=False):
    """one substep of the two-tool scene forward; with `sure` backward from the masked cotangent.  action_grad: both effectors' rows, stacked"""
    eng, effs = two_tool_engine(lib, sc)
    for e, r in zip(effs, sc['tools']):
        eng.eff_set_action(e, 0, 0, sc['n_substeps'], r['action'])
    eng.step(0, 0, 1, 1)
    f1 = S.get_state(eng, 1)
    out = dict(v1=f1['v'].astype(np.float64), used=f1['used'].astype(bool))
    if classify:
        out['cls'] = classify_two(sc, eng, effs)
        sure = out['cls']['sure'] if sure is None else sure
    if sure is not None:
        cot = cotangent(sc, sure)
        eng.reset_grad()
        eng.add_grad(1, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        eng.step_grad(0, 0, 1, 1)
        grads = []
        for e, r in zip(effs, sc['tools']):
            eng.eff_set_action_grad(e, 0, 0, sc['n_substeps'])
            eng.eff_apply_action_p_grad(e)
            grads.append(np.asarray(eng.eff_get_action_grad(e, 0, sc['horizon'], r['action_dim']), np.float64))
        g = eng.get_grad(0)
        out.update(gx=g[0].astype(np.float64), gv=g[1].astype(np.float64), action_grad=np.concatenate([a.reshape(-1) for a in grads]))
    eng.close()
    return out
