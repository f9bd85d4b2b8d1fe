"""TEST INFRASTRUCTURE -- an fp64 numpy restatement of what fe_contact_wrench reports (include/fluidengine_ext.h), built on the forward
pieces of oracle/mpm_numpy.py: `weights`, `static_collide`, `dynamic_collide`, `boundary_v`.

A liquid-only P2G gives the summed (p, m) of every node; the node chain (gravity, the statics in order, the moving colliders when the
engine collides at nodes) and the particle chain (agent.collide on the gathered velocity) then run collider by collider, and after each one
the change of the velocity is booked to that collider: impulse += m dv, ang_impulse += r x m dv, one contact where the collider took its
contact branch.  The domain boundary's change is applied (the gather needs v_out) and booked to nobody.

A moving collider is a dict for oracle.mpm_numpy.dynamic_collide: voxels [res]^3, T (mesh -> voxels, 4x4), friction, softness, pos0, quat0,
pos1, quat1 (the carrier's pose at f and f + 1); None stands for an effector without a mesh.  A static: voxels, T, friction.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import mpm_numpy as M  # noqa: E402

EPS = M.EPS


def new_record():
    return dict(impulse=np.zeros(3), ang_impulse=np.zeros(3), n_particles=0, n_nodes=0, abs_impulse=0.0, abs_ang=0.0, min_abs_sd=np.inf)


def book(rec, m, r, v_in, v_out, hit, node):
    """the contacts `hit` (bool rows) of one collider: m [M], r, v_in, v_out [M,3]"""
    J = m[hit, None] * (v_out[hit] - v_in[hit])
    rec['impulse'] += J.sum(0)
    rec['ang_impulse'] += np.cross(r[hit], J).sum(0)
    rec['abs_impulse'] += float(np.abs(J).sum())                 # sum |m dv| over contacts and axes: what an error is measured against
    rec['abs_ang'] += float(np.abs(np.cross(r[hit], J)).sum())
    rec['n_nodes' if node else 'n_particles'] += int(hit.sum())


def static_sd(static, pos):
    """signed distance sample (voxel units of the lattice's values) of a static at world positions pos [M,3]"""
    T = np.asarray(static['T'], np.float64)
    return M._sdf_sample(np.asarray(static['voxels'], np.float64), pos @ T[:3, :3].T + T[:3, 3])


def dynamic_sd(dyn, pos):
    T, q0 = np.asarray(dyn['T'], np.float64), np.asarray(dyn['quat0'], np.float64)
    qi = np.array([q0[0], -q0[1], -q0[2], -q0[3]]) / np.linalg.norm(q0)
    pm = M._quat_rot(pos - np.asarray(dyn['pos0'], np.float64), qi)
    return M._sdf_sample(np.asarray(dyn['voxels'], np.float64), pm @ T[:3, :3].T + T[:3, 3])


def dynamic_hit(dyn, pos):
    sd = dynamic_sd(dyn, pos)
    infl = np.minimum(np.exp(-sd * dyn['softness']), 1.0)
    return (sd <= 0) | ((dyn['softness'] > 0) & (infl > 0.1)), sd


def dynamic_chain(dynamics, collide_min_y, dt, m, x, nv, recs, node):
    """agent_collide_particle: the colliders in order, pos = x + dt nv re-formed before each (a node's position does not move), skipped
    while pos_y <= collide_min_y.  Returns the velocity behind the chain."""
    nv = nv.copy()
    for e, dyn in enumerate(dynamics):
        if dyn is None:
            continue
        pos = x if node else x + dt * nv
        act = pos[:, 1] > collide_min_y
        if not act.any():
            continue
        hit_a, sd = dynamic_hit(dyn, pos[act])
        out_a = M.dynamic_collide(dyn, pos[act], nv[act], dt)
        hit = np.zeros(len(x), bool); hit[act] = hit_a
        out = nv.copy(); out[act] = out_a
        book(recs[e], m, pos, nv, out, hit, node)
        if len(sd):                                               # distance to where the branch is decided: sd = 0, or the soft branch's infl = 0.1
            edge = np.abs(sd - np.log(10.0) / dyn['softness']) if dyn['softness'] > 0 else np.abs(sd)
            recs[e]['min_abs_sd'] = min(recs[e]['min_abs_sd'], float(edge.min()))
        nv = out
    return nv


def p2g_liquid(x, v, C, F, used, mass, lam, n_grid, dt, p_vol):
    """summed momentum [n,n,n,3] and mass [n,n,n] of the used particles of an inviscid liquid (mpm:254-264, 339-378 with mu = 0)"""
    n, dx, inv_dx = n_grid, 1.0 / n_grid, float(n_grid)
    act = used.astype(bool)
    xs, vs, Cs, Fs, ms, lams = x[act], v[act], C[act], F[act], mass[act], lam[act]
    I = np.eye(3)
    J = np.linalg.det((I + dt * Cs) @ Fs)
    stress = (-dt * p_vol * 4 * inv_dx * inv_dx) * (lams * J * (J - 1))[:, None, None] * I
    affine = stress + ms[:, None, None] * Cs
    base, fx, w = M.weights(xs, inv_dx)
    g_p, g_m = np.zeros((n, n, n, 3)), np.zeros((n, n, n))
    for i in range(3):
        for j in range(3):
            for k in range(3):
                off = np.array([i, j, k])
                wt = w[i][:, 0] * w[j][:, 1] * w[k][:, 2]
                idx = base + off
                np.add.at(g_p, (idx[:, 0], idx[:, 1], idx[:, 2]), wt[:, None] * (ms[:, None] * vs + np.einsum('nab,nb->na', affine, (off - fx) * dx)))
                np.add.at(g_m, (idx[:, 0], idx[:, 1], idx[:, 2]), wt * ms)
    return g_p, g_m


def node_chain(g_p, g_m, n_grid, dt, gravity, bnd, statics, dynamics, node_dyn, collide_min_y, recs_eff, recs_st, eps=EPS):
    """grid_op (mpm:380-398) with bookkeeping.  Returns v_out [n,n,n,3] and the positions, masses and per-static |sd| of the nodes with mass."""
    dx = 1.0 / n_grid
    occ = g_m > eps
    ii, jj, kk = np.nonzero(occ)
    m = g_m[occ]
    xn = np.stack([ii, jj, kk], 1) * dx
    vo = g_p[occ] / m[:, None] + dt * np.asarray(gravity, np.float64)
    for s, st in enumerate(statics):
        sd = static_sd(st, xn)
        out = M.static_collide(st, xn, vo)
        book(recs_st[s], m, xn, vo, out, sd <= 0, True)
        if len(sd):
            recs_st[s]['min_abs_sd'] = min(recs_st[s]['min_abs_sd'], float(np.abs(sd).min()))
        vo = out
    if node_dyn:
        vo = dynamic_chain(dynamics, collide_min_y, dt, m, xn, vo, recs_eff, True)
    v_out = np.zeros(g_p.shape)
    v_out[occ] = M.boundary_v(bnd, xn, vo) if bnd is not None else vo
    return v_out, xn, m


def gather(x, v_out, n_grid):
    """the 27-node B-spline sum of v_out at positions x (mpm:400-414)"""
    base, fx, w = M.weights(x, float(n_grid))
    nv = np.zeros_like(x)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                idx = base + [i, j, k]
                nv += (w[i][:, 0] * w[j][:, 1] * w[k][:, 2])[:, None] * v_out[idx[:, 0], idx[:, 1], idx[:, 2]]
    return nv


def contact_ref(x, v, C, F, used, mass, lam, n_grid, dt, p_vol, gravity, bnd, statics=(), dynamics=(), collide_type=1, collide_min_y=-1e30):
    """The records of one substep: a list, the effectors first (an effector without a mesh: None in `dynamics`, a record of zeros), then
    the statics.  Inputs are frame f in fp64 (widened fp32 words); mass is the engine's fp32 mass, widened."""
    recs_eff = [new_record() for _ in dynamics]
    recs_st = [new_record() for _ in statics]
    has_mesh = any(d is not None for d in dynamics)
    g_p, g_m = p2g_liquid(x, v, C, F, used, mass, lam, n_grid, dt, p_vol)
    v_out, xn, mn = node_chain(g_p, g_m, n_grid, dt, gravity, bnd, statics, dynamics, has_mesh and bool(collide_type & 2), collide_min_y, recs_eff, recs_st)
    if has_mesh and (collide_type & 1):
        act = used.astype(bool)
        dynamic_chain(dynamics, collide_min_y, dt, mass[act], x[act], gather(x[act], v_out, n_grid), recs_eff, False)
    return recs_eff + recs_st, dict(v_out=v_out, node_x=xn, node_m=mn, g_p=g_p, g_m=g_m)
