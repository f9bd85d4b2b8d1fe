"""The smoke solver's edge cases, shared by the CPU checks of the oracle (test_smoke_cases.py) and the HIP-vs-oracle parity tests
(test_smoke_hip_stages.py): the case table, the static obstacles, the inputs (drawn once from a fixed seed and rounded to fp32, so
every engine starts from the same bits) and the drivers that step an engine of any precision through them."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
import mpm_numpy  # noqa: E402
import scenarios as S  # noqa: E402
import smoke_numpy  # noqa: E402
from fluidlab_amd._capi import Engine, FE_EFF_AIRCON  # noqa: E402

U = 2.0 ** -24                       # fp32 unit roundoff
DT = float(np.float32(0.03))
INJECT_V = (-0.3, 0.1, 1.0)
FIELDS = ('v', 'v_tmp', 'div', 'p', 'q')

#        name             res  ly  hy  q_dim iters statics    v scale
_TABLE = [
    ('base',           12,  3,  8, 1, 12, 'box',     1.5),
    ('q3',             12,  3,  8, 3,  7, 'box',     1.5),
    ('q2-one-sweep',   12,  3,  8, 2,  1, 'two',     1.5),
    ('walls',          12, -1, 12, 1,  7, 'box',     1.5),
    ('beyond',         12, -3, 14, 2,  6, 'two',     1.5),
    ('one-layer',      12,  5,  7, 1,  5, 'none',    1.5),
    ('empty',          12,  5,  6, 1,  5, 'none',    1.5),
    ('tiny',            4,  0,  2, 1,  3, 'none',    1.5),
    ('all-free-odd',    5, -1,  5, 3,  4, 'none',    1.5),
    ('pocket',         13,  2,  9, 1,  9, 'pocket',  1.5),
    ('fast-walls',     12, -1, 12, 1,  7, 'box',   120.0),
    ('fast-pocket',    13,  2,  9, 2,  8, 'pocket', 120.0),
    ('no-sweeps',      12,  3,  8, 1,  0, 'box',     1.5),
]
CASES = {t[0]: dict(name=t[0], res=t[1], ly=t[2], hy=t[3], q_dim=t[4], iters=t[5], statics=t[6], vscale=t[7]) for t in _TABLE}
NAMES = [t[0] for t in _TABLE]
FAST = [n for n in NAMES if CASES[n]['vscale'] > 10]

# the pocket obstacle (res 13, slab 2 < j < 9): a solid block over the slab's whole height with three cavities
POCKET_BLOCK = (slice(4, 9), slice(3, 9), slice(4, 9))
POCKET_ISOLATED = (6, 5, 6)                  # free, all six neighbours solid
POCKET_PAIR = ((5, 7, 5), (5, 7, 6))         # free, each other's only free neighbour
POCKET_DEAD_END = (8, 4, 6)                  # free, its only free neighbour (9, 4, 6) is in the open space


def _box_voxels(centre, half, vres=16):
    g = np.linspace(0, 1, vres)
    X, Y, Z = np.meshgrid(g, g, g, indexing='ij')
    q = np.abs(np.stack([X - centre[0], Y - centre[1], Z - centre[2]], -1)) - list(half)
    return np.linalg.norm(np.maximum(q, 0), axis=-1) + np.minimum(q.max(-1), 0)


def _scaling(s):
    T = np.eye(4); T[:3, :3] *= float(s)
    return T


def _pocket_voxels(res=13):
    """An SDF-like field on 2 res + 1 voxels (T = 2 res): the centre of cell i sits on voxel node 2 i + 1, and nodes 2 i and 2 i + 1
    both carry cell i's value (-1 solid, +1 free), so a sample at a cell centre is +-1 whichever way the fp32 coordinate rounds."""
    solid = np.zeros((res, res, res), bool)
    solid[POCKET_BLOCK] = True
    for c in (POCKET_ISOLATED,) + POCKET_PAIR + (POCKET_DEAD_END,):
        solid[c] = False
    node_cell = np.minimum(np.arange(2 * res + 1) // 2, res - 1)
    val = np.where(solid, -1.0, 1.0)
    return val[np.ix_(node_cell, node_cell, node_cell)]


def statics_of(case):
    """[(voxels as fp32 values, T_mesh_to_voxels)] of a case"""
    kind = case['statics']
    box = (_box_voxels((0.62, 0.45, 0.4), (0.1, 0.3, 0.12)), _scaling(15.0))             # the obstacle of test_smoke.py
    wall_box = (_box_voxels((0.04, 0.47, 0.75), (0.13, 0.3, 0.11)), _scaling(15.0))     # reaches through the x = 0 wall
    if kind == 'pocket':
        out = [(_pocket_voxels(case['res']), _scaling(2 * case['res']))]
    else:
        out = {'none': [], 'box': [box], 'two': [box, wall_box]}[kind]
    return [(S.f32(v).astype(np.float64), T) for v, T in out]


def static_sdf_at_centres(case):
    """per static: the SDF sample at every cell centre (voxel units) and the field's largest change over one voxel"""
    n = case['res']
    g = (np.arange(n) + 0.5) / n
    pts = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)
    out = []
    for vox, T in statics_of(case):
        sd = mpm_numpy._sdf_sample(vox, pts @ T[:3, :3].T + T[:3, 3]).reshape(n, n, n)
        lip = max(np.abs(np.diff(vox, axis=a)).max() for a in range(3))
        out.append((sd, lip))
    return out


def free_mask(case):
    """the numpy free mask of a case (Static.is_collide, static.py:107-113, for every static)"""
    sts = statics_of(case)

    def solid(pts):
        hit = np.zeros(len(pts), bool)
        for vox, T in sts:
            hit |= mpm_numpy._sdf_sample(vox, pts @ T[:3, :3].T + T[:3, 3]) <= 0
        return hit
    return smoke_numpy.free_space(case['res'], case['ly'], case['hy'], solid if sts else None)


def free_neighbours(free):
    """number of free, in-range 6-neighbours of every cell"""
    pad = np.pad(free, 1, constant_values=False).astype(int)
    n = free.shape[0]
    cnt = np.zeros(free.shape, int)
    for ax in range(3):
        for sh in (0, 2):
            idx = [slice(1, n + 1)] * 3
            idx[ax] = slice(sh, sh + n)
            cnt += pad[tuple(idx)]
    return cnt


def near_wall_mask(free):
    """cells that are not free (outside the slab, inside a static) plus every cell with such a cell, or the domain wall, next to it"""
    return (~free) | (free_neighbours(free) < 6)


def inputs(case, seed=0):
    """v0, q0, p0 of frame 0 as fp64 arrays holding fp32 values; q is set outside the slab as well, so that its carry-over shows"""
    n, qd = case['res'], case['q_dim']
    rng = np.random.RandomState(seed)
    v0 = rng.normal(0, case['vscale'], (n, n, n, 3))
    j = np.arange(n)
    slab = ((j > case['ly']) & (j < case['hy']))[None, :, None, None]
    q0 = np.where(slab, 1.0, 0.25) * (1 + 0.3 * rng.normal(size=(n, n, n, qd)))
    p0 = rng.normal(0, 0.3, (n, n, n))
    return tuple(S.f32(a).astype(np.float64) for a in (v0, q0, p0))


def actions(H=3, seed=1):
    rng = np.random.RandomState(seed)
    a = np.zeros((H, 8))
    a[:, :3] = rng.uniform(-0.02, 0.02, (H, 3)); a[:, 3:6] = rng.uniform(-0.2, 0.2, (H, 3))
    a[:, 6] = rng.uniform(0.5, 1.0, H); a[:, 7] = rng.uniform(0.6, 1.2, H)
    return S.f32(a).astype(np.float64)


def make_engine(elib, case, action_steps=4, max_steps_local=None, device=0, perturb=None, set_inputs=True):
    """The room of test_smoke.py generalised: slab, q_dim, statics, velocity scale and ring length from the case.  The effector and
    particle rings hold all `action_steps` steps (2 substeps each); the smoke ring holds `max_steps_local` of them."""
    n = case['res']
    eng = Engine(elib, n_grid=8, n_particles=4, max_substeps_local=action_steps * 2, n_substeps=2, max_action_steps=action_steps, dt=2e-4,
                 p_vol=(0.5 / 8) ** 2, gravity=(0.0, -10.0, 0.0), boundary=elib.make_boundary(), device=device)
    eng.init_particles(S.f32(np.full((4, 3), -100.0)), np.zeros(4, np.int32), np.zeros(4, np.int32), np.full(4, 200, np.int32),
                       np.zeros(4), np.full(4, 277.78), np.ones(4), np.zeros(4, np.int32))
    for vox, T in statics_of(case):
        eng.add_static(S.f32(vox), T, friction=0.0)
    e = eng.add_effector(type=FE_EFF_AIRCON, action_dim=8, action_scale_v=(1, 1, 1, 1, 1, 1, 40.0, 3.0), action_scale_p=(1,) * 8,
                         boundary=elib.make_boundary(), inject_v=INJECT_V)
    st = eng.eff_get_state(e, 0)
    st[:7] = S.f32(np.array([0.3, 0.45, 0.25, 0.9689124, 0.0, 0.2474040, 0.0]))
    eng.eff_set_state(e, 0, st)
    eng.smoke_create(res=n, dt=DT, solver_iters=case['iters'], q_dim=case['q_dim'],
                     max_steps_local=action_steps if max_steps_local is None else max_steps_local, lower_y=case['ly'], higher_y=case['hy'])
    if set_inputs:
        v0, q0, p0 = inputs(case)
        if perturb is not None:                   # (field, index, delta) for finite differences
            {'v': v0, 'q': q0, 'p': p0}[perturb[0]][perturb[1]] += perturb[2]
        eng.smoke_set_frame(0, v=v0, q=q0, p=p0)
    return eng, e


def aircon_at(eng, e, f):
    st = eng.eff_get_state(e, f)
    sa, ra = eng.eff_get_sr(e, f)
    return dict(pos=st[:3].astype(np.float64), quat=st[3:7].astype(np.float64), inject_v=INJECT_V, s=sa, r=ra)


def as64(d):
    return {k: np.asarray(a, np.float64) for k, a in d.items()}


def one_step(elib, case, cots=(), device=0):
    """One smoke step with every action component in play: the action drives one substep, so the AirCon the smoke step reads (frame 1)
    has moved, turned and taken its strength and radius from it.  Returns the stage fields, and per cotangent (cot_v, cot_q) on frame 1
    the adjoints at frame 0 and the action gradient [8]."""
    eng, e = make_engine(elib, case, action_steps=1)
    act = actions(1)[0]
    eng.eff_set_action(e, 0, 0, 2, act)
    eng.step(0, 0, 1, 1)
    eng.smoke_step(0, 1)
    out = as64(eng.smoke_get_frame(0, ('v_tmp', 'div')))
    f1 = as64(eng.smoke_get_frame(1, ('v', 'q', 'p')))
    out.update(v1=f1['v'], q1=f1['q'], p1=f1['p'], aircon=aircon_at(eng, e, 1), grads=[])
    for cot_v, cot_q in cots:
        eng.reset_grad()
        eng.smoke_add_grad(1, gv=cot_v, gq=cot_q)
        eng.smoke_step_grad(0, 1)
        eng.step_grad(0, 0, 1, 1)
        eng.eff_set_action_grad(e, 0, 0, 2)
        gv0, gq0 = eng.smoke_get_grad(0)
        out['grads'].append(dict(gv0=gv0.astype(np.float64), gq0=gq0.astype(np.float64),
                                 action=eng.eff_get_action_grad(e, 0, 1, 8)[0].astype(np.float64)))
    eng.close()
    return out


def run_steps(elib, case, acts, cot_v=None, cot_q=None, device=0, perturb=None):
    """test_smoke.run_smoke for a case: H steps of (set_action, smoke_step, the step's substeps); with a cotangent on the last frame,
    loss = <cot, (v, q)[H]> and its gradient with respect to the actions and to frame 0."""
    H = len(acts)
    eng, e = make_engine(elib, case, action_steps=max(H, 1), device=device, perturb=perturb)
    for s in range(H):
        eng.eff_set_action(e, s, s, 2, acts[s])
        eng.smoke_step(s, 2 * s)
        eng.step(2 * s, 2 * s, 2, 1)
    out = dict(final=as64(eng.smoke_get_frame(H, ('v', 'q', 'p'))))
    if cot_v is not None:
        out['loss'] = float((out['final']['v'] * cot_v).sum() + (out['final']['q'] * cot_q).sum())
        eng.reset_grad()
        eng.smoke_add_grad(H, gv=cot_v, gq=cot_q)
        for s in reversed(range(H)):
            eng.step_grad(2 * s, 2 * s, 2, 1)
            eng.smoke_step_grad(s, 2 * s)
            eng.eff_set_action_grad(e, s, s, 2)
        gv0, gq0 = eng.smoke_get_grad(0)
        out.update(action_grad=eng.eff_get_action_grad(e, 0, H, 8)[:H].astype(np.float64), gv0=gv0.astype(np.float64), gq0=gq0.astype(np.float64))
    eng.close()
    return out


def cotangents(case, free, seed=3):
    """the three cotangent patterns on (v, q) of the last frame, fp32 values: dense; v only, on the cells at walls, obstacles and outside
    the slab; q only"""
    n, qd = case['res'], case['q_dim']
    rng = np.random.RandomState(seed)
    cv, cq = S.f32(rng.normal(size=(n, n, n, 3))).astype(np.float64), S.f32(rng.normal(size=(n, n, n, qd))).astype(np.float64)
    return {'dense': (cv, cq), 'v-at-walls': (cv * near_wall_mask(free)[..., None], np.zeros_like(cq)), 'q-only': (np.zeros_like(cv), cq)}
