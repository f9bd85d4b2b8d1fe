"""Shared by test_rigid_bodies_oracle.py (CPU) and test_rigid_bodies_hip.py (GPU): the variants of
scenarios.rigid_bodies_many, oracle rollouts computed once per library and variant, the fp32-oracle yardsticks, and the
shape-matching step of one substep (mpm:449-505) as a plain numpy chain in a chosen precision."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import mpm_numpy  # noqa: E402

N_SUB = 8
GRADS = ('gx', 'gv', 'gC', 'gF')
VARIANTS = dict(plain=dict(), scattered=dict(unused='scattered'), interleave=dict(interleave=True),
                whole_body=dict(unused='whole_body'),
                three=dict(counts=(1213, 768, 169)))       # same N as the eight bodies: what a handle is re-initialised with
UNUSED_BODY = 3                                            # the body unused='whole_body' switches off

_scenes, _rollouts = {}, {}


def scene(variant):
    if variant not in _scenes:
        _scenes[variant] = S.rigid_bodies_many(**VARIANTS[variant])
    return _scenes[variant]


def cotangent(sc, dtype=np.float32):
    return {k: v.astype(dtype) for k, v in S.random_cotangent(sc['N']).items()}


def rollout(lib, variant):
    """N_SUB substeps forward and backward on an oracle library: every frame's state and the frame-0 adjoint.  Computed once."""
    key = (lib.path, variant)
    if key not in _rollouts:
        sc = scene(variant)
        eng = S.make_engine(lib, sc)
        frames = [S.get_state(eng, 0)]
        for f in range(N_SUB):
            eng.substep(f, f, 0)
            frames.append(S.get_state(eng, f + 1))
        cot = cotangent(sc, lib.dtype)
        eng.reset_grad()
        eng.add_grad(N_SUB, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
        for f in reversed(range(N_SUB)):
            eng.substep_grad(f, f, 0)
        _rollouts[key] = dict(frames=frames, final=frames[-1], grad=dict(zip(GRADS, eng.get_grad(0))))
        eng.close()
    return _rollouts[key]


def bodies(sc):
    return range(1, int(sc['body_id'].max()) + 1)


def distances(sc, final, grad, ref, skip=None):
    """d_x: max |dx| over the rigid particles; d_g[k], d_grigid[k]: rel L2 over all / the rigid particles; d_body[b]: rel L2
    of gx over body b -- of (final, grad) against the fp64 rollout `ref`.  skip: particles left out of every figure."""
    keep = np.ones(sc['N'], bool) if skip is None else ~skip
    rigid = (sc['body_id'] > 0) & keep
    return dict(d_x=float(np.abs(final['x'][rigid] - ref['final']['x'][rigid]).max()),
                d_g={k: S.rel_l2(grad[k][keep], ref['grad'][k][keep]) for k in GRADS},
                d_grigid={k: S.rel_l2(grad[k][rigid], ref['grad'][k][rigid]) for k in GRADS},
                d_body={b: S.rel_l2(grad['gx'][(sc['body_id'] == b) & keep], ref['grad']['gx'][(sc['body_id'] == b) & keep])
                        for b in bodies(sc) if ((sc['body_id'] == b) & keep).any()})


def yardstick(oracle32, oracle64, variant, skip=None):
    """distances() of the fp32 oracle from the fp64 oracle on the same rollout: what fp32 arithmetic alone costs here"""
    a = rollout(oracle32, variant)
    return distances(scene(variant), a['final'], a['grad'], rollout(oracle64, variant), skip)


def body_H_singular_values(sc, frame, v_next, b):
    """singular values of body b's H (mpm:464-478) from a frame and the next frame's velocities, fp64; None without used particles"""
    allb = sc['body_id'] == b
    sel = allb & (frame['used'] == 1)
    if not sel.any():
        return None
    x = frame['x'][sel].astype(np.float64)
    y = x + sc['dt'] * v_next[sel].astype(np.float64)
    c0, c1 = x.sum(0) / allb.sum(), y.sum(0) / allb.sum()
    return np.linalg.svd((x - c0).T @ (y - c1), compute_uv=False)


def shape_match(x, v_next, used, body_id, dt, dtype):
    """The rigid branch of one substep for every body, from x[f], used and v[f+1] as read back from an engine (fp32 arrays):
    y = x + dt v,  c0 = sum x / n,  c1 = sum y / n  (n: ALL particles of the body, mpm:201,461),  H = sum (x - c0)(y - c1)^T,
    R = V U^T from numpy's SVD with the sign convention of mpm_numpy.proper_svd,  x' = R (x - c0) + c1
    -- every sum, the SVD and the rotation in `dtype`.  Returns {body: (selection, x' [n_used, 3])}."""
    dt = dtype(np.float32(dt))
    out = {}
    for b in range(1, int(body_id.max()) + 1):
        allb = body_id == b
        sel = allb & (used == 1)
        if not sel.any():
            continue
        xs = x[sel].astype(dtype)
        ys = xs + dt * v_next[sel].astype(dtype)
        n = dtype(allb.sum())
        c0, c1 = xs.sum(0, dtype=dtype) / n, ys.sum(0, dtype=dtype) / n
        H = (xs - c0).T @ (ys - c1)
        U, _, V = mpm_numpy.proper_svd(H[None])
        R = V[0] @ U[0].T
        new = (xs - c0) @ R.T + c1
        assert new.dtype == dtype and H.dtype == dtype and R.dtype == dtype
        out[b] = (sel, new)
    return out


def pairwise(x):
    x = np.asarray(x, np.float64)
    return np.linalg.norm(x[:, None] - x[None], axis=2)
