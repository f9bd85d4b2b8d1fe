"""The scene part of the renderer's contract (include/fluidengine_ext.h, "The scene in that picture") restated in numpy, fp64, operation for
operation, on top of tests/render_ref.py, which restates the spheres.  A helper, not a test; written from the header's text.

render_scene() returns id, depth, rgb and a `fragile` mask.  Fragile pixels are those where a colour channel (or, for a smoke cell, a
channel of its base colour) lies within 1e-9 of a rounding boundary of the byte rule, and those whose nearest sphere fragment and nearest
volume fragment lie within 4 fp32 ulps of each other."""
import numpy as np

import render_ref as RR

MAX_SETS, MAX_POINTS, MAX_VOLUMES, MAX_MARCH = 2, 1 << 20, 16, 4096
BG = RR.BG


def vol_id0(N):
    return N + MAX_SETS * MAX_POINTS


def cell_id0(N):
    return vol_id0(N) + MAX_VOLUMES


def volume(vox, T_mesh_to_voxels, rgba, pos=None, quat=None):
    """a volume as the engine holds it: fp32 voxels [res]^3, rows 0..2 of T as fp32, Rinv = inverse(T[:3, :3]) formed in fp64 by cofactors and
    rounded to fp32 (fe_add_static), and for an effector the fp32 pose words of the frame drawn"""
    vox = np.ascontiguousarray(vox, np.float32)
    T = np.asarray(T_mesh_to_voxels, np.float64).reshape(4, 4).astype(np.float32)[:3].reshape(12).copy()
    A = [[float(T[r * 4 + c]) for c in range(3)] for r in range(3)]
    det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + \
        A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0])
    Rinv = np.zeros(9, np.float32)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            Rinv[j * 3 + i] = np.float32((A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1]) / det)
    return dict(res=int(vox.shape[0]), vox=vox, T=T, Rinv=Rinv, rgba=np.asarray(rgba, np.uint8).reshape(4),
                p=None if pos is None else np.asarray(pos, np.float32).reshape(3), q=None if quat is None else np.asarray(quat, np.float32).reshape(4))


def _qrot(v, q):
    ux = q[2] * v[2] - q[3] * v[1]; uy = q[3] * v[0] - q[1] * v[2]; uz = q[1] * v[1] - q[2] * v[0]
    wx = q[2] * uz - q[3] * uy; wy = q[3] * ux - q[1] * uz; wz = q[1] * uy - q[2] * ux
    return [v[0] + 2.0 * (q[0] * ux + wx), v[1] + 2.0 * (q[0] * uy + wy), v[2] + 2.0 * (q[0] * uz + wz)]


def ray(cam, V):
    """per pixel [H, W]: d (world), ov, dv (voxels), and the normalised pose quaternion"""
    W, H = cam['width'], cam['height']
    ii, jj = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    a = ((ii + 0.5) - 0.5 * float(W)) / cam['focal']
    b = ((jj + 0.5) - 0.5 * float(H)) / cam['focal']
    d = [(float(cam['fwd'][c]) + a * float(cam['right'][c])) - b * float(cam['up'][c]) for c in range(3)]
    o = [float(cam['pos'][c]) for c in range(3)]
    dm = d
    q = [1.0, 0.0, 0.0, 0.0]
    if V['p'] is not None:
        q0, q1, q2, q3 = (float(v) for v in V['q'])
        qn = 1.0 / np.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
        q = [q0 * qn, q1 * qn, q2 * qn, q3 * qn]
        qi = [q[0], -q[1], -q[2], -q[3]]
        o = _qrot([o[c] - float(V['p'][c]) for c in range(3)], qi)
        dm = _qrot(d, qi)
    T = [float(v) for v in V['T']]
    ov = [((T[c * 4] * o[0] + T[c * 4 + 1] * o[1]) + T[c * 4 + 2] * o[2]) + T[c * 4 + 3] for c in range(3)]
    dv = [(T[c * 4] * dm[0] + T[c * 4 + 1] * dm[1]) + T[c * 4 + 2] * dm[2] for c in range(3)]
    return d, ov, dv, q


def sample(V, p0, p1, p2):
    """the trilinear sample of t_sdf_sample in fp64, 1 outside [0, res - 1)^3"""
    top = float(V['res'] - 1)
    p0, p1, p2 = np.broadcast_arrays(np.asarray(p0, np.float64), np.asarray(p1, np.float64), np.asarray(p2, np.float64))
    with np.errstate(invalid='ignore'):
        ins = (p0 >= 0.0) & (p0 < top) & (p1 >= 0.0) & (p1 < top) & (p2 >= 0.0) & (p2 < top)
    q0, q1, q2 = (np.where(ins, p, 0.0) for p in (p0, p1, p2))
    b0, b1, b2 = q0.astype(np.int64), q1.astype(np.int64), q2.astype(np.int64)
    f0, f1, f2 = q0 - b0, q1 - b1, q2 - b2
    g0, g1, g2 = 1.0 - f0, 1.0 - f1, 1.0 - f2
    v = V['vox'].astype(np.float64)
    sd = g0 * g1 * g2 * v[b0, b1, b2]
    sd = sd + g0 * g1 * f2 * v[b0, b1, b2 + 1]
    sd = sd + g0 * f1 * g2 * v[b0, b1 + 1, b2]
    sd = sd + g0 * f1 * f2 * v[b0, b1 + 1, b2 + 1]
    sd = sd + f0 * g1 * g2 * v[b0 + 1, b1, b2]
    sd = sd + f0 * g1 * f2 * v[b0 + 1, b1, b2 + 1]
    sd = sd + f0 * f1 * g2 * v[b0 + 1, b1 + 1, b2]
    sd = sd + f0 * f1 * f2 * v[b0 + 1, b1 + 1, b2 + 1]
    return np.where(ins, sd, 1.0)


def march(cam, V, march_step=0.5, bisect_iters=10):
    """(hit bool [H, W], depth float32 [H, W]) of one volume, and the ray for the shading"""
    d, ov, dv, q = ray(cam, V)
    H, W = cam['height'], cam['width']
    ov = [np.broadcast_to(np.asarray(o, np.float64), (H, W)) for o in ov]
    top = float(V['res'] - 1)
    t0 = np.full((H, W), float(cam['near']))
    t1 = np.full((H, W), 1e300)
    miss = np.zeros((H, W), bool)
    with np.errstate(divide='ignore', invalid='ignore'):
        for c in range(3):
            zero = dv[c] == 0.0
            miss |= zero & ((ov[c] < 0.0) | (ov[c] > top))
            ta = (0.0 - ov[c]) / dv[c]
            tb = (top - ov[c]) / dv[c]
            sw = ta > tb
            ta, tb = np.where(sw, tb, ta), np.where(sw, ta, tb)
            t0 = np.where(~zero & (ta > t0), ta, t0)
            t1 = np.where(~zero & (tb < t1), tb, t1)
        live = ~miss & (t0 <= t1)
        dt = float(march_step) / np.sqrt((dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2])
        kd = np.where(live, (t1 - t0) / dt, 0.0)
    K = np.where(kd >= float(MAX_MARCH), MAX_MARCH, np.minimum(kd, float(MAX_MARCH)).astype(np.int64))
    hit = np.zeros((H, W), bool)
    depth = np.full((H, W), np.inf, np.float32)

    def at(t, m):
        return sample(V, ov[0][m] + t * dv[0][m], ov[1][m] + t * dv[1][m], ov[2][m] + t * dv[2][m])
    tp = t0.copy()
    for k in range(int(K[live].max()) + 1 if live.any() else 0):
        m = live & ~hit & (k <= K)
        if not m.any():
            break
        t = t0[m] + float(k) * dt[m]
        neg = at(t, m) <= 0.0
        if neg.any():
            mh = np.zeros((H, W), bool)
            mh[m] = neg
            lo, hi = tp[mh], t[neg]
            if k > 0:
                for _ in range(int(bisect_iters)):
                    mid = 0.5 * (lo + hi)
                    inside = at(mid, mh) <= 0.0
                    hi = np.where(inside, mid, hi)
                    lo = np.where(inside, lo, mid)
            depth[mh] = hi.astype(np.float32)
            hit |= mh
        tp[m] = t
    return hit, depth, (d, ov, dv, q)


def _light(lights, n, P, base):
    """raw channel values base / 255 (ambient + sum colour max(0, n.l)), [3][...]"""
    acc = [np.full(np.shape(P[0]), float(lights['ambient'][a])) for a in range(3)]
    for k in range(len(lights['pos'])):
        l0, l1, l2 = (float(lights['pos'][k][a]) - P[a] for a in range(3))
        ln = np.sqrt((l0 * l0 + l1 * l1) + l2 * l2)
        ok = ln > 0.0
        ndl = ((n[0] * l0 + n[1] * l1) + n[2] * l2) / np.where(ok, ln, 1.0)
        ok = ok & (ndl > 0.0)
        for a in range(3):
            acc[a] = np.where(ok, acc[a] + float(lights['color'][k][a]) * ndl, acc[a])
    return [(base[a] / 255.0) * acc[a] for a in range(3)]


def shade_volume(cam, lights, V, rayv, depth, m):
    """raw channels [3][n] of the pixels m of volume V at their stored depths"""
    d, ov, dv, q = rayv
    t = depth[m].astype(np.float64)
    delta = 1e-2
    pv = [ov[c][m] + t * dv[c][m] for c in range(3)]
    g = []
    for c in range(3):
        inc = [pv[a] + delta if a == c else pv[a] for a in range(3)]
        dec = [pv[a] - delta if a == c else pv[a] for a in range(3)]
        g.append((sample(V, *inc) - sample(V, *dec)) / (2.0 * delta))
    Ri = [float(v) for v in V['Rinv']]
    n = [(Ri[c * 3] * g[0] + Ri[c * 3 + 1] * g[1]) + Ri[c * 3 + 2] * g[2] for c in range(3)]
    if V['p'] is not None:
        n = _qrot(n, q)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = (ln > 0.0) & (ln < 1e300)
        n = [np.where(ok, n[c] / np.where(ok, ln, 1.0), 0.0 - float(cam['fwd'][c])) for c in range(3)]
    dd = [d[c][m] for c in range(3)]
    flip = (n[0] * dd[0] + n[1] * dd[1]) + n[2] * dd[2] > 0.0
    n = [np.where(flip, 0.0 - n[c], n[c]) for c in range(3)]
    P = [float(cam['pos'][c]) + t * dd[c] for c in range(3)]
    return _light(lights, n, P, [float(V['rgba'][a]) for a in range(3)])


def cell_centres(n, lo, hi):
    """(x float32 [m, 3], linear cell index [m]) of the slab lo < j < hi, all i and k"""
    i, j, k = np.meshgrid(np.arange(n), np.arange(lo + 1, hi), np.arange(n), indexing='ij')
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    inv = np.float32(1.0) / np.float32(n)
    x = np.stack([(c.astype(np.float32) + np.float32(0.5)) * inv for c in (i, j, k)], axis=1).astype(np.float32)
    return x, (i * n + j) * n + k


def cell_colours(q, cold, hot):
    """(bytes uint8 [m, 3], near a rounding boundary bool [m]) from q float32 [m]"""
    q = np.asarray(q, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        raw = np.stack([float(cold[a]) * (1.0 - q) + float(hot[a]) * q for a in range(3)], axis=1)
        return RR.byte(raw), _near_boundary(raw).any(axis=1)


def _near_boundary(c):
    with np.errstate(invalid='ignore'):
        c = np.where(c >= 0.0, c, 0.0)
        c = np.where(c > 1.0, 1.0, c)
    v = c * 255.0 + 0.5
    return np.abs(v - np.round(v)) <= 1e-9


def render_scene(cam, lights, N, x=None, ids=None, radius=0.0, rgba=None, volumes=(), smoke=None, march_step=0.5, bisect_iters=10):
    """x, ids, radius, rgba: the spheres to draw other than cells (render_ref.render's arguments: used particles and point sets with their ids).
    volumes: [(slot, volume(...))].  smoke: None or dict(n, lo, hi, q float32 [n, n, n] (component 0 of the frame drawn), radius, cold, hot).
    Returns dict(rgb, depth, id, fragile, covered)."""
    W, H = cam['width'], cam['height']
    xs = np.zeros((0, 3), np.float32) if x is None else np.asarray(x, np.float32).reshape(-1, 3)
    n_sph = len(xs)
    sid = np.zeros(0, np.int64) if ids is None else np.asarray(ids, np.int64).reshape(-1)
    rad = np.broadcast_to(np.asarray(radius, np.float64), (n_sph,)).copy()
    col = np.zeros((0, 4), np.uint8) if rgba is None else np.asarray(rgba, np.uint8).reshape(-1, 4)
    base_fragile = np.zeros(n_sph, bool)
    if smoke is not None:
        cx, lin = cell_centres(smoke['n'], smoke['lo'], smoke['hi'])
        cb, cf = cell_colours(np.asarray(smoke['q'], np.float32).reshape(-1)[lin], smoke['cold'], smoke['hot'])
        xs = np.concatenate([xs, cx]); sid = np.concatenate([sid, cell_id0(N) + lin])
        rad = np.concatenate([rad, np.full(len(cx), float(smoke['radius']))])
        col = np.concatenate([col, np.concatenate([cb, np.full((len(cb), 1), 255, np.uint8)], axis=1)])
        base_fragile = np.concatenate([base_fragile, cf])
    # spheres: the nearest fragment per pixel
    key_s = np.full((H, W), BG, np.uint64)
    who = np.full((H, W), -1, np.int64)
    U = np.zeros((H, W)); V_ = np.zeros((H, W)); NZ = np.zeros((H, W))
    for k in range(len(xs)):
        sp = RR.project(cam, xs[k], rad[k])
        if sp is None or sp['i1'] < sp['i0'] or sp['j1'] < sp['j0']:
            continue
        jj, ii, cov, u, v, nz, dep, _ = RR.fragments(sp)
        key = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(int(sid[k]))
        better = cov & (key < key_s[jj, ii])
        jb, ib = jj[better], ii[better]
        key_s[jb, ib] = key[better]
        who[jb, ib] = k
        U[jb, ib] = u[better]; V_[jb, ib] = v[better]; NZ[jb, ib] = nz[better]
    # volumes
    key_v = np.full((H, W), BG, np.uint64)
    whov = np.full((H, W), -1, np.int64)
    rays = {}
    for slot, V in volumes:
        hit, dep, rv = march(cam, V, march_step, bisect_iters)
        rays[slot] = rv
        key = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(vol_id0(N) + slot)
        better = hit & (key < key_v)
        key_v[better] = key[better]
        whov[better] = slot
    key = np.minimum(key_s, key_v)
    covered = key != BG
    bits = (key >> np.uint64(32)).astype(np.uint32)
    depth = np.where(covered, bits.view(np.float32), np.float32(np.inf)).astype(np.float32)
    idimg = np.where(covered, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    both = (key_s != BG) & (key_v != BG)
    gap = np.abs((key_s >> np.uint64(32)).astype(np.int64) - (key_v >> np.uint64(32)).astype(np.int64))
    fragile = both & (gap <= 4)
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = RR.byte(np.asarray(lights['background'], np.float64))
    ms = covered & (key == key_s)
    if ms.any():
        w = who[ms]
        u, v, nz = U[ms], V_[ms], NZ[ms]
        n = [(u * cam['right'][a] - v * cam['up'][a]) - nz * cam['fwd'][a] for a in range(3)]
        P = [xs[w, a].astype(np.float64) + rad[w] * n[a] for a in range(3)]
        raw = np.stack(_light(lights, n, P, [col[w, a].astype(np.float64) for a in range(3)]), axis=1)
        rgb[ms] = RR.byte(raw)
        fragile[ms] |= _near_boundary(raw).any(axis=1) | base_fragile[w]
    for slot, V in volumes:
        m = covered & (key == key_v) & (whov == slot)
        if m.any():
            raw = np.stack(shade_volume(cam, lights, V, rays[slot], depth, m), axis=1)
            rgb[m] = RR.byte(raw)
            fragile[m] |= _near_boundary(raw).any(axis=1)
    return dict(rgb=rgb, depth=depth, id=idimg, fragile=fragile, covered=covered)


def compare(ref, rgba, depth, ids, max_fragile=0.005):
    """the rule of the GPU tests: id and depth bit for bit; RGB within one level outside `fragile`; fragile at most 0.5 % of the covered
    pixels.  Returns a list of complaints (empty: equal)."""
    bad = []
    if not np.array_equal(ids, ref['id']):
        bad.append(f"id differs on {int((ids != ref['id']).sum())} pixels")
    if not np.array_equal(np.asarray(depth, np.float32).view(np.uint32), ref['depth'].view(np.uint32)):
        bad.append(f"depth bits differ on {int((np.asarray(depth, np.float32).view(np.uint32) != ref['depth'].view(np.uint32)).sum())} pixels")
    ok = ~ref['fragile']
    d = np.abs(rgba[..., :3].astype(np.int32) - ref['rgb'].astype(np.int32))[ok]
    if d.size and d.max() > 1:
        bad.append(f'rgb off by up to {int(d.max())} levels on {int((d.max(axis=-1) > 1).sum())} robust pixels')
    nf, nc = int(ref['fragile'].sum()), int(ref['covered'].sum())
    if nf > max_fragile * max(nc, 1):
        bad.append(f'{nf} fragile pixels of {nc} covered')
    return bad
