"""The renderer's contract (include/fluidengine_ext.h, "Headless particle renderer") restated in numpy, operation for operation in fp64: the
same + - * / and sqrt in the same order as fluidlab_amd/csrc/fe_render.h, so that the images can be compared bit for bit.  A helper, not a
test.  Besides the image it reports what a comparison needs to know about the scene: per pixel the second-nearest fragment and a mask
of FRAGILE pixels -- those whose two nearest fragments of different ids lie within 4 fp32 ulps of each other, or on which some fragment
has |s - 1| <= 1e-9 (coverage decided by the last bits).  Two spheres with the same centre words and the same radius are the one exception to
the first rule: every implementation computes the same depth bits for both, and the tie is decided by an integer comparison of the ids, so
the pixels of an identical pair are not fragile."""
import numpy as np

BG = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera(res, pos, lookat, fov, up=(0.0, 1.0, 0.0), near=0.01, max_radius_px=32.0):
    """a plain dict with the fields of FeRenderCamera, the basis built as renderers/hip_renderer.py builds it"""
    pos, at, up = (np.asarray(v, np.float64) for v in (pos, lookat, up))
    fwd = at - pos
    fwd = fwd / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    right = right / np.linalg.norm(right)
    return dict(pos=pos, right=right, up=np.cross(right, fwd), fwd=fwd, focal=float(0.5 * res[1] / np.tan(np.deg2rad(float(fov)) / 2.0)),
                near=float(near), max_radius_px=float(max_radius_px), width=int(res[0]), height=int(res[1]))


def camera_of(c):
    """the same dict from a FeRenderCamera"""
    return dict(pos=np.array(c.pos[:]), right=np.array(c.right[:]), up=np.array(c.up[:]), fwd=np.array(c.fwd[:]), focal=float(c.focal),
                near=float(c.near), max_radius_px=float(c.max_radius_px), width=int(c.width), height=int(c.height))


def lights_of(L):
    n = int(L.n_lights)
    return dict(ambient=np.array(L.ambient[:]), background=np.array(L.background[:]), pos=np.array([L.pos[k][:] for k in range(n)]).reshape(n, 3),
                color=np.array([L.color[k][:] for k in range(n)]).reshape(n, 3))


def _clamp(a, lo, hi):
    return lo if a < lo else (hi if a > hi else a)


def project(cam, xf, R):
    """None, or a dict with zc, px, py, rp, the clipped box i0..i1 x j0..j1 (inclusive) and the centre pixel ci, cj"""
    xf = np.asarray(xf, np.float32)
    if not np.all(np.isfinite(xf)):
        return None
    x = [float(xf[0]), float(xf[1]), float(xf[2])]
    R = float(R)
    W, H = float(cam['width']), float(cam['height'])
    pos, f, r, u = cam['pos'], cam['fwd'], cam['right'], cam['up']
    d0, d1, d2 = x[0] - float(pos[0]), x[1] - float(pos[1]), x[2] - float(pos[2])
    zc = (d0 * float(f[0]) + d1 * float(f[1])) + d2 * float(f[2])
    xc = (d0 * float(r[0]) + d1 * float(r[1])) + d2 * float(r[2])
    yc = (d0 * float(u[0]) + d1 * float(u[1])) + d2 * float(u[2])
    if not zc > cam['near'] + R:
        return None
    px = 0.5 * W + (cam['focal'] * xc) / zc
    py = 0.5 * H - (cam['focal'] * yc) / zc
    rp = (cam['focal'] * R) / zc
    clamped = rp > cam['max_radius_px']
    if clamped:
        rp = cam['max_radius_px']
    return dict(x=x, R=R, zc=zc, px=px, py=py, rp=rp, clamped=clamped,
                i0=int(np.floor(_clamp((px - rp) - 0.5, 0.0, W))), i1=int(np.ceil(_clamp((px + rp) - 0.5, -1.0, W - 1.0))),
                j0=int(np.floor(_clamp((py - rp) - 0.5, 0.0, H))), j1=int(np.ceil(_clamp((py + rp) - 0.5, -1.0, H - 1.0))),
                ci=int(np.floor(_clamp(px, -1.0, W))), cj=int(np.floor(_clamp(py, -1.0, H))))


def fragments(sp):
    """every pixel of the sphere's box: (jj, ii, covered, u, v, nz, depth fp32, s before the centre clamp) as arrays over the box"""
    ii, jj = np.meshgrid(np.arange(sp['i0'], sp['i1'] + 1), np.arange(sp['j0'], sp['j1'] + 1))
    u = ((ii.astype(np.float64) + 0.5) - sp['px']) / sp['rp']
    v = ((jj.astype(np.float64) + 0.5) - sp['py']) / sp['rp']
    s_raw = u * u + v * v
    centre = (ii == sp['ci']) & (jj == sp['cj'])
    covered = (s_raw <= 1.0) | centre
    s = np.where(centre & ~(s_raw <= 1.0), 1.0, s_raw)
    nz = np.sqrt(np.where(covered, 1.0 - s, 0.0))
    depth = (sp['zc'] - sp['R'] * nz).astype(np.float32)
    return jj, ii, covered, u, v, nz, depth, s_raw


def byte(c):
    c = np.where(c >= 0.0, c, 0.0)
    c = np.where(c > 1.0, 1.0, c)
    return (c * 255.0 + 0.5).astype(np.int64).astype(np.uint8)


def render(cam, lights, x, ids, radius, rgba):
    """x float32 [n, 3], ids int [n] (unique), radius fp64 [n] or a scalar, rgba uint8 [n, 4] -- only what is to be drawn (the caller drops unused
    particles).  Returns a dict: rgb uint8 [H, W, 3], depth float32 (+inf background), id int32 (-1), depth2 (the second-nearest fragment of
    another id, +inf where there is none), id2, fragile bool, covered bool, and the counts n_clamped / n_subpixel (rp < 0.5) of drawn spheres."""
    W, H = cam['width'], cam['height']
    x = np.asarray(x, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64).reshape(-1)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (len(x),))
    rgba = np.asarray(rgba, np.uint8).reshape(-1, 4)
    key1 = np.full((H, W), BG, np.uint64)
    key2 = np.full((H, W), BG, np.uint64)
    fragile = np.zeros((H, W), bool)
    U = np.zeros((H, W)); V = np.zeros((H, W)); NZ = np.zeros((H, W))
    who = np.full((H, W), -1, np.int64)                          # index into x of the winner
    who2 = np.full((H, W), -1, np.int64)                         # ... and of the runner-up
    n_clamped = n_subpixel = 0
    for k in range(len(x)):
        sp = project(cam, x[k], radius[k])
        if sp is None or sp['i1'] < sp['i0'] or sp['j1'] < sp['j0']:
            continue
        n_clamped += bool(sp['clamped'])
        n_subpixel += bool(sp['rp'] < 0.5)
        jj, ii, cov, u, v, nz, depth, s_raw = fragments(sp)
        fragile[jj, ii] |= np.abs(s_raw - 1.0) <= 1e-9
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(int(ids[k]))
        jc, ic, kc = jj[cov], ii[cov], key[cov]
        old1 = key1[jc, ic]
        better = kc < old1
        # the displaced best (or the newcomer that lost) competes for second place
        cand2 = np.where(better, old1, kc)
        cand2_who = np.where(better, who[jc, ic], k)
        second = cand2 < key2[jc, ic]
        key2[jc[second], ic[second]] = cand2[second]
        who2[jc[second], ic[second]] = cand2_who[second]
        jb, ib = jc[better], ic[better]
        key1[jb, ib] = kc[better]
        U[jb, ib] = u[cov][better]; V[jb, ib] = v[cov][better]; NZ[jb, ib] = nz[cov][better]
        who[jb, ib] = k
    covered = key1 != BG
    bits1 = (key1 >> np.uint64(32)).astype(np.uint32)
    bits2 = (key2 >> np.uint64(32)).astype(np.uint32)
    has2 = key2 != BG
    w1, w2 = np.maximum(who, 0), np.maximum(who2, 0)
    twins = has2 & np.all(x[w1].view(np.uint32) == x[w2].view(np.uint32), axis=-1) & (radius[w1] == radius[w2])
    fragile |= covered & has2 & ~twins & ((bits2.astype(np.int64) - bits1.astype(np.int64)) <= 4)
    depth = np.where(covered, bits1.view(np.float32), np.float32(np.inf)).astype(np.float32)
    depth2 = np.where(has2, bits2.view(np.float32), np.float32(np.inf)).astype(np.float32)
    idimg = np.where(covered, (key1 & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    id2 = np.where(has2, (key2 & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    # shade
    rgb = np.empty((H, W, 3), np.uint8)
    rgb[:] = byte(np.asarray(lights['background'], np.float64))
    jj, ii = np.nonzero(covered)
    if len(jj):
        w = who[jj, ii]
        u, v, nz = U[jj, ii], V[jj, ii], NZ[jj, ii]
        xs = x[w].astype(np.float64)
        Rs = radius[w]
        n = [(u * cam['right'][a] - v * cam['up'][a]) - nz * cam['fwd'][a] for a in range(3)]
        P = [xs[:, a] + Rs * n[a] for a in range(3)]
        acc = [np.full(len(jj), float(lights['ambient'][a])) for a in range(3)]
        for k in range(len(lights['pos'])):
            l0, l1, l2 = (float(lights['pos'][k][a]) - P[a] for a in range(3))
            ln = np.sqrt((l0 * l0 + l1 * l1) + l2 * l2)
            ok = ln > 0.0
            ndl = ((n[0] * l0 + n[1] * l1) + n[2] * l2) / np.where(ok, ln, 1.0)
            ok &= ndl > 0.0
            for a in range(3):
                acc[a] = np.where(ok, acc[a] + float(lights['color'][k][a]) * ndl, acc[a])
        base = rgba[w].astype(np.float64)
        for a in range(3):
            rgb[jj, ii, a] = byte((base[:, a] / 255.0) * acc[a])
    return dict(rgb=rgb, depth=depth, id=idimg, depth2=depth2, id2=id2, fragile=fragile, covered=covered, n_clamped=n_clamped, n_subpixel=n_subpixel)


def compare(ref, rgba, depth, ids):
    """the rule of the GPU tests: outside fragile pixels id and depth bits equal and RGB within one level; on a fragile pixel the id is one of
    the two nearest.  Returns a list of complaints (empty: equal)."""
    bad = []
    ok = ~ref['fragile']
    if not np.array_equal(ids[ok], ref['id'][ok]):
        bad.append(f"id differs on {int((ids[ok] != ref['id'][ok]).sum())} robust pixels")
    if not np.array_equal(depth[ok].view(np.uint32), ref['depth'][ok].view(np.uint32)):
        bad.append(f"depth bits differ on {int((depth[ok].view(np.uint32) != ref['depth'][ok].view(np.uint32)).sum())} robust pixels")
    d = np.abs(rgba[..., :3].astype(np.int32) - ref['rgb'].astype(np.int32))[ok]
    if d.size and d.max() > 1:
        bad.append(f'rgb off by up to {int(d.max())} levels on robust pixels')
    fr = ref['fragile']
    if not np.all((ids[fr] == ref['id'][fr]) | (ids[fr] == ref['id2'][fr])):
        bad.append('a fragile pixel shows neither of its two nearest ids')
    return bad
