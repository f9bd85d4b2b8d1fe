"""The liquid surface of the renderer's contract (include/fluidengine_ext.h, "Liquids in that picture") restated in numpy, fp64, operation for
operation in the order of fluidlab_amd/csrc/fe_surface.h, on top of tests/render_ref.py (the spheres) and tests/render_scene_ref.py (volumes
and smoke cells).  A helper, not a test; written from the header's text.  Vectorised over pixels, with plain loops over the spheres and over
the window offsets of the smoothing.

render_surface() returns the finished picture (rgb, depth, id), the layer's own images (liq_id, z_raw, z_smooth, thick_words, thickness) and a
`fragile` mask: the rule of render_ref (the two nearest fragments of different spheres within 4 fp32 ulps, or coverage decided by the last
bits) applied to the opaque layer and to the liquid layer, the scene rule of render_scene_ref, and every pixel within smooth_radius_px *
smooth_iters of a fragile pixel of the liquid layer -- a depth that could differ there reaches that far through the passes."""
import numpy as np

import render_ref as RR
import render_scene_ref as RS

BG = RR.BG
FIX = 4294967296.0


def params(radius_scale=1.5, smooth_iters=2, smooth_radius_px=5, range=0.05, absorb=40.0, alpha_min=0.25, specular=0.3, shininess_log2=5):
    """a plain dict with the fields of FeSurfaceParams"""
    return dict(radius_scale=float(radius_scale), smooth_iters=int(smooth_iters), smooth_radius_px=int(smooth_radius_px), range=float(range),
                absorb=float(absorb), alpha_min=float(alpha_min), specular=float(specular), shininess_log2=int(shininess_log2))


def params_of(p):
    """the same dict from a FeSurfaceParams"""
    return params(p.radius_scale, p.smooth_iters, p.smooth_radius_px, p.range, p.absorb, p.alpha_min, p.specular, p.shininess_log2)


def liquid_layer(cam, x, ids, Rs, opaque_depth):
    """step 2: per pixel the smallest word of the liquid spheres' fragments in front of opaque_depth, the summed thickness words, and the
    fragile pixels of the layer.  Returns (key uint64 [H, W], words uint64 [H, W], fragile bool [H, W])."""
    W, H = cam['width'], cam['height']
    x = np.asarray(x, np.float32).reshape(-1, 3)
    key1 = np.full((H, W), BG, np.uint64)
    key2 = np.full((H, W), BG, np.uint64)
    who = np.full((H, W), -1, np.int64)
    who2 = np.full((H, W), -1, np.int64)
    words = np.zeros((H, W), np.uint64)
    fragile = np.zeros((H, W), bool)
    for k in range(len(x)):
        sp = RR.project(cam, x[k], Rs)
        if sp is None or sp['i1'] < sp['i0'] or sp['j1'] < sp['j0']:
            continue
        jj, ii, cov, u, v, nz, depth, s_raw = RR.fragments(sp)
        fragile[jj, ii] |= np.abs(s_raw - 1.0) <= 1e-9
        cov = cov & (depth < opaque_depth[jj, ii])
        key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(int(ids[k]))
        jc, ic, kc = jj[cov], ii[cov], key[cov]
        words[jc, ic] += np.rint((2.0 * sp['R'] * nz[cov]) * FIX).astype(np.uint64)
        old1 = key1[jc, ic]
        better = kc < old1
        cand2 = np.where(better, old1, kc)
        cand2_who = np.where(better, who[jc, ic], k)
        second = cand2 < key2[jc, ic]
        key2[jc[second], ic[second]] = cand2[second]
        who2[jc[second], ic[second]] = cand2_who[second]
        key1[jc[better], ic[better]] = kc[better]
        who[jc[better], ic[better]] = k
    has1, has2 = key1 != BG, key2 != BG
    bits1 = (key1 >> np.uint64(32)).astype(np.int64)
    bits2 = (key2 >> np.uint64(32)).astype(np.int64)
    w1, w2 = np.maximum(who, 0), np.maximum(who2, 0)
    twins = has2 & np.all(x[w1].view(np.uint32) == x[w2].view(np.uint32), axis=-1) if len(x) else np.zeros((H, W), bool)
    fragile |= has1 & has2 & ~twins & ((bits2 - bits1) <= 4)
    return key1, words, fragile


def _shift(z, di, dj):
    """z at (i + di, j + dj), +inf outside the image"""
    H, W = z.shape
    out = np.full((H, W), np.inf, z.dtype)
    j0, j1 = max(0, -dj), min(H, H - dj)
    i0, i1 = max(0, -di), min(W, W - di)
    if j0 < j1 and i0 < i1:
        out[j0:j1, i0:i1] = z[j0 + dj:j1 + dj, i0 + di:i1 + di]
    return out


def smooth(z, r, rng):
    """step 3, one pass over a float32 depth image with +inf on pixels without liquid"""
    z = np.asarray(z, np.float32)
    liquid = np.isfinite(z)
    zp = np.where(liquid, z, 0.0).astype(np.float64)
    num = np.zeros(z.shape)
    den = np.zeros(z.shape)
    rr = float((r + 1) * (r + 1))
    for dj in range(-r, r + 1):
        for di in range(-r, r + 1):
            s2 = float(di * di + dj * dj) / rr
            if s2 >= 1.0:
                continue
            zq32 = _shift(z, di, dj)
            ok = liquid & np.isfinite(zq32)
            zq = np.where(ok, zq32, 0.0).astype(np.float64)
            dz = (zq - zp) / rng
            dz2 = dz * dz
            ok &= ~(dz2 >= 1.0)
            a, b = 1.0 - s2, 1.0 - dz2
            w = (a * a) * (b * b)
            num = np.where(ok, num + w * zq, num)
            den = np.where(ok, den + w, den)
    out = np.full(z.shape, np.inf, np.float32)
    out[liquid] = (num[liquid] / den[liquid]).astype(np.float32)
    return out


def rays(cam):
    """d[3][H + 2][W + 2] of the pixels i = -1 .. W, j = -1 .. H (index + 1)"""
    W, H = cam['width'], cam['height']
    ii, jj = np.meshgrid(np.arange(-1, W + 1, dtype=np.float64), np.arange(-1, H + 1, dtype=np.float64))
    a = ((ii + 0.5) - 0.5 * float(W)) / cam['focal']
    b = ((jj + 0.5) - 0.5 * float(H)) / cam['focal']
    return [(float(cam['fwd'][c]) + a * float(cam['right'][c])) - b * float(cam['up'][c]) for c in range(3)]


def _tangent(cam, z, d, zm, zp, dm, dp, rng):
    with np.errstate(invalid='ignore'):
        am = np.where(np.isfinite(zm), np.abs(np.where(np.isfinite(zm), zm, 0.0).astype(np.float64) - z), -1.0)
        ap = np.where(np.isfinite(zp), np.abs(np.where(np.isfinite(zp), zp, 0.0).astype(np.float64) - z), -1.0)
    am = np.where((am >= 0.0) & (am < rng), am, -1.0)
    ap = np.where((ap >= 0.0) & (ap < rng), ap, -1.0)
    use_p = (ap >= 0.0) & ((am < 0.0) | (ap <= am))
    use_m = ~use_p & (am >= 0.0)
    zn = np.where(use_p, np.where(use_p, zp, 0.0).astype(np.float64), np.where(use_m, np.where(use_m, zm, 0.0).astype(np.float64), z))
    dn = [np.where(use_m, dm[c], dp[c]) for c in range(3)]
    return [(float(cam['pos'][c]) + zn * dn[c]) - (float(cam['pos'][c]) + z * d[c]) for c in range(3)]


def alpha_of(P, thickness):
    """the opacity of a thickness (world length)"""
    at = P['absorb'] * np.asarray(thickness, np.float64)
    return P['alpha_min'] + ((1.0 - P['alpha_min']) * at) / (1.0 + at)


def shade(cam, lights, P, z_smooth, liquid, base, words, behind):
    """step 4 on the pixels `liquid`: base uint8 [H, W, 3] (the colour of the layer's winner), behind uint8 [H, W, 3].  Returns the raw channel
    values [n, 3] before the byte rule."""
    W, H = cam['width'], cam['height']
    D = rays(cam)
    jj, ii = np.nonzero(liquid)
    pad = np.full((H + 2, W + 2), np.inf, np.float32)
    pad[1:-1, 1:-1] = z_smooth
    z = pad[jj + 1, ii + 1].astype(np.float64)
    d = [D[c][jj + 1, ii + 1] for c in range(3)]
    rng = P['range']
    tx = _tangent(cam, z, d, pad[jj + 1, ii], pad[jj + 1, ii + 2], [D[c][jj + 1, ii] for c in range(3)], [D[c][jj + 1, ii + 2] for c in range(3)], rng)
    ty = _tangent(cam, z, d, pad[jj, ii + 1], pad[jj + 2, ii + 1], [D[c][jj, ii + 1] for c in range(3)], [D[c][jj + 2, ii + 1] for c in range(3)], rng)
    n = [ty[1] * tx[2] - ty[2] * tx[1], ty[2] * tx[0] - ty[0] * tx[2], ty[0] * tx[1] - ty[1] * tx[0]]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = (ln > 0.0) & (ln < 1e300)
        n = [np.where(ok, n[c] / np.where(ok, ln, 1.0), 0.0 - float(cam['fwd'][c])) for c in range(3)]
    flip = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] > 0.0
    n = [np.where(flip, 0.0 - n[c], n[c]) for c in range(3)]
    dl = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    Pw = [float(cam['pos'][c]) + z * d[c] for c in range(3)]
    diff = [np.full(len(jj), float(lights['ambient'][c])) for c in range(3)]
    spec = [np.zeros(len(jj)) for c in range(3)]
    for k in range(len(lights['pos'])):
        l = [float(lights['pos'][k][c]) - Pw[c] for c in range(3)]
        ll = np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])
        lit = ll > 0.0
        l = [l[c] / np.where(lit, ll, 1.0) for c in range(3)]
        ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]
        okd = lit & (ndl > 0.0)
        for c in range(3):
            diff[c] = np.where(okd, diff[c] + float(lights['color'][k][c]) * ndl, diff[c])
        hv = [l[c] - d[c] / dl for c in range(3)]
        hl = np.sqrt((hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2])
        oks = lit & (hl > 0.0)
        s = ((n[0] * hv[0] + n[1] * hv[1]) + n[2] * hv[2]) / np.where(oks, hl, 1.0)
        oks &= s > 0.0
        s = np.where(oks, s, 0.0)
        for _ in range(P['shininess_log2']):
            s = s * s
        for c in range(3):
            spec[c] = np.where(oks, spec[c] + float(lights['color'][k][c]) * s, spec[c])
    t = words[jj, ii].astype(np.float64) / FIX
    alpha = alpha_of(P, t)
    raw = []
    for c in range(3):
        lit_c = (base[jj, ii, c].astype(np.float64) / 255.0) * diff[c] + P['specular'] * spec[c]
        raw.append(lit_c * alpha + (behind[jj, ii, c].astype(np.float64) / 255.0) * (1.0 - alpha))
    return np.stack(raw, axis=1)


def dilate(mask, k):
    """every pixel within k (in both image directions) of a pixel of mask"""
    out = mask.copy()
    H, W = mask.shape
    jj, ii = np.nonzero(mask)
    for j, i in zip(jj, ii):
        out[max(0, j - k):min(H, j + k + 1), max(0, i - k):min(W, i + k + 1)] = True
    return out


def render_surface(cam, lights, N, x, ids, radius, rgba, liquid, P, volumes=(), smoke=None, march_step=0.5, bisect_iters=10):
    """x float32 [n, 3], ids int [n], radius fp64 [n] or a scalar, rgba uint8 [n, 4]: the spheres to draw other than smoke cells (used particles
    and point sets with their ids, as render_scene_ref.render_scene takes them); liquid bool [n]: which of them are the liquid (drawn with
    radius_scale * radius); P: params().  volumes, smoke, march_step, bisect_iters: render_scene_ref.render_scene's.
    Returns dict(rgb, depth, id, liq_id, z_raw, z_smooth, thick_words, thickness, liquid, covered, fragile, opaque)."""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64).reshape(-1)
    radius = np.broadcast_to(np.asarray(radius, np.float64), (len(x),))
    rgba = np.asarray(rgba, np.uint8).reshape(-1, 4)
    m = np.asarray(liquid, bool).reshape(-1)
    W, H = cam['width'], cam['height']
    op = RS.render_scene(cam, lights, N, x[~m], ids[~m], radius[~m], rgba[~m], volumes, smoke, march_step, bisect_iters)
    fragile = op['fragile'].copy()
    if (~m).any():
        fragile |= RR.render(cam, lights, x[~m], ids[~m], radius[~m], rgba[~m])['fragile']
    out = dict(rgb=op['rgb'].copy(), depth=op['depth'].copy(), id=op['id'].copy(), opaque=op)
    if not m.any():
        inf = np.full((H, W), np.inf, np.float32)
        out.update(liq_id=np.full((H, W), -1, np.int32), z_raw=inf, z_smooth=inf.copy(), thick_words=np.zeros((H, W), np.uint64), thickness=np.zeros((H, W)),
                   liquid=np.zeros((H, W), bool), covered=op['covered'].copy(), fragile=fragile)
        return out
    Rl = np.unique(radius[m])
    assert len(Rl) == 1, 'the liquid particles share one radius'
    key, words, fl = liquid_layer(cam, x[m], ids[m], P['radius_scale'] * float(Rl[0]), op['depth'])
    liq = key != BG
    z_raw = np.where(liq, (key >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf)).astype(np.float32)
    liq_id = np.where(liq, (key & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    z = z_raw
    for _ in range(P['smooth_iters']):
        z = smooth(z, P['smooth_radius_px'], P['range'])
    col_of = np.zeros((int(ids.max()) + 1, 4), np.uint8)
    col_of[ids] = rgba
    base = col_of[np.maximum(liq_id, 0)][..., :3]
    if liq.any():
        raw = shade(cam, lights, P, z, liq, base, words, op['rgb'])
        out['rgb'][liq] = RR.byte(raw)
    out['depth'][liq] = z[liq]
    out['id'][liq] = liq_id[liq]
    fragile |= dilate(fl, P['smooth_radius_px'] * P['smooth_iters'])
    out.update(liq_id=liq_id, z_raw=z_raw, z_smooth=z, thick_words=words, thickness=words.astype(np.float64) / FIX, liquid=liq,
               covered=op['covered'] | liq, fragile=fragile)
    return out


def compare(ref, rgba, depth, ids, z_raw=None, z_smooth=None, thickness=None, max_fragile=0.005):
    """the rule of the GPU tests: id, depth, and the layer's images bit for bit; RGB within one level outside `fragile`; fragile at most 0.5 % of
    the covered pixels.  Returns a list of complaints (empty: equal)."""
    bad = []

    def bits(a):
        a = np.ascontiguousarray(a)
        return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
    for name, got, want in (('id', ids, ref['id']), ('depth', depth, ref['depth']), ('z_raw', z_raw, ref['z_raw']), ('z_smooth', z_smooth, ref['z_smooth']),
                            ('thickness', thickness, ref['thickness'])):
        if got is None:
            continue
        got = np.asarray(got, want.dtype)
        same = got == want if want.dtype.kind == 'i' else bits(got) == bits(want)
        if not same.all():
            bad.append(f'{name} differs on {int((~same).sum())} pixels')
    ok = ~ref['fragile']
    d = np.abs(rgba[..., :3].astype(np.int32) - ref['rgb'].astype(np.int32))[ok]
    if d.size and d.max() > 1:
        bad.append(f'rgb off by up to {int(d.max())} levels on {int((d.max(axis=-1) > 1).sum())} robust pixels')
    nf, nc = int(ref['fragile'].sum()), int(ref['covered'].sum())
    if nf > max_fragile * max(nc, 1):
        bad.append(f'{nf} fragile pixels of {nc} covered')
    return bad
