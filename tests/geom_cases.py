"""Inputs, references and library loading for the per-function tests of the geometry and contact half of fluidlab_amd/csrc/fe_math.h
(tests/test_csrc_geom_cases.py on the CPU, tests/test_csrc_geom_hip.py on the GPU).  tests/csrc/geom_device_test.hip wraps the SDF sampling, the
contact law, the static and the moving collider, the quaternion helpers, the boundaries and the stencil in thin kernels and in CPU entries of the
same lane functions; this module builds it (device library: the engine's flags; fp64 library: host only, with the `classify` entry), generates the
seeded cases and holds the references that do not come from the header: oracle/mpm_numpy.py and central differences of the fp64 value functions.

Every input is a float32 value widened to float64, so the fp32 and the fp64 builds start from the same words.  A case of the moving collider is
20 numbers (p0[3] q0[4] p1[3] q1[4] pos[3] mv[3]) and a (friction, softness) pair.  The generators enforce their margins BY REJECTION, from the
fp64 `classify` entry: every case they return is asserted by the tests, nothing is filtered afterwards."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import math_cases as M                                        # noqa: E402  (hipcc())
import mpm_numpy as NP                                        # noqa: E402
import scenarios as S                                         # noqa: E402

SRC = os.path.join(ROOT, 'tests', 'csrc', 'geom_device_test.hip')
HEADER = os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_math.h')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')

f32 = np.float32
DT = float(f32(2e-4))
EPS = 1e-12                                                   # FE_EPS
ENTRIES = ('sdf', 'contact_law', 'static_collide', 'dynamic_collide', 'move_quat', 'quat', 'boundary', 'stencil', 'classify')
N_IN, N_OUT, N_IOUT = 4, 4, 2
P0, Q0, P1, Q1, POS, MV = slice(0, 3), slice(3, 7), slice(7, 10), slice(10, 14), slice(14, 17), slice(17, 20)
BLOCKS20 = dict(p0=P0, q0=Q0, p1=P1, q1=Q1, pos=POS, mv=MV)
# columns of the classify entry
C_SD, C_PV, C_PVP, C_PVM, C_G, C_NC, C_VTN, C_T, C_INFL, C_N, C_CV = 0, slice(1, 4), slice(4, 7), slice(7, 10), 10, 11, 12, 13, 14, slice(15, 18), slice(18, 21)


def w32(a):
    """float32 values, widened: what every build reads"""
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(f32).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------------------
# libraries
# ------------------------------------------------------------------------------------------------------------------------------------
def _compile(lib, flags):
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        os.makedirs(OUT, exist_ok=True)
        tmp = f'{lib}.{os.getpid()}.tmp'
        subprocess.check_call([M.hipcc()] + flags + ['-o', tmp, SRC])
        os.replace(tmp, lib)
    return lib


def build_device_lib():
    """gfx950 kernels + launcher + the fp32 CPU evaluation, with the flags the engine is built with."""
    import __graft_entry__ as entry
    return _compile(os.path.join(OUT, 'libgeom_device_test.so'), list(entry.HIPCC_FLAGS))


def build_f64_lib():
    """The header in double on the host: the reference of every value and Jacobian (held against numpy and finite differences on the CPU)."""
    return _compile(os.path.join(OUT, 'libgeom_device_test_f64.so'),
                    ['--offload-host-only', '-O2', '-std=c++17', '-shared', '-fPIC', '-DFE_T=double', '-DGDT_HOST_ONLY', '-x', 'hip'])


CUBE = dict(type='cube', lower=(0.1, 0.1, 0.1), upper=(0.9, 0.9, 0.9), restitution=0.0)


class GeomLib:
    """ctypes face of one build of geom_device_test.hip: run(entry, inputs, ..., device=True) launches the kernel, device=False the CPU evaluation."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        nb = self.lib.gdt_real_bytes()
        self.real = {4: np.float32, 8: np.float64}[nb]
        creal = {4: ctypes.c_float, 8: ctypes.c_double}[nb]
        self.has_device = bool(self.lib.gdt_has_device())
        assert self.lib.gdt_entries() == len(ENTRIES)

        class BoundaryP(ctypes.Structure):
            _fields_ = [('type', ctypes.c_int), ('lower', creal * 3), ('upper', creal * 3), ('cx', creal), ('cz', creal), ('radius', creal),
                        ('restitution', creal), ('lock_dims', ctypes.c_int)]

        class Params(ctypes.Structure):
            _fields_ = [('res', ctypes.c_int), ('vox', ctypes.c_void_p), ('T', creal * 12), ('Rinv', creal * 9), ('bnd', BoundaryP),
                        ('dt', creal), ('inv_dx', creal), ('n_grid', ctypes.c_int)]
        self.Params = Params
        self.widths = {}
        for e, name in enumerate(ENTRIES):
            w = (ctypes.c_int * (N_IN + N_OUT + N_IOUT))()
            assert self.lib.gdt_widths(e, w) == 0
            self.widths[name] = list(w)
        self.lib.gdt_run.restype = ctypes.c_int
        self.lib.gdt_run.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4

    def params(self, collider=None, bnd=None, dt=DT, inv_dx=16.0, n_grid=16, rinv=None):
        """-> (Params, the arrays it points into).  The collider's T and Rinv are float32 values unless `rinv` hands over another inverse."""
        p, keep = self.Params(), []
        if collider is not None:
            vox = np.ascontiguousarray(collider['vox'], dtype=self.real).reshape(-1)
            assert vox.size == collider['res'] ** 3
            keep.append(vox)
            p.res, p.vox = collider['res'], vox.ctypes.data
            p.T[:] = [float(v) for v in np.asarray(collider['T'])[:3].reshape(-1)]
            p.Rinv[:] = [float(v) for v in np.asarray(collider['Rinv'] if rinv is None else rinv).reshape(-1)]
        b = dict(CUBE, **(bnd or {}))
        if b['type'] == 'cube':
            p.bnd.type, lo, up, c, r = 0, b['lower'], b['upper'], (0.0, 0.0), 0.0
        else:                                             # boundaries.py's cylinder: x and z clamp to [0, 1], y to y_range
            p.bnd.type, c, r = 1, b['xz_center'], b['xz_radius']
            lo, up = (0.0, b['y_range'][0], 0.0), (1.0, b['y_range'][1], 1.0)
        p.bnd.lower[:], p.bnd.upper[:] = [float(v) for v in lo], [float(v) for v in up]
        p.bnd.cx, p.bnd.cz, p.bnd.radius, p.bnd.restitution = float(c[0]), float(c[1]), float(r), float(b.get('restitution', 0.0))
        p.bnd.lock_dims = sum(1 << d for d in b.get('lock_dims', ()))
        p.dt, p.inv_dx, p.n_grid = dt, inv_dx, n_grid
        return p, keep

    def run(self, entry, ins, device=False, **prm):
        """-> rc, [real outputs], [int outputs]; each (n, width)"""
        w = self.widths[entry]
        n = len(ins[0])
        p, keep = self.params(**prm)
        cin = [np.ascontiguousarray(a, dtype=self.real).reshape(n, wi) for a, wi in zip(ins, [x for x in w[:N_IN] if x])]
        assert len(cin) == sum(1 for x in w[:N_IN] if x), (entry, len(ins))
        outs = [np.full((n, wo), np.nan, self.real) for wo in w[N_IN:N_IN + N_OUT] if wo]
        iouts = [np.full((n, wo), -77, np.int32) for wo in w[N_IN + N_OUT:] if wo]

        def ptrs(arrs, slots):
            a = (ctypes.c_void_p * slots)()
            for j, x in enumerate(arrs):
                a[j] = x.ctypes.data
            return a
        pi, po, pio = ptrs(cin, N_IN), ptrs(outs, N_OUT), ptrs(iouts, N_IOUT)
        rc = self.lib.gdt_run(ENTRIES.index(entry), 1 if device else 0, n, ctypes.addressof(pi), ctypes.addressof(po), ctypes.addressof(pio),
                              ctypes.addressof(p))
        del keep
        return rc, outs, iouts


@functools.lru_cache(None)
def device_lib():
    alt = os.environ.get('FE_TEST_GEOM_LIB')              # A/B builds of the header (a mutated fe_math.h): tests only
    return GeomLib(os.path.abspath(alt) if alt else build_device_lib())


@functools.lru_cache(None)
def f64_lib():
    alt = os.environ.get('FE_TEST_GEOM_LIB_F64')          # the same for the fp64 build (a mutation the CPU tests are to catch)
    return GeomLib(os.path.abspath(alt) if alt else build_f64_lib())


# ------------------------------------------------------------------------------------------------------------------------------------
# colliders
# ------------------------------------------------------------------------------------------------------------------------------------
def _collider(name, vox, T, lo, hi, radius, scale=(1.0, 1.0, 1.0)):
    """lo, hi: the solid's bounding box in mesh coordinates; `scale` stretches the mesh into the effector's frame (T gets its inverse)."""
    T = np.array(T, np.float64)
    T[:3, :3] = T[:3, :3] @ np.diag(1.0 / np.asarray(scale))
    T = w32(T)
    res = vox.shape[0]
    c = dict(name=name, vox=w32(vox), res=res, T=T, Rinv=w32(np.linalg.inv(T[:3, :3])), Rinv_exact=np.linalg.inv(T[:3, :3]), lo=np.asarray(lo, np.float64),
             hi=np.asarray(hi, np.float64), radius=radius, scale=np.asarray(scale, np.float64), nominal=2 * radius / (res - 1))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(None)
def colliders():
    """thin: the plate of stirrer_mini; thick; sphere: offset_sphere_sdf_mesh; odd: res = 29, the mid-planes lie on grid points; scaled: the plate
    under a non-uniform mesh scale (0.3, 0.4, 0.3) / 0.4, so that Rinv is not a multiple of the identity."""
    out = {}
    for name, half, res, scale in (('thin', (0.12, 0.05, 0.08), 28, (1, 1, 1)), ('thick', (0.12, 0.10, 0.11), 28, (1, 1, 1)),
                                   ('odd', (0.12, 0.05, 0.08), 29, (1, 1, 1)), ('scaled', (0.12, 0.05, 0.08), 28, (0.75, 1.0, 0.75))):
        vox, T = S.box_sdf_mesh(half=half, res=res)
        out[name] = _collider(name, vox, T, -np.asarray(half), np.asarray(half), 0.3, scale)
    vox, T = S.offset_sphere_sdf_mesh()
    c = np.array((0.05, 0.0, 0.03))
    out['sphere'] = _collider('sphere', vox, T, c - 0.1, c + 0.1, 0.3)
    return out


VARIANTS = ((0.5, 0.0), (0.1, 60.0), (2.0, 0.0), (20.0, 0.0))          # (friction, softness); friction > 10 is the sticky road
BRANCHES = ('miss', 'sticky', 'separating', 'slide', 'stick')
MARGIN = 1e-4                                    # sd against its branch edges (mesh units), voxel coordinates against an integer
# nc and t = vtn + nc friction against 0, relative to 1 + |rel|: the host fp32 build's output is within 5.4e-4 (|out| + 1) of fp64 on the well-conditioned
# cases, and nc, t are formed from the same normal as the output -- twice that distance keeps the fp32 selects on the fp64 side.
SELECT_MARGIN = 1e-3
FLAT = 1e-3                                      # |g| below FLAT x nominal: the flat cell layer


# ------------------------------------------------------------------------------------------------------------------------------------
# quaternion helpers (float64, rows)
# ------------------------------------------------------------------------------------------------------------------------------------
def qrot(v, q):
    qv = q[..., 1:]
    uv = np.cross(qv, v)
    return v + 2 * (q[..., :1] * uv + np.cross(qv, uv))


def qconj_n(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0]) / np.linalg.norm(q, axis=-1, keepdims=True)


def qmul_ref(q, r):
    """fe_math.h's quat_mul(q, r) convention (geom.py:8-28), unnormalised"""
    return np.stack([r[..., 0] * q[..., 0] - r[..., 1] * q[..., 1] - r[..., 2] * q[..., 2] - r[..., 3] * q[..., 3],
                     r[..., 0] * q[..., 1] + r[..., 1] * q[..., 0] - r[..., 2] * q[..., 3] + r[..., 3] * q[..., 2],
                     r[..., 0] * q[..., 2] + r[..., 1] * q[..., 3] + r[..., 2] * q[..., 0] - r[..., 3] * q[..., 1],
                     r[..., 0] * q[..., 3] - r[..., 1] * q[..., 2] + r[..., 2] * q[..., 1] + r[..., 3] * q[..., 0]], -1)


def qrot_dq(v, q):
    """d qrot(v, q) / d q -> (n, 3, 4)"""
    qv = q[..., 1:]
    J = np.empty(v.shape[:-1] + (3, 4))
    J[..., 0] = 2 * np.cross(qv, v)
    for k in range(3):
        e = np.zeros(3); e[k] = 1.0
        ev = np.cross(e, v)
        J[..., 1 + k] = 2 * (q[..., :1] * ev + np.cross(e, np.cross(qv, v)) + np.cross(qv, ev))
    return J


def unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# moving-collider cases
# ------------------------------------------------------------------------------------------------------------------------------------
def classify(col, x, fs, dt=DT):
    rc, (c,), (hit,) = f64_lib().run('classify', [x, fs], collider=col, dt=dt)
    assert rc == 0
    return c, hit[:, 0].astype(bool)


def verdict(col, c, hit, fs):
    """-> (sure, flat, branch index) per case from the classify columns: the margins of the issue's table"""
    fr, so = fs[:, 0], fs[:, 1]
    frac = lambda a: np.abs(a - np.rint(a))
    sd = c[:, C_SD]
    edge = np.where(so > 0, np.log(10.0) / np.where(so > 0, so, 1.0), -1.0)            # infl = 0.1 (no edge at softness 0)
    ok = (np.abs(sd) >= MARGIN) & (np.abs(sd - edge) >= MARGIN) & (frac(c[:, C_PV]) >= MARGIN).all(axis=1)
    frictional = hit & (fr <= 10.0)
    rel = 1.0 + np.abs(c[:, C_NC]) + c[:, C_VTN]
    sampled = (frac(c[:, C_PVP]) >= MARGIN).all(axis=1) & (frac(c[:, C_PVM]) >= MARGIN).all(axis=1)
    # a sample that leaves the voxel box reads the constant 1: the step between it and the field is a kink of the same kind as a cell face
    selects = (np.abs(c[:, C_NC]) >= SELECT_MARGIN * rel) & ((c[:, C_NC] >= 0) | (np.abs(c[:, C_T]) >= SELECT_MARGIN * rel)) & \
              ((c[:, C_NC] >= 0) | (c[:, C_VTN] >= 5e-2 * rel))
    flat = frictional & ok & (c[:, C_G] < FLAT * col['nominal'])
    sure = ok & (~frictional | (sampled & (c[:, C_G] >= 0.5 * col['nominal']) & selects))
    branch = np.where(~hit, 0, np.where(fr > 10.0, 1, np.where(c[:, C_NC] >= 0, 2, np.where(c[:, C_T] > 0, 3, 4))))
    return sure, flat, branch


GROUP = 50                                       # cases that share a pose: the numpy reference takes one pose per call


def _draw(col, friction, softness, rng, groups):
    """groups x GROUP candidate cases (float32 values): a moving, turning collider with an unnormalised q0, positions in and around the solid, over
    the whole voxel box and outside it; velocities normal in every direction, and for two in five drawn INTO the surface (stick at low friction)."""
    k = groups * GROUP
    p0 = np.repeat(rng.uniform(0.35, 0.65, (groups, 3)), GROUP, axis=0)
    q0 = np.repeat(unit_quats(rng, groups) * rng.uniform(0.999, 1.001, (groups, 1)), GROUP, axis=0)
    p1 = p0 + np.repeat(DT * rng.normal(0, 0.5, (groups, 3)), GROUP, axis=0)
    w = np.repeat(DT * rng.normal(0, 2.0, (groups, 3)), GROUP, axis=0)
    wn = np.linalg.norm(w, axis=1, keepdims=True)
    a = np.concatenate([np.cos(wn / 2), w / wn * np.sin(wn / 2)], axis=1)
    q1 = qmul_ref(q0, a)
    q1 /= np.linalg.norm(q1, axis=1, keepdims=True)
    where = rng.uniform(size=k)
    near = rng.uniform(col['lo'] - 0.05, col['hi'] + 0.05, (k, 3))
    m = np.where((where < 0.75)[:, None], near, np.where((where < 0.92)[:, None], rng.uniform(-col['radius'], col['radius'], (k, 3)),
                                                          rng.uniform(-1.5 * col['radius'], 1.5 * col['radius'], (k, 3))))
    pm = m * col['scale']                                                              # mesh -> effector frame
    pos = p0 + qrot(pm, q0 / np.linalg.norm(q0, axis=1, keepdims=True))
    x = w32(np.concatenate([p0, q0, p1, q1, pos, rng.normal(0, 1.0, (k, 3))], axis=1))
    fs = np.tile(w32([friction, softness]), (k, 1))
    # velocities into the surface: the normal and the collider's velocity do not depend on mv
    c, _ = classify(col, x, fs)
    n, cv = c[:, C_N], c[:, C_CV]
    tang = np.cross(n, rng.normal(size=(k, 3)))
    tang /= np.maximum(np.linalg.norm(tang, axis=1, keepdims=True), 1e-30)
    depth = rng.uniform(0.2, 2.0, (k, 1))
    into = cv - depth * n + tang * depth * min(friction, 1.0) * rng.uniform(0, 1.5, (k, 1))
    x[:, MV] = np.where((rng.uniform(size=k) < 0.4)[:, None], w32(into), x[:, MV])
    return x, fs, np.repeat(np.arange(groups), GROUP)


@functools.lru_cache(None)
def collide_class(cname, vi, n=2000):
    """One class of moving-collider cases: collider `cname`, VARIANTS[vi].  -> dict x (n, 20), fs (n, 2), group (n,), branch (n,), soft_outside (n,),
    hit (n,), flat: the same for the flat-cell hits met on the way (at most n), drawn / rejected counts.  Read-only."""
    col = colliders()[cname]
    friction, softness = VARIANTS[vi]
    rng = np.random.RandomState(1000 + 17 * sorted(colliders()).index(cname) + vi)
    keep, flat_keep, drawn, rejected, g0 = [], [], 0, 0, 0
    while sum(len(k[0]) for k in keep) < n:
        x, fs, grp = _draw(col, friction, softness, rng, 2 * n // GROUP)
        c, hit = classify(col, x, fs)
        sure, flat, branch = verdict(col, c, hit, fs)
        drawn += len(x); rejected += int((~sure & ~flat).sum())
        assert drawn <= 20 * n, (cname, vi, drawn, rejected)                            # a generator that rejects nearly everything is a bug here
        keep.append((x[sure], fs[sure], grp[sure] + g0, branch[sure], (hit & (c[:, C_SD] > 0))[sure], hit[sure]))
        flat_keep.append((x[flat], fs[flat], grp[flat] + g0, branch[flat]))
        g0 += 2 * n // GROUP
    cat = lambda parts, j, lim: np.ascontiguousarray(np.concatenate([p[j] for p in parts])[:lim])
    out = dict(collider=cname, variant=vi, x=cat(keep, 0, n), fs=cat(keep, 1, n), group=cat(keep, 2, n), branch=cat(keep, 3, n), soft_outside=cat(keep, 4, n),
               hit=cat(keep, 5, n), drawn=drawn, rejected=rejected,
               flat=dict(x=cat(flat_keep, 0, n), fs=cat(flat_keep, 1, n), group=cat(flat_keep, 2, n), branch=cat(flat_keep, 3, n)))
    for v in list(out.values()) + list(out['flat'].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(None)
def tie_collider():
    """A collider whose ties are exact in float32 and in float64 alike: res = 5, the planar field vox[i, j, k] = (j - 2) / 4 (its zero plane is a plane of grid
    points), T = 4 x + 2 (powers of two).  With the identity pose pv = 4 pos + 2 and sd = pos_y hold without rounding for the positions of collide_ties()."""
    vox = np.broadcast_to(((np.arange(5) - 2) / 4.0)[None, :, None], (5, 5, 5)).copy()
    T = np.eye(4) * 4.0
    T[:3, 3], T[3, 3] = 2.0, 1.0
    c = _collider('tie_plane', vox, T, (-0.5, -0.5, -0.5), (0.5, 0.0, 0.5), 0.5)
    return c


def collide_ties():
    """hand-written: sd exactly 0 and one step (2^-20) to either side, at softness 0 and 60 -- at 60, sd = 0 is infl exactly at its cap of 1 and sd < 0 is the
    capped road --, and sd 2e-6 to either side of the soft edge infl = 0.1 (the fp32 exp is good to 1e-7 of infl, 2e-6 in sd moves infl by 1.2e-5); each frictional
    and sticky.  The collider rests in the identity pose (cv = 0 exactly), the velocity points into the plane.  -> x (n, 20), fs (n, 2), expected hit (n,)"""
    step, edge = 2.0 ** -20, np.log(10.0) / 60.0
    rows = [(0.0, 0.0, True), (step, 0.0, False), (-step, 0.0, True), (0.0, 60.0, True), (-step, 60.0, True), (step, 60.0, True),
            (float(f32(edge - 2e-6)), 60.0, True), (float(f32(edge + 2e-6)), 60.0, False)]
    ident = [0.0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    x, fs, hit = [], [], []
    for friction in (0.5, 20.0):
        for y, soft, h in rows:
            x.append(ident + [0.25, y, -0.25] + [0.3, -0.7, 0.2]); fs.append([friction, soft]); hit.append(h)
    x = w32(x)
    assert np.array_equal(x, np.array(x))
    return x, w32(fs), np.array(hit)


CLASS_KEYS = tuple((c, v) for c in ('thin', 'thick', 'sphere', 'odd', 'scaled') for v in range(len(VARIANTS)))


def run_collide(lib, col, x, fs, device=False, dt=DT, rinv=None):
    """-> dict out (n, 3), J (n, 3, 20), hit (n,) bool"""
    rc, (out, J), (hit,) = lib.run('dynamic_collide', [x, fs], device=device, collider=col, dt=dt, rinv=rinv)
    assert rc == 0, rc
    return dict(out=out, J=J.reshape(-1, 3, 20), hit=hit[:, 0])


def collide_errors(o, ref):
    """class maxima: out relative to |out| + 1 per case, J relative to its largest entry per case"""
    eo = np.abs(o['out'].astype(np.float64) - ref['out']).max(axis=1) / (np.abs(ref['out']).max(axis=1) + 1.0)
    ej = np.abs(o['J'].astype(np.float64) - ref['J']).max(axis=(1, 2)) / np.abs(ref['J']).max(axis=(1, 2))
    return dict(out=float(eo.max()), J=float(ej.max()))


def numpy_collide(col, x, fs, group, dt=DT):
    """oracle/mpm_numpy.py's dynamic_collide, one call per pose group"""
    out = np.empty((len(x), 3))
    for g in np.unique(group):
        m = group == g
        i = np.flatnonzero(m)[0]
        dyn = dict(voxels=col['vox'].reshape((col['res'],) * 3), T=np.vstack([col['T'][:3], [0, 0, 0, 1.0]]), friction=fs[i, 0], softness=fs[i, 1],
                   pos0=x[i, P0], quat0=x[i, Q0], pos1=x[i, P1], quat1=x[i, Q1])
        out[m] = NP.dynamic_collide(dyn, x[m][:, POS], x[m][:, MV], dt)
    return out


# Steps of the central differences.  Every pose and position column reaches the output through cv = (...) / dt, so a step h moves the relative velocity by
# h / dt (p0, p1, pos) or by up to 0.5 h / dt (q0, q1): the steps keep that below 1e-5, where the direction vt / |vt| (|vt| >= 0.05 by the margin) is linear to
# (1e-5 / 0.05)^2 = 4e-8; the rounding of cv (1e-16 x 0.5 / dt = 3e-13) over the step stays below 3e-8 of the 1 / dt = 5000 scale of those columns.
FD_STEP = np.concatenate([np.full(3, 2e-9), np.full(4, 1e-8), np.full(3, 2e-9), np.full(4, 1e-8), np.full(3, 2e-9), np.full(3, 1e-6)])


def fd_jacobian(fn, x, steps):
    """central differences of fn: (n, k) -> (n, m), column by column -> (n, m, k)"""
    cols = []
    for c in range(x.shape[1]):
        xp, xm = x.copy(), x.copy()
        xp[:, c] += steps[c]; xm[:, c] -= steps[c]
        cols.append((fn(xp) - fn(xm)) / (xp[:, c] - xm[:, c])[:, None])
    return np.stack(cols, axis=-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# the smaller functions
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def sdf_points(cname, n=4000):
    """voxel coordinates over the whole box of a collider and beyond it (a margin of 1e-4 to every integer for pv and pv +- 1e-2)"""
    col = colliders()[cname]
    rng = np.random.RandomState(77)
    out = np.empty((0, 3))
    while len(out) < n:
        pv = w32(rng.uniform(-2.0, col['res'] + 1.0, (2 * n, 3)))
        frac = lambda a: np.abs(a - np.rint(a))
        ok = np.all([(frac(pv + d) >= MARGIN).all(axis=1) for d in (0.0, 1e-2, -1e-2)], axis=0)
        out = np.concatenate([out, pv[ok]])
    out = out[:n]
    out.setflags(write=False)
    return out


def sdf_edge_points(col):
    """hand-written: a coordinate exactly on an integer, at res - 1, at res - 1 - 1e-2, at 0 and just below it (the other two mid-cell)"""
    r = col['res']
    vals = [5.0, float(r - 1), float(f32(r - 1 - 1e-2)), float(np.nextafter(f32(r - 1), f32(0))), 0.0, float(-np.nextafter(f32(0), f32(1))), -1e-3,
            float(f32(r - 2)), float(f32(1e-2)), float(f32(r - 1 + 1e-2))]
    pts = []
    for v in vals:
        for d in range(3):
            p = [11.37, 14.21, 9.63]
            p[d] = v
            pts.append(p)
    return w32(pts)


def contact_law_cases(n=4000, seed=5):
    """unit normals, relative velocities of every sign of nc, frictions 0, 0.1, 0.5, 2; margins on nc, vtn and t as for the collider"""
    rng = np.random.RandomState(seed)
    N, RV, G, FR = (np.empty((0, k)) for k in (3, 3, 3, 1))
    while len(N) < n:
        nn = rng.normal(size=(2 * n, 3)); nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        nn = w32(nn)
        rv, g, fr = w32(rng.normal(size=(2 * n, 3))), w32(rng.normal(size=(2 * n, 3))), w32(rng.choice([0.0, 0.1, 0.5, 2.0], (2 * n, 1)))
        rv[::3] = w32(-nn[::3] * rng.uniform(0.3, 2, (len(nn[::3]), 1)) + 0.3 * rng.normal(size=nn[::3].shape))          # into the surface
        nc = (rv * nn).sum(1)
        vt = rv - np.minimum(nc, 0)[:, None] * nn
        vtn = np.linalg.norm(vt, axis=1)
        t = vtn + nc * fr[:, 0]
        ok = (np.abs(nc) >= 1e-3) & ((nc >= 0) | ((np.abs(t) >= 1e-3) & (vtn >= 1e-2)))
        N, RV, G, FR = (np.concatenate([a, b[ok]]) for a, b in ((N, nn), (RV, rv), (G, g), (FR, fr)))
    return N[:n], RV[:n], G[:n], FR[:n]


def numpy_contact_law(n, rv, fr):
    """static.py:88-101 on rows, the normal given (oracle/mpm_numpy.py's static_collide from its normal on)"""
    nc = (rv * n).sum(1)
    vt = rv - np.minimum(nc, 0)[:, None] * n
    vtn = np.linalg.norm(vt, axis=1)
    flag = (nc < 0) & (vtn > EPS)
    return vt * np.where(flag, np.maximum(0, vtn + nc * fr) / np.where(vtn > 0, vtn, 1.0), 1.0)[:, None]


CYLINDER = dict(type='cylinder', y_range=(0.2, 0.8), xz_center=(0.5, 0.45), xz_radius=0.3, restitution=0.0)
BOUNDARIES = {
    'cube': dict(CUBE, restitution=0.25),
    'cube_locked': dict(CUBE, lock_dims=(1,)),
    'cube_flat': dict(type='cube', lower=(0.1, 0.62, 0.1), upper=(0.9, 0.62, 0.9), restitution=0.0),          # the y_range = (0.62, 0.62) effector
    'cylinder': dict(CYLINDER, restitution=0.5),
    'cylinder_locked': dict(CYLINDER, lock_dims=(0, 2)),
}


def boundary_f32(b):
    """the boundary with every number rounded to float32 (what the fp32 builds compare with), as python floats"""
    out = dict(b)
    for k in ('lower', 'upper', 'y_range', 'xz_center'):
        if k in out:
            out[k] = tuple(float(f32(v)) for v in out[k])
    for k in ('xz_radius', 'restitution'):
        if k in out:
            out[k] = float(f32(out[k]))
    return out


def boundary_cases(bname, n=3000, seed=21):
    """positions inside, outside and around every face (margin 1e-5 to a face and to the cylinder's wall), velocities of both signs (|v| >= 1e-3)"""
    b = boundary_f32(BOUNDARIES[bname])
    rng = np.random.RandomState(seed)
    X, V = np.empty((0, 3)), np.empty((0, 3))
    while len(X) < n:
        x = w32(rng.uniform(-0.1, 1.1, (2 * n, 3)))
        v = w32(rng.normal(size=(2 * n, 3)))
        if b['type'] == 'cube':
            lo, up = np.array(b['lower']), np.array(b['upper'])
            ok = (np.abs(x - lo) >= 1e-5).all(1) & (np.abs(x - up) >= 1e-5).all(1)
        else:
            nrm = np.sqrt((x[:, 0] - b['xz_center'][0]) ** 2 + (x[:, 2] - b['xz_center'][1]) ** 2 + EPS)
            ok = (np.abs(nrm - b['xz_radius']) >= 1e-5) & (np.abs(x[:, 1] - b['y_range'][0]) >= 1e-5) & (np.abs(x[:, 1] - b['y_range'][1]) >= 1e-5)
            ok &= (np.abs(x[:, [0, 2]]) >= 1e-5).all(1) & (np.abs(x[:, [0, 2]] - 1.0) >= 1e-5).all(1)
        ok &= (np.abs(v) >= 1e-3).all(1)
        X, V = np.concatenate([X, x[ok]]), np.concatenate([V, v[ok]])
    return b, X[:n], V[:n]


def numpy_boundary(b, x, v):
    """-> v', xn, is_out by oracle/mpm_numpy.py (impose_x position by position) and boundaries.py:80-93, 127-134 for is_out"""
    xn = np.array([NP.impose_x(b, p) for p in x])
    if b['type'] == 'cube':
        is_out = ((x > np.array(b['upper'])) | (x < np.array(b['lower']))).any(1)
    else:
        nrm = np.sqrt((x[:, 0] - b['xz_center'][0]) ** 2 + (x[:, 2] - b['xz_center'][1]) ** 2 + EPS)
        is_out = (x[:, 1] > b['y_range'][1]) | (x[:, 1] < b['y_range'][0]) | (nrm > b['xz_radius'])
    return NP.boundary_v(b, x, v), xn, is_out


def stencil_cases(n=4000, n_grid=16, seed=31):
    """positions over the grid and a little beyond it on both sides, x inv_dx - 0.5 at least 1e-4 from an integer"""
    rng = np.random.RandomState(seed)
    X = np.empty((0, 3))
    while len(X) < n:
        x = w32(rng.uniform(-0.2, 1.2, (2 * n, 3)))
        a = x * n_grid - 0.5
        X = np.concatenate([X, x[(np.abs(a - np.rint(a)) >= 1e-4).all(1)]])
    return X[:n]


def stencil_ties(n_grid=16):
    """hand-written, exact in float32 (inv_dx is a power of two): x inv_dx - 0.5 on an integer and one float32 step to either side of it, for
    integers over and around the grid, negative ones included (truncation toward zero)"""
    xs = []
    for k in (-2, -1, 0, 1, 7, n_grid - 3, n_grid - 2, n_grid - 1, n_grid):
        at = f32((k + 0.5) / n_grid)
        xs += [float(np.nextafter(at, f32(-9))), float(at), float(np.nextafter(at, f32(9)))]
    xs = np.array(xs)
    x = np.full((3 * len(xs), 3), 0.53125)
    for d in range(3):
        x[d * len(xs):(d + 1) * len(xs), d] = xs
    return x


STENCIL_WILD = np.array([1e30, -1e30, np.inf, -np.inf, np.nan])


def stencil_reference(x, n_grid, dtype=np.float64):
    """base by truncation toward zero (Taichi's cast) of x inv_dx - 0.5 formed in `dtype` -- inv_dx is a power of two, so the product is exact and a fused
    multiply-add rounds as the two operations do: one float32 step from an integer the fp32 and the fp64 base may differ, each is right --, then fx, w, dw
    and inside in float64"""
    a = (x.astype(dtype) * dtype(n_grid) - dtype(0.5)).astype(np.float64)
    base = np.trunc(a).astype(np.int64)
    fx = x * n_grid - base
    w = np.stack([0.5 * (1.5 - fx) ** 2, 0.75 - (fx - 1.0) ** 2, 0.5 * (fx - 0.5) ** 2], axis=1)          # (n, 3 offsets, 3 dims)
    dw = np.stack([-(1.5 - fx), -2 * (fx - 1.0), fx - 0.5], axis=1)
    inside = ((base >= 0) & (base <= n_grid - 3)).all(1)
    return base, fx, w, dw, inside


def move_quat_cases(n=3000, seed=41):
    """w of a substep's size (|w| ~ 1e-3) and of a whole turn, q of norm 0.999 ... 1.001; plus the hand-written w = 0 and |w| = 1e-7"""
    rng = np.random.RandomState(seed)
    w = rng.normal(size=(n, 3)) * np.where(np.arange(n) % 2 == 0, 1e-3, 1.0)[:, None]
    q = unit_quats(rng, n) * rng.uniform(0.999, 1.001, (n, 1))
    hand_w = np.array([[0, 0, 0], [1e-7, 0, 0], [0, -1e-7, 0], [6e-8, 6e-8, -5e-8]])
    hand = np.concatenate([hand_w, unit_quats(rng, len(hand_w))], axis=1)
    return w32(np.concatenate([w, q], axis=1)), w32(hand)


def numpy_move_quat(wq):
    b = dict(CUBE)
    return np.array([NP.effector_move(b, (0.5, 0.5, 0.5), r[3:], (0, 0, 0), r[:3])[1] for r in wq])
