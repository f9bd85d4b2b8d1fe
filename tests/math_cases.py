"""Inputs, references and library loading for the per-function tests of fluidlab_amd/csrc/fe_math.h (tests/test_csrc_math_cases.py on the CPU,
tests/test_csrc_math_hip.py on the GPU).  tests/csrc/math_device_test.hip wraps the header's cube root, SVD and constitutive model in thin kernels
and in CPU entries of the same lane functions; this module builds it (device library: the engine's flags; fp64 library: host only), generates the
seeded cases and computes the references that do not come from the header: numpy's SVD, determinant and power in float64 on the float32 inputs.
Every case that is generated is asserted: gaps between singular values are enforced by rejection here, nothing is filtered afterwards."""
import ctypes
import functools
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'math_device_test.hip')
HEADER = os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_math.h')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')

f32 = np.float32
UNIT = 6e-8                               # the unit of tests/csrc/math_test.cpp's cube-root check (relative)

# constants of tests/csrc/math_test.cpp, rounded to float32 once: every build (device, host fp32, host fp64, numpy) gets these values
DT = float(f32(2e-4))
LAM = float(f32(277.78))
MASS = float(f32(6.1e-5))
_N = 64
SCALE = float(f32(-2e-4 * (0.5 / _N) ** 2 * 4 * _N * _N))
LIQUID, PLASTO, ELASTIC, RIGID, PLASTO_DEMO = 200, 201, 202, 203, 204          # fe_math.h FE_MAT_*
CLAMP_LO = f32(1.0) - f32(2e-3)           # the header's fp32 clamp edges (1.0f - 2e-3f, 1.0f + 3e-3f)
CLAMP_HI = f32(1.0) + f32(3e-3)
EDGE_MARGIN = 4e-6                        # > 3e-6 x 1.1: the SVD contract's bound on a sigma's error at the largest sigma_0 of the plastic classes


# ------------------------------------------------------------------------------------------------------------------------------------
# libraries
# ------------------------------------------------------------------------------------------------------------------------------------
def hipcc():
    return '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')


def _stale(lib):
    return not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER))


def _compile(lib, flags):
    if _stale(lib):
        os.makedirs(OUT, exist_ok=True)
        tmp = f'{lib}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc()] + flags + ['-o', tmp, SRC])
        os.replace(tmp, lib)
    return lib


def build_device_lib():
    """gfx950 kernels + launchers + the fp32 CPU entries, with the flags the engine is built with."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    return _compile(os.path.join(OUT, 'libmath_device_test.so'), list(entry.HIPCC_FLAGS))


def build_f64_lib():
    """The header in double on the host: the adjoint reference (tests/test_csrc_math.py holds this build against finite differences)."""
    return _compile(os.path.join(OUT, 'libmath_device_test_f64.so'),
                    ['--offload-host-only', '-O2', '-std=c++17', '-shared', '-fPIC', '-DFE_T=double', '-DMDT_HOST_ONLY', '-x', 'hip'])


CONST_OUT = ('affine', 'Fnew', 'J', 'full', 'sig', 'gC', 'gF')


class MathLib:
    """ctypes face of one build of math_device_test.hip.  `suffix` = '' runs the kernels, '_host' the CPU evaluation."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.real = {4: np.float32, 8: np.float64}[self.lib.mdt_real_bytes()]
        self.creal = {4: ctypes.c_float, 8: ctypes.c_double}[self.lib.mdt_real_bytes()]

    def _fn(self, name, argtypes):
        fn = getattr(self.lib, name)
        fn.argtypes, fn.restype = argtypes, ctypes.c_int
        return fn

    def _in(self, a, dtype=None):
        return np.ascontiguousarray(a, dtype=dtype or self.real)

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def cbrt(self, J, suffix=''):
        J = self._in(J)
        n = J.size
        cb, pm = np.empty(n, self.real), np.empty(n, self.real)
        rc = self._fn('mdt_cbrt' + suffix, [ctypes.c_void_p] * 3 + [ctypes.c_int])(self._p(J), self._p(cb), self._p(pm), n)
        return rc, cb, pm

    def svd(self, F, mask=None, suffix=''):
        """-> rc, U, sig, V; rows whose mask is 0 stay NaN."""
        F = self._in(F).reshape(-1, 3, 3)
        n = len(F)
        mask = np.ones(n, np.int32) if mask is None else self._in(mask, np.int32)
        assert mask.shape == (n,)
        U, sig, V = (np.full(s, np.nan, self.real) for s in ((n, 3, 3), (n, 3), (n, 3, 3)))
        rc = self._fn('mdt_svd' + suffix, [ctypes.c_void_p] * 5 + [ctypes.c_int])(self._p(F), self._p(mask), self._p(U), self._p(sig), self._p(V), n)
        return rc, U, sig, V

    def constitutive(self, cs, general=True, suffix=''):
        """cs: dict with C, F, GA, Fg (n,3,3), mu, lam (n,), cls (n,) -> rc, dict of CONST_OUT."""
        n = len(cs['mu'])
        m = {k: self._in(cs[k]).reshape(n, 3, 3) for k in ('C', 'F', 'GA', 'Fg')}
        mu, lam, cls = self._in(cs['mu']), self._in(cs['lam']), self._in(cs['cls'], np.int32)
        assert mu.shape == lam.shape == cls.shape == (n,)
        o = dict(affine=np.empty((n, 3, 3), self.real), Fnew=np.empty((n, 3, 3), self.real), J=np.empty(n, self.real), full=np.empty(n, np.int32),
                 sig=np.empty((n, 3), self.real), gC=np.empty((n, 3, 3), self.real), gF=np.empty((n, 3, 3), self.real))
        fn = self._fn('mdt_constitutive' + suffix, [ctypes.c_int] + [ctypes.c_void_p] * 7 + [self.creal] * 3 + [ctypes.c_void_p] * 7 + [ctypes.c_int])
        rc = fn(1 if general else 0, self._p(m['C']), self._p(m['F']), self._p(mu), self._p(lam), self._p(cls), self._p(m['GA']), self._p(m['Fg']),
                DT, MASS, SCALE, *[self._p(o[k]) for k in CONST_OUT], n)
        return rc, o


@functools.lru_cache(None)
def device_lib():
    alt = os.environ.get('FE_TEST_MATH_LIB')          # A/B builds of the header (a mutated fe_math.h): tests only
    return MathLib(os.path.abspath(alt) if alt else build_device_lib())


@functools.lru_cache(None)
def f64_lib():
    return MathLib(build_f64_lib())


# ------------------------------------------------------------------------------------------------------------------------------------
# generators
# ------------------------------------------------------------------------------------------------------------------------------------
def rotations(rng, n):
    """n proper rotations (float64), uniform: QR of a Gaussian matrix with the signs of R's diagonal moved into Q"""
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q


def _between(rng, s):
    """R1 diag(s) R2^T for fresh rotations R1, R2; s is (n, 3)"""
    n = len(s)
    return np.einsum('nij,nj,nkj->nik', rotations(rng, n), s, rotations(rng, n))


SVD_KINDS = ('fluid', 'generic', 'rank2', 'rank1', 'zero', 'scaled_identity', 'rotation', 'clamp_band', 'two_equal', 'reflection', 'scaled')


def svd_kind(kind, n, rng):
    """n float32 3x3 matrices of one kind.  Entries stay within 1e-3 ... 1e3 of unit scale: svd3's skip thresholds are absolute."""
    if kind == 'fluid':
        F = np.eye(3) + rng.normal(0, 0.02, (n, 3, 3))
    elif kind == 'generic':                           # half have det < 0
        F = rng.normal(size=(n, 3, 3))
    elif kind == 'rank2':                             # third column in the span of the first two (formed in float32, as math_test.cpp does)
        F = f32(rng.normal(size=(n, 3, 3)))
        F[:, :, 2] = F[:, :, 0] * f32(0.5) - F[:, :, 1]
    elif kind == 'rank1':
        a = f32(rng.normal(size=(n, 3, 2)))
        F = a[:, :, None, 0] * a[:, None, :, 1]
    elif kind == 'zero':
        F = np.zeros((n, 3, 3))
    elif kind == 'scaled_identity':
        F = rng.uniform(0.5, 1.5, n)[:, None, None] * np.eye(3)
    elif kind == 'rotation':
        F = rotations(rng, n)
    elif kind == 'clamp_band':                        # the plastic clamp of ICECREAM: sigma within [1 - 2e-3, 1 + 3e-3]
        F = _between(rng, 1.0 + rng.uniform(-2e-3, 3e-3, (n, 3)))
    elif kind == 'two_equal':
        F = _between(rng, np.tile([1.3, 1.3, 0.8], (n, 1)))
    elif kind == 'reflection':
        F = _between(rng, np.tile([1.2, 0.9, -0.7], (n, 1)))
    elif kind == 'scaled':                            # generic, half at 1e-3 and half at 1e3
        F = rng.normal(size=(n, 3, 3)) * np.where(np.arange(n) % 2 == 0, 1e-3, 1e3)[:, None, None]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(F, dtype=f32)


@functools.lru_cache(None)
def svd_cases(n_per_kind=40000, seed=2024):
    """-> (F float32 (K n, 3, 3), kind index (K n,)), the kinds shuffled together so that every wave of 64 holds a mixture.  Read-only."""
    rng = np.random.RandomState(seed)
    F = np.concatenate([svd_kind(k, n_per_kind, rng) for k in SVD_KINDS])
    kind = np.repeat(np.arange(len(SVD_KINDS)), n_per_kind)
    perm = rng.permutation(len(F))
    F, kind = F[perm], kind[perm]
    F.setflags(write=False); kind.setflags(write=False)
    return F, kind


@functools.lru_cache(None)
def svd_reference(n_per_kind=40000, seed=2024):
    """float64 singular values (descending) and determinant of the float32 matrices of svd_cases, by numpy.  Read-only."""
    F, _ = svd_cases(n_per_kind, seed)
    F64 = F.astype(np.float64)
    s, det = np.linalg.svd(F64, compute_uv=False), np.linalg.det(F64)
    s.setflags(write=False); det.setflags(write=False)
    return s, det


def svd_contract(F, U, sig, V, s_ref, det_ref):
    """The contract of tests/csrc/math_test.cpp for float32 results, measured in float64 per matrix.
    -> dict of per-matrix arrays: recon, orth, sigma (errors), det (min of det U, det V), and booleans ordered, nonneg, sign_ok."""
    F, U, sig, V = (np.asarray(a, np.float64) for a in (F, U, sig, V))
    R = np.einsum('nij,nj,nkj->nik', U, sig, V)
    nrm = np.maximum(np.abs(F).max(axis=(1, 2)), 1e-30)
    eye = np.eye(3)
    UtU, VtV = np.einsum('nji,njk->nik', U, U), np.einsum('nji,njk->nik', V, V)
    s0 = np.maximum(s_ref[:, 0], 1e-30)
    a = np.abs(sig)
    return dict(
        recon=np.abs(R - F).max(axis=(1, 2)) / nrm,
        orth=np.maximum(np.abs(UtU - eye).max(axis=(1, 2)), np.abs(VtV - eye).max(axis=(1, 2))),
        sigma=np.abs(a - s_ref).max(axis=1) / s0,
        det=np.minimum(np.linalg.det(U), np.linalg.det(V)),
        ordered=(a[:, 0] >= a[:, 1]) & (a[:, 1] >= a[:, 2]),
        nonneg=(sig[:, 0] >= 0) & (sig[:, 1] >= 0),
        # the sign of sig[2] follows det F, unless sig[2] is zero to working precision (math_test.cpp's exemption: |sig[2]| < 1e-6 |sig[0]|)
        sign_ok=((det_ref < 0) == (sig[:, 2] < 0)) | (a[:, 2] < 1e-6 * a[:, 0]) | (a[:, 0] == 0),
        finite=np.isfinite(U).all(axis=(1, 2)) & np.isfinite(V).all(axis=(1, 2)) & np.isfinite(sig).all(axis=1))


SVD_TOL = dict(recon=3e-6, orth=3e-6, sigma=3e-6, det=0.99)


def assert_svd_contract(c, kind, label):
    """asserts the contract on every matrix and returns the worst figures per kind (for printing)"""
    worst = {}
    for ki, name in enumerate(SVD_KINDS):
        m = kind == ki
        if not m.any():
            continue
        worst[name] = dict(recon=c['recon'][m].max(), orth=c['orth'][m].max(), sigma=c['sigma'][m].max(), det=c['det'][m].min())
        print(f'{label} svd3 {name:16s} n={m.sum():6d} recon {worst[name]["recon"]:.3g} orth {worst[name]["orth"]:.3g} '
              f'sigma {worst[name]["sigma"]:.3g} min det {worst[name]["det"]:.6f}')
    for flag in ('finite', 'ordered', 'nonneg', 'sign_ok'):
        bad = np.flatnonzero(~c[flag])
        assert bad.size == 0, f'{label}: {flag} violated by {bad.size} matrices, first {bad[:5]} (kinds {[SVD_KINDS[k] for k in kind[bad[:5]]]})'
    for name, w in worst.items():
        assert w['recon'] <= SVD_TOL['recon'] and w['orth'] <= SVD_TOL['orth'] and w['sigma'] <= SVD_TOL['sigma'] and w['det'] > SVD_TOL['det'], (label, name, w)
    return worst


def _gapped(rng, n, draw, gap):
    """(n, 3) singular values from draw(k) -> (k, 3), redrawn until neighbouring values (sorted) are at least `gap` apart"""
    out = np.empty((0, 3))
    while len(out) < n:
        s = draw(2 * n)
        d = np.diff(np.sort(s, axis=1), axis=1)
        out = np.concatenate([out, s[(d >= gap).all(axis=1)]])
    return out[:n]


# label -> (material class, mu, how the singular values of F are drawn, smallest gap between neighbours)
CLASSES = {
    'a': (LIQUID, 0.0, lambda rng, k: 1.0 + rng.normal(0, 0.02, (k, 3)), None),           # inviscid liquid: the road without an SVD
    'b': (LIQUID, 200.0, lambda rng, k: rng.uniform(0.6, 1.5, (k, 3)), 0.05),
    'c': (ELASTIC, 416.67, None, 0.05),                                                   # the singular values of (b)
    'd': (ELASTIC, 416.67, lambda rng, k: rng.uniform(0.6, 1.5, (k, 3)), 0.01),
    'e': (PLASTO, 416.67, lambda rng, k: rng.uniform(0.994, 1.007, (k, 3)), 5e-4),        # inside, outside and across the clamp edges
    'f': (PLASTO_DEMO, 160.0, lambda rng, k: rng.uniform(0.9, 1.1, (k, 3)), 0.05),        # the band is 5e-3 wide: at most one sigma inside, the rest clamped
}
_CLASS_SEED = {'a': 11, 'b': 12, 'c': 12, 'd': 14, 'e': 15, 'f': 16}


@functools.lru_cache(None)
def constitutive_class(label, n=2000):
    """One class of the table above as float32 arrays: F = R1 diag(s) R2^T, C ~ N(0, 5), GA and Fg ~ N(0, 1).  Read-only."""
    cls, mu, draw, gap = CLASSES[label]
    rng = np.random.RandomState(_CLASS_SEED[label])
    if label == 'c':
        draw = CLASSES['b'][2]
    s = draw(rng, n) if gap is None else _gapped(rng, n, lambda k: draw(rng, k), gap)
    cs = dict(F=f32(_between(rng, s)), C=f32(rng.normal(0, 5, (n, 3, 3))), GA=f32(rng.normal(size=(n, 3, 3))), Fg=f32(rng.normal(size=(n, 3, 3))),
              mu=np.full(n, mu, f32), lam=np.full(n, LAM, f32), cls=np.full(n, cls, np.int32), s=s)
    if cls in (PLASTO, PLASTO_DEMO):
        # The clamp's adjoint jumps at the edges: a sigma of F_tmp = (I + dt C) F closer to an edge than the fp32 SVD resolves it is passed by one
        # rounding and blocked by another, and gC, gF then differ by O(1) with nothing wrong.  The contract bounds svd3's sigma error by 3e-6 sigma_0,
        # so C is redrawn until no sigma lies within EDGE_MARGIN of an edge; sigma exactly ON an edge is the business of tie_cases().
        while True:
            sig = np.linalg.svd((np.eye(3) + DT * cs['C'].astype(np.float64)) @ cs['F'].astype(np.float64), compute_uv=False)
            near = (np.minimum(np.abs(sig - (1.0 - 2e-3)), np.abs(sig - (1.0 + 3e-3))) < EDGE_MARGIN).any(axis=1)
            if not near.any():
                break
            cs['C'][near] = f32(rng.normal(0, 5, (int(near.sum()), 3, 3)))
    for v in cs.values():
        v.setflags(write=False)
    return cs


def block_err(a, b):
    """max |a - b| / max |b| per 3x3 block (or per row of any trailing shape) -> (n,)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ax = tuple(range(1, a.ndim))
    if not ax:
        return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return np.abs(a - b).max(axis=ax) / np.maximum(np.abs(b).max(axis=ax), 1e-300)


BLOCKS = ('affine', 'Fnew', 'gC', 'gF')


def class_errors(o, ref):
    """class maxima of the per-block error of `o` against `ref` for BLOCKS and J"""
    return {k: float(block_err(o[k], ref[k]).max()) for k in BLOCKS + ('J',)}


def numpy_forward(cs):
    """affine, J, |sig| and F_new of constitutive_eval_t in float64 by numpy, from the float32 inputs (F_new: liquid and elastic classes only)"""
    C, F = cs['C'].astype(np.float64), cs['F'].astype(np.float64)
    mu, lam = cs['mu'].astype(np.float64), cs['lam'].astype(np.float64)
    Ft = (np.eye(3) + DT * C) @ F
    U, s, Vt = np.linalg.svd(Ft)
    J = np.linalg.det(Ft)
    assert (J > 0).all()                              # no class here inverts a particle: U V^T of numpy is the proper rotation
    R = U @ Vt
    stress = 2.0 * mu[:, None, None] * ((Ft - R) @ np.swapaxes(Ft, 1, 2)) + (lam * J * (J - 1.0))[:, None, None] * np.eye(3)
    out = dict(affine=SCALE * stress + MASS * C, J=J, sig=s)
    # affine is a sum whose first two terms cancel for F_tmp near a rotation (class (e): |F_tmp - R| = 5e-3, the terms 700 times the sum): two fp64
    # evaluations differ by eps times the largest term, not eps times the sum.  That is the scale the comparison with the header is relative to.
    FtFt = np.abs(Ft @ np.swapaxes(Ft, 1, 2)).max(axis=(1, 2))
    out['affine_scale'] = np.maximum.reduce([np.abs(out['affine']).max(axis=(1, 2)), abs(SCALE) * 2.0 * mu * FtFt,
                                             np.abs(SCALE * lam * J * (J - 1.0)), MASS * np.abs(C).max(axis=(1, 2))])
    cls = cs['cls'][0]
    if cls == LIQUID:
        out['Fnew'] = np.power(J, 1.0 / 3.0)[:, None, None] * np.eye(3)
    elif cls == ELASTIC:
        out['Fnew'] = Ft
    return out


# ---- hand-made ties of the plastic clamp -------------------------------------------------------------------------------------------
def _signed_perms():
    """the 24 proper signed permutation matrices"""
    import itertools
    out = []
    for p in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            P = np.zeros((3, 3))
            for col, (row, sg) in enumerate(zip(p, signs)):
                P[row, col] = sg
            if np.linalg.det(P) > 0:
                out.append(P)
    return out


@functools.lru_cache(None)
def tie_cases():
    """Plasto-elastic cases F = P1 diag(s) P2^T (P1, P2 proper signed permutations: the Jacobi SVD rotates nothing and returns the entries of s exactly)
    with C = 0, GA = 0 and Fg = u_d v_d^T for the slot d whose sigma sits at, one float32 step below, or one above a clamp edge.
    Then gF = pass_d u_d v_d^T, so <gF, u_d v_d^T> is the pass decision (1 or 0) of slot d.
    The fp32 builds compare with the header's fp32 edges, the fp64 build with 1 - 2e-3 and 1 + 3e-3 in double, which are other numbers: a case `at` the
    edge gives each build its own edge, so that both decide a real tie; the neighbours are the same float32 values in every build.
    -> dict: cs32, cs64 (inputs), proj (n,3,3) the matrix to project gF on, where (n,) in {'below', 'at', 'above'}, edge (n,) in {'lo', 'hi'},
       expect (n,) the decision of Taichi's max/min tie rule pass = sd > lo and max(sd, lo) < hi."""
    rng = np.random.RandomState(5)
    perms = _signed_perms()
    others = [(0.9, 1.1), (1.0, 1.001), (0.9995, 1.0025), (0.7, 0.8), (1.2, 1.4), (1.0015, 0.95)]       # inside and outside the band, distinct
    others = [tuple(float(f32(v)) for v in o) for o in others]
    F32, F64, proj, where, edge, expect = [], [], [], [], [], []
    for ename, e32, e64 in (('lo', CLAMP_LO, 1.0 - 2e-3), ('hi', CLAMP_HI, 1.0 + 3e-3)):
        for wname, v32, v64 in (('below', np.nextafter(e32, f32(0)), None), ('at', e32, e64), ('above', np.nextafter(e32, f32(2)), None)):
            v64 = float(v32) if v64 is None else v64
            for oth in others:
                for slot in range(3):
                    P1, P2 = perms[rng.randint(len(perms))], perms[rng.randint(len(perms))]
                    s32 = np.insert(np.array(oth, np.float64), slot, float(v32))
                    s64 = np.insert(np.array(oth, np.float64), slot, v64)
                    F32.append(P1 @ np.diag(s32) @ P2.T); F64.append(P1 @ np.diag(s64) @ P2.T)
                    proj.append(np.outer(P1[:, slot], P2[:, slot]))
                    where.append(wname); edge.append(ename)
                    expect.append(bool(v32 > CLAMP_LO and max(v32, CLAMP_LO) < CLAMP_HI))
    n = len(F32)
    proj = np.array(proj)
    base = dict(C=np.zeros((n, 3, 3)), GA=np.zeros((n, 3, 3)), Fg=proj, mu=np.full(n, 416.67, f32), lam=np.full(n, LAM, f32),
                cls=np.full(n, PLASTO, np.int32))
    cs32 = dict(base, F=f32(np.array(F32)))
    assert np.array_equal(cs32['F'].astype(np.float64), np.array(F32))            # the float32 values are exact in F
    return dict(cs32=cs32, cs64=dict(base, F=np.array(F64)), proj=proj, where=np.array(where), edge=np.array(edge), expect=np.array(expect))


def tie_decisions(o, proj):
    """<gF, u_d v_d^T> per case -> (projection, decision)"""
    p = np.einsum('nij,nij->n', np.asarray(o['gF'], np.float64), proj)
    return p, p > 0.5
