"""Inputs, the numpy restatement and library loading for the tests of fluidlab_amd/csrc/fe_smoke_index.h (tests/test_smoke_index.py on the
CPU, tests/test_smoke_index_hip.py on the GPU).  tests/csrc/smoke_index_test.hip wraps sm_tri_axis in a host entry and a one-lane-per-case
kernel; this module builds it, after the pattern of tests/math_cases.py."""
import ctypes
import functools
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'smoke_index_test.hip')
HEADER = os.path.join(ROOT, 'fluidlab_amd', 'csrc', 'fe_smoke_index.h')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')

f32 = np.float32
P_MAX = f32(2.0 ** 30)
GRIDS = (1, 2, 16, 128)


def hipcc():
    return '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')


def _compile(lib, flags):
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(SRC), os.path.getmtime(HEADER)):
        os.makedirs(OUT, exist_ok=True)
        tmp = f'{lib}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc()] + flags + ['-o', tmp, SRC])
        os.replace(tmp, lib)
    return lib


def build_host_lib():
    return _compile(os.path.join(OUT, 'libsmoke_index_test_host.so'),
                    ['--offload-host-only', '-O2', '-std=c++17', '-shared', '-fPIC', '-DSIT_HOST_ONLY', '-x', 'hip'])


def build_device_lib():
    """the gfx950 kernel, its launcher and the CPU entry, with the flags the engine is built with"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    return _compile(os.path.join(OUT, 'libsmoke_index_test.so'), list(entry.HIPCC_FLAGS))


class IndexLib:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)

    def axis(self, p, n, entry='sit_axis_host'):
        """-> rc, base (int32), f (float32), c0, c1 (int32)"""
        p = np.ascontiguousarray(p, f32)
        m = p.size
        base, c0, c1 = (np.full(m, -12345, np.int32) for _ in range(3))
        f = np.full(m, np.nan, f32)
        fn = getattr(self.lib, entry)
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int], ctypes.c_int
        rc = fn(*[a.ctypes.data_as(ctypes.c_void_p) for a in (p,)], int(n), *[a.ctypes.data_as(ctypes.c_void_p) for a in (base, f, c0, c1)], m)
        return rc, base, f, c0, c1


@functools.lru_cache(None)
def host_lib():
    return IndexLib(build_host_lib())


@functools.lru_cache(None)
def device_lib():
    return IndexLib(build_device_lib())


def _bits(u):
    return np.array(u, np.uint32).view(f32)


@functools.lru_cache(None)
def cases():
    """every case class, then 100,000 seeded values over +-1.5 * 2^30 and 100,000 in [-2, 128 + 2] (the largest grid; the tests cut the second
    set to [-2, n + 2] per grid by scaling)"""
    fmax = np.finfo(f32).max
    edge = [0.0, 0.5, 2.0 ** 24, 2.0 ** 30 - 64, 2.0 ** 30, 3e9, 2.0 ** 31, 3e38, fmax, np.inf]
    edge += [n + 0.5 for n in GRIDS] + [n - 0.5 for n in GRIDS]
    cls = np.array([s * v for v in edge for s in (1.0, -1.0)], f32)
    nan = _bits([0x7FC00000, 0xFFC00000, 0x7FA00000, 0xFFA00000, 0x7F800001])          # quiet, quiet with sign, signalling x 3
    den = _bits([0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF])                      # smallest and largest denormals
    rng = np.random.RandomState(20251)
    wide = rng.uniform(-1.5 * 2.0 ** 30, 1.5 * 2.0 ** 30, 100000).astype(f32)
    unit = rng.uniform(0.0, 1.0, 100000)
    return dict(cls=np.concatenate([cls, nan, den]), wide=wide, unit=unit)


def inputs(n):
    c = cases()
    near = (-2.0 + c['unit'] * (n + 4.0)).astype(f32)                                  # [-2, n + 2]
    return np.concatenate([c['cls'], c['wide'], near])


def restate(p, n):
    """sm_tri_axis in numpy, float32 operation by operation: -> base (int64), f (float32), c0, c1 (int64)"""
    p = np.asarray(p, f32)
    lo, hi = -P_MAX, P_MAX
    with np.errstate(invalid='ignore'):
        q = np.where(p > lo, np.where(p < hi, p, hi), lo).astype(f32)                  # NaN compares false: -> lo
    t = (q - f32(0.5)).astype(f32)
    fl = np.floor(t)
    base = fl.astype(np.int64)
    f = (t - fl.astype(f32)).astype(f32)
    return base, f, np.clip(base, 0, n - 1), np.clip(base + 1, 0, n - 1)


def old_expression(p):
    """what sm_trilerp computed before the helper, for finite |p| <= 2^30 only: (int)floorf(p - 0.5f) in int64, p - 0.5f - (float)base in float32"""
    p = np.asarray(p, f32)
    t = (p - f32(0.5)).astype(f32)
    fl = np.floor(t)
    return fl.astype(np.int64), (t - fl).astype(f32)
