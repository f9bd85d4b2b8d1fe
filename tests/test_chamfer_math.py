"""Host build of the nearest-point math of fluidlab_amd/csrc/fe_nearest.h -- the skip test, d2, the grid, the cell of a point, the ring
bound, the fixed-point deposit and the ring search that k_nn_query runs -- against numpy on seeded points
(tests/csrc/nearest_math_test.hip writes what the functions give, the comparisons are here).  100 grids x 100 queries: d2 bit for bit, the
search equal to the all-pairs restatement in index and bits, and the invariant the search rests on -- no point outside the rings 0 .. r is as
close as the bound of ring r -- by brute force over every ring, queries outside the box included.  No GPU, no oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from fluidlab_amd.fluidengine.losses import term_program as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'csrc', 'nearest_math_test.hip')
OUT = os.path.join(ROOT, 'tests', 'csrc', '_build')
MASKS = [7, 5, 2, 1, 3, 6, 4]
CELLS = [0, 1, 2, 3, 5, 8, 17, 64, 200]
M, Q, N_CASES = 150, 100, 100
RINGS = 65


def make_cases():
    rs = np.random.RandomState(11)
    cases = []
    for c in range(N_CASES):
        mask, cells = MASKS[c % len(MASKS)], CELLS[c % len(CELLS)]
        lo = rs.uniform(-1.5, 1.0, 3)
        ext = rs.uniform(0.01, 0.9, 3) * (rs.rand(3) < 0.85)      # now and then an axis without extent
        p = (lo + ext * rs.rand(M, 3)).astype(np.float32)
        if c % 5 == 1:                                           # two clusters and an empty middle
            p[: M // 2] = (lo + 0.1 * ext * rs.rand(M // 2, 3)).astype(np.float32)
        if c % 5 == 2:                                           # duplicated points
            p[M // 2:] = p[: M - M // 2][::-1]
        if c % 7 == 3:                                           # every point the same
            p[:] = p[0]
        if c % 4 == 0:                                           # points the skip test drops
            p[3] = [np.nan, 0.1, 0.1]
            p[5] = [0.1, np.inf, 0.1]
            p[7] = [2.5, -2.5, 2.5]
        q = (lo + ext * rs.rand(Q, 3)).astype(np.float32)
        q[: Q // 3] = rs.uniform(-2.0, 2.0, (Q // 3, 3)).astype(np.float32)      # mostly outside the box
        q[Q // 3: Q // 3 + 10] = p[:10]                          # on a point: d2 = 0 (or a skipped point)
        q[-1] = [np.nan, 0.0, 0.0]
        q[-2] = [0.0, 3.0, 0.0]
        cases.append((mask, cells, p, q))
    return cases


@pytest.fixture(scope='module')
def results():
    hipcc = '/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else shutil.which('hipcc')
    if hipcc is None:
        pytest.skip('hipcc not available')
    os.makedirs(OUT, exist_ok=True)
    exe, fin, fout = (os.path.join(OUT, n) for n in ('nearest_math_test', 'nearest_math_in.bin', 'nearest_math_out.bin'))
    subprocess.check_call([hipcc, '--offload-host-only', '-O2', '-std=c++17', '-x', 'hip', SRC, '-o', exe])
    cases = make_cases()
    with open(fin, 'wb') as f:
        f.write(np.int32(len(cases)).tobytes())
        for mask, cells, p, q in cases:
            f.write(np.array([mask, cells, len(p), len(q)], np.int32).tobytes())
            f.write(p.tobytes())
            f.write(q.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = np.fromfile(fout, np.float64)
    per = 10 + RINGS + M + 3 * M + Q + 3 * Q + Q * M + 3 * Q + 3 * Q + 3 + Q + Q * RINGS
    assert raw.size == per * len(cases)
    out = []
    for c, (mask, cells, p, q) in enumerate(cases):
        v, at = raw[c * per:(c + 1) * per], 0

        def take(n, shape=None):
            nonlocal at
            a = v[at:at + n]
            at += n
            return a if shape is None else a.reshape(shape)
        out.append(dict(mask=mask, cells=cells, p=p, q=q, lo=take(3), h=take(3), h_min=take(1)[0], n=take(3).astype(int), bound=take(RINGS),
                        ok=take(M) != 0, cell=take(3 * M, (M, 3)).astype(int), qok=take(Q) != 0, qcell=take(3 * Q, (Q, 3)).astype(int),
                        d2=take(Q * M, (Q, M)), found=take(3 * Q, (Q, 3)), quant=take(3 * Q, (Q, 3)), hi=take(3), gap2=take(Q),
                        qbound=take(Q * RINGS, (Q, RINGS))))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_skip_rule_and_grid(results):
    for R in results:
        mask = R['mask']
        assert (R['ok'] == TP.cloud_point_ok(R['p'], mask)).all() and (R['qok'] == TP.cloud_point_ok(R['q'], mask)).all()
        pts = R['p'][R['ok']].astype(np.float64)
        kmax = min(R['cells'], 64) if R['cells'] > 0 else 64
        for a in range(3):
            ext = pts[:, a].max() - pts[:, a].min() if (mask >> a) & 1 else 0.0
            assert 1 <= R['n'][a] <= kmax
            if ext == 0.0:
                assert R['n'][a] == 1
            if R['n'][a] > 1:
                assert R['lo'][a] == pts[:, a].min()
                assert R['h'][a] == ext / R['n'][a]
        edges = [R['h'][a] for a in range(3) if R['n'][a] > 1]
        if edges:
            assert R['h_min'] == min(edges)
        if R['cells'] == 1:
            assert tuple(R['n']) == (1, 1, 1)
        if R['cells'] == 0 and edges:                             # the engine's choice: about four points per cell, far from one cell
            assert int(np.prod(R['n'])) >= len(pts) // 32


def test_d2_cells_bound_and_deposit_match_numpy(results):
    for R in results:
        mask = R['mask']
        m = np.array([(mask >> a) & 1 for a in range(3)], np.float64)
        p, q = R['p'].astype(np.float64), R['q'].astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            d = np.where(m[None, None, :] != 0, q[:, None, :] - p[None, :, :], 0.0)
            want = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        both = R['qok'][:, None] & R['ok'][None, :]
        assert (_bits(R['d2'])[both] == _bits(want)[both]).all()
        r = np.arange(RINGS, dtype=np.float64)
        b = r * R['h_min']
        assert (_bits(R['bound']) == _bits((b * b + 0.0) * (1.0 - 2e-6))).all()
        # the gap of a query to the box of the members, over the axes of the mask, and the bounds with it
        pts = p[R['ok']]
        gap2 = np.zeros(len(q))
        for a in range(3):
            if (mask >> a) & 1:
                lo_a, hi_a = pts[:, a].min(), pts[:, a].max()
                assert R['hi'][a] == hi_a
                with np.errstate(invalid='ignore'):
                    g = np.where(q[:, a] < lo_a, lo_a - q[:, a], np.where(q[:, a] > hi_a, q[:, a] - hi_a, 0.0))
                gap2 = gap2 + g * g
        ok = R['qok']
        assert (_bits(R['gap2'])[ok] == _bits(gap2)[ok]).all() and (gap2[ok] > 0).any() and (gap2[ok] == 0).any()
        assert (_bits(R['qbound'])[ok] == _bits((b * b + gap2[ok][:, None]) * (1.0 - 2e-6))).all()
        for x, ok, got in ((p, R['ok'], R['cell']), (q, R['qok'], R['qcell'])):
            for a in range(3):
                if R['n'][a] == 1:
                    assert (got[:, a] == 0).all()
                    continue
                u = np.floor((x[ok, a] - R['lo'][a]) / R['h'][a])
                assert (got[ok, a] == np.clip(u, 0, R['n'][a] - 1).astype(int)).all()
        ok0 = R['qok'] & TP.cloud_point_ok(R['p'][:1], 7)[0]
        assert (R['quant'][ok0] == np.rint((q[ok0] - p[0]) * 2.0 ** 40)).all()


def test_no_point_outside_the_visited_rings_is_within_the_bound(results):
    pairs = 0
    for R in results:
        ok, qok = R['ok'], R['qok']
        cheb = np.abs(R['cell'][None, ok, :] - R['qcell'][qok][:, None, :]).max(axis=2)      # [queries, points]
        d2 = R['d2'][qok][:, ok]
        qb = R['qbound'][qok]
        assert (d2 >= qb[:, :1]).all()                            # before any ring: every member is at least the gap away
        for r in range(int(cheb.max()) + 1):
            out = cheb > r
            assert (d2[out] > np.broadcast_to(qb[:, r:r + 1], d2.shape)[out]).all(), (R['mask'], R['cells'], r)
        pairs += int(qok.sum())
    assert pairs >= 9000                                          # (10^4 pairs less the queries the skip test drops)


def test_ring_search_equals_all_pairs(results):
    for R in results:
        nn, d2 = TP.nearest_bruteforce(R['q'], R['p'], R['mask'])
        assert (R['found'][:, 0].astype(np.int64) == nn).all(), (R['mask'], R['cells'])
        assert (_bits(R['found'][:, 1]) == _bits(d2)).all()
        # where it stopped: at the bound, or at the last ring of the grid
        for i in np.nonzero(R['qok'])[0]:
            r = int(R['found'][i, 2])
            last = max(max(R['qcell'][i, a], R['n'][a] - 1 - R['qcell'][i, a]) for a in range(3))
            assert 0 <= r <= last
            assert r == last or d2[i] <= R['qbound'][i, r]
