"""CPU: scenarios.rigid_bodies_many on the oracle alone.  test_rigid_bodies_hip.py holds the HIP engine's k_rigid_body to
bounds taken from this scene (twice what the fp32 oracle loses against the fp64 one); these tests establish that the scene
supports such bounds -- the oracle agrees with the independent numpy restatement on it, every body's H is well conditioned
at every substep (so the SVD adjoint is a derivative), fp32 stays far inside the 1e-2 cap -- and record what the oracle does
with a body that has no used particle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402
import rigid_cases as RC  # noqa: E402
from rigid_cases import mpm_numpy  # noqa: E402


def test_scene_layout():
    sc = RC.scene('plain')
    counts = [int((sc['body_id'] == b).sum()) for b in RC.bodies(sc)]
    assert counts == list(S.RIGID_MANY_COUNTS) and sc['N'] == 1000 + sum(counts)
    assert [-(-c // 256) for c in counts] == [1, 1, 1, 1, 1, 2, 3, 3]        # passes of the 256-thread workgroup
    cls = np.array([S.MATERIALS[int(m)][3] for m in sc['mat']])
    assert ((cls == S.MAT_RIGID) == (sc['body_id'] > 0)).all()
    lo = np.array([sc['x'][sc['body_id'] == b].min(0) for b in RC.bodies(sc)])
    hi = np.array([sc['x'][sc['body_id'] == b].max(0) for b in RC.bodies(sc)])
    for i in range(len(lo)):                                                  # the boxes do not overlap
        for j in range(i):
            assert ((lo[i] > hi[j]) | (lo[j] > hi[i])).any(), (i + 1, j + 1)
    ext = np.sort(hi - lo, axis=1)
    assert (ext[:, 1] >= 1.25 * ext[:, 0]).all() and (ext[:, 2] >= 1.25 * ext[:, 1]).all()      # three different extents
    dx = 1.0 / sc['n_grid']
    assert (lo.min(0) - dx >= np.array(sc['boundary']['lower'])).all() and (hi.max(0) + dx <= np.array(sc['boundary']['upper'])).all()
    # the variants change what they say and nothing else
    sca, wb, il = RC.scene('scattered'), RC.scene('whole_body'), RC.scene('interleave')
    for b in RC.bodies(sc):
        want = np.ones(counts[b - 1], np.int32)
        if b in (4, 7):
            want[::7] = 0
        assert (sca['used'][sca['body_id'] == b] == want).all()
        assert (wb['used'][wb['body_id'] == b] == (0 if b == RC.UNUSED_BODY else 1)).all()
    assert (sca['x'] == sc['x']).all() and (wb['x'] == sc['x']).all()
    for b in RC.bodies(il):                                                   # interleaved: no body's pids are contiguous
        pid = np.flatnonzero(il['body_id'] == b)
        assert len(pid) == counts[b - 1] and pid[-1] - pid[0] + 1 > 2 * len(pid)
    order = np.lexsort(il['x'].T), np.lexsort(sc['x'].T)
    for k in ('x', 'v', 'F', 'C', 'used', 'mat', 'body_id'):                  # the same particles in another order
        assert (il[k][order[0]] == sc[k][order[1]]).all(), k
    three = RC.scene('three')
    assert three['N'] == sc['N'] and int(three['body_id'].max()) == 3


@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave'])
def test_oracle_matches_numpy(oracle64, variant):
    sc = RC.scene(variant)
    frames = RC.rollout(oracle64, variant)['frames']
    props = np.array([S.MATERIALS[int(m)] for m in sc['mat']])
    n = sc['n_grid']
    x, v, C, F = (frames[0][k].astype(np.float64) for k in 'xvCF')
    for f in range(4):
        x, v, C, F, _ = mpm_numpy.substep(x, v, C, F, sc['used'], props[:, 0], props[:, 1], (0.5 / n) ** 2 * props[:, 2],
                                          props[:, 3].astype(int), n, sc['dt'], (0.5 / n) ** 2, sc['gravity'], sc['boundary'],
                                          body_id=sc['body_id'])
    for k, ref in zip('xvCF', (x, v, C, F)):
        assert np.abs(frames[4][k] - ref).max() < 1e-9 * max(1.0, np.abs(ref).max()), k
    for b in RC.bodies(sc):
        sel = (sc['body_id'] == b) & (sc['used'] == 1)
        assert np.abs(RC.pairwise(frames[4]['x'][sel]) - RC.pairwise(frames[0]['x'][sel])).max() < 1e-12
        assert np.abs(frames[4]['x'][sel] - frames[0]['x'][sel]).max() > 1e-4      # and the body did move


@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave', 'whole_body', 'three'])
def test_every_body_is_well_conditioned(oracle64, variant):
    """backward_svd divides by s_j^2 - s_i^2 (mpm:272-292): pairwise gaps >= 0.1 s_max and s_min >= 0.05 s_max at every substep"""
    sc = RC.scene(variant)
    frames = RC.rollout(oracle64, variant)['frames']
    worst_gap, worst_min = np.inf, np.inf
    for f in range(RC.N_SUB):
        for b in RC.bodies(sc):
            s = RC.body_H_singular_values(sc, frames[f], frames[f + 1]['v'], b)
            if s is None:
                assert variant == 'whole_body' and b == RC.UNUSED_BODY
                continue
            gap = min(s[0] - s[1], s[1] - s[2]) / s[0]
            worst_gap, worst_min = min(worst_gap, gap), min(worst_min, s[2] / s[0])
            assert gap >= 0.1 and s[2] >= 0.05 * s[0], (f, b, s)
    print(f'MEASURED rigid_conditioning[{variant}]: min gap / s_max {worst_gap:.3f}  min s_min / s_max {worst_min:.3f}')


@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave', 'whole_body', 'three'])
def test_fp32_yardstick(oracle32, oracle64, variant):
    """What the fp32 oracle loses against the fp64 one over the rollout: the GPU bounds are twice these, capped at 1e-2"""
    y = RC.yardstick(oracle32, oracle64, variant)
    print(f'MEASURED rigid_yardstick[{variant}]: d_x {y["d_x"]:.2e}  d_g ' + ' '.join(f'{k} {y["d_g"][k]:.2e}' for k in RC.GRADS) +
          '  d_grigid ' + ' '.join(f'{k} {y["d_grigid"][k]:.2e}' for k in RC.GRADS) +
          '  d_body(gx) ' + ' '.join(f'{b}:{d:.1e}' for b, d in y['d_body'].items()))
    g64 = RC.rollout(oracle64, variant)['grad']
    for k in RC.GRADS:
        assert np.isfinite(g64[k]).all(), k
        assert y['d_g'][k] <= 1e-2 and y['d_grigid'][k] <= 1e-2, (k, y['d_g'][k], y['d_grigid'][k])
    assert 0 < y['d_x'] < np.inf


@pytest.mark.parametrize('variant', ['plain', 'scattered', 'interleave'])
def test_numpy_chain_is_the_oracles_rigid_step(oracle64, variant):
    """rigid_cases.shape_match -- the reference of the GPU test of the kernel alone -- reproduces the fp64 oracle's rigid
    particles from the oracle's own x[f], used, v[f+1] when these are fp32 numbers (frame 0 is), and its fp32 run gives e32"""
    sc = RC.scene(variant)
    frames = RC.rollout(oracle64, variant)['frames']
    x0, v1 = frames[0]['x'], S.f32(frames[1]['v'])
    ref =RC.shape_match(S.f32(x0), v1, frames[0]['used'], sc['body_id'], sc['dt'], np.float64)
    lo = RC.shape_match(S.f32(x0), v1, frames[0]['used'], sc['body_id'], sc['dt'], np.float32)
    e32 = {b: float(np.abs(lo[b][1] - ref[b][1]).max()) for b in ref}
    print(f'MEASURED rigid_e32[{variant}, oracle frame 0]: ' + ' '.join(f'{b}:{e:.1e}' for b, e in e32.items()))
    assert sorted(ref) == list(RC.bodies(sc))
    for b, (sel, new) in ref.items():
        # v[1] of the oracle was rounded to fp32 for the chain: dt |dv| <= 2e-4 * 2^-24 |v| moves a particle by less than 1e-10
        assert np.abs(new - frames[1]['x'][sel]).max() <= 1e-10, b
        assert 0 < e32[b] <= 2e-6, (b, e32[b])              # fp32 sums of O(1) coordinates: a few ulp, never exact


def test_whole_unused_body_on_the_oracle(oracle64):
    """A body without a used particle: H = 0, and the oracle runs svd3 / backward_svd on it, but no particle reads the
    result.  Its particles keep x, v, C, F bit for bit in every frame (unused particles are carried over), and the adjoint
    of an unused particle is carried back unchanged as well: at frame 0 it equals the cotangent seeded on the last frame,
    bit for bit.  test_rigid_bodies_hip.py asks the same of the HIP engine."""
    sc = RC.scene('whole_body')
    r = RC.rollout(oracle64, 'whole_body')
    body = sc['body_id'] == RC.UNUSED_BODY
    assert body.sum() == 65 and (sc['used'][body] == 0).all()
    for f in range(RC.N_SUB + 1):
        assert (r['frames'][f]['used'][body] == 0).all()
        for k in 'xvCF':
            assert (r['frames'][f][k][body] == r['frames'][0][k][body]).all(), (f, k)
    cot = RC.cotangent(sc, np.float64)
    for k in RC.GRADS:
        assert np.isfinite(r['grad'][k]).all(), k
        assert (r['grad'][k][body] == cot[k][body]).all(), k
    # everything else is the plain scene minus that body's grid contribution: the other bodies are still moved rigidly
    for b in RC.bodies(sc):
        sel = (sc['body_id'] == b) & (sc['used'] == 1)
        if sel.any():
            assert np.abs(RC.pairwise(r['final']['x'][sel]) - RC.pairwise(sc['x'][sel])).max() < 1e-12
