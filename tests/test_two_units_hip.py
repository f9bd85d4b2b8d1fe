"""The HIP engine is two translation units in one library: fe_particles.hip emits the particle kernels and defines their launchers, fe_engine.hip the grid
kernels, the sort, the host code and the C ABI, and every particle launch crosses from one to the other through fe_particle_launch.h.  One small
water block through a 12-substep window, forward and backward, against the fp64 oracle -- with the default options (the fused launches, the separate
kernels at a sort, the grid kernels and the sort: every crossing in both directions), with fuse_g2p = fuse_bwd = 0 (the separate particle kernels and
their launchers throughout) and as two engines through fe_step_batch / fe_step_grad_batch (the _b entries).  Tolerances: those of
tests/test_hip_parity.py for the same quantities on its water blocks with a sort every few substeps and a ranged reverse sweep
(test_grid_sizes_with_an_odd_number_of_blocks_per_axis): max |dx| <= 2e-6, rel L2 (v) <= 1e-4, adjoints cosine >= 0.99999 and rel L2 <= 1e-3.
The last test needs no GPU: the hash recorded beside the library covers every source and header of both units."""
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import scenarios as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 12
N = 4000


def _scene(seed):
    sc = S.water_block(n_grid=32, n_particles=N, seed=seed)
    sc['v'] = S.f32(np.random.RandomState(40 + seed).normal(0, 0.5, (N, 3)))
    return sc


_REF = {}


def _oracle(oracle64, seed):
    """the fp64 reference of scene `seed`, computed once and shared by the cases that use it (nobody writes to it)"""
    if seed not in _REF:
        cot = S.random_cotangent(N, seed=60 + seed)
        _REF[seed] = S.run_forward_backward(S.make_engine(oracle64, _scene(seed)), L, {k: v.astype(np.float64) for k, v in cot.items()})
    return _REF[seed]


def _check(name, st, g, ref):
    sb, gb = ref
    print(f'MEASURED two units [{name}]: max|dx| {np.abs(st["x"] - sb["x"]).max():.2e} v relL2 {S.rel_l2(st["v"], sb["v"]):.2e} ' +
          ' '.join(f'{k} 1-cos {1 - S.cosine(g[k], gb[k]):.1e} relL2 {S.rel_l2(g[k], gb[k]):.2e}' for k in ('gx', 'gv', 'gC', 'gF')))
    assert (st['used'] == sb['used']).all()
    assert np.abs(st['x'] - sb['x']).max() <= 2e-6
    assert S.rel_l2(st['v'], sb['v']) <= 1e-4
    for k in ('gx', 'gv', 'gC', 'gF'):
        assert np.isfinite(g[k]).all(), k
        assert S.cosine(g[k], gb[k]) >= 0.99999, (k, S.cosine(g[k], gb[k]))
        assert S.rel_l2(g[k], gb[k]) <= 1e-3, (k, S.rel_l2(g[k], gb[k]))


def _grads(eng):
    gx, gv, gC, gF = eng.get_grad(0)
    return dict(gx=gx, gv=gv, gC=gC, gF=gF)


@pytest.mark.gpu
@pytest.mark.parametrize('separate', [False, True], ids=['default', 'separate'])
def test_window_crosses_the_units(hiplib, oracle64, separate):
    opts = {'sort_interval': 4}
    if separate:
        opts.update(fuse_g2p=0, fuse_bwd=0)
    cot = S.random_cotangent(N, seed=60)
    eng = S.make_engine(hiplib, _scene(0), max_substeps_local=L, options=opts)
    eng.profile_enable(True)
    eng.step(0, 0, L, 0)
    eng.reset_grad(); eng.add_grad(L, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    eng.step_grad(0, 0, L, 0)
    prof = eng.profile_read()
    eng.profile_enable(False)
    print('launches', {k: v[1] for k, v in prof.items() if v[1]})
    if separate:                                           # no fused launch: the separate kernels and their launchers throughout
        assert prof['g2p_p2g'][1] == 0 and prof['pgg_g2pg'][1] == 0 and prof['p2g'][1] == L and prof['g2p'][1] == L and prof['p2g_grad'][1] == L, prof
    elif eng.get_option('fuse_g2p') == 1.0 and eng.get_option('fuse_bwd') == 1.0:      # (the defaults, unless an FE_* override of the run changed them)
        assert prof['g2p_p2g'][1] > 0 and prof['p2g'][1] > 0 and prof['pgg_g2pg'][1] > 0 and prof['p2g_grad'][1] > 0, prof      # fused launches and, at the sorts, the separate ones
    assert prof['sort'][1] > 0 and (prof['grid_op'][1] == L or eng.get_option('fuse_grid') != 0.0), prof      # the engine unit's own kernels between them
    _check('separate' if separate else 'default', S.get_state(eng, L), _grads(eng), _oracle(oracle64, 0))
    eng.close()


@pytest.mark.gpu
def test_two_engines_in_a_batch(hiplib, oracle64):
    engs = [S.make_engine(hiplib, _scene(seed), max_substeps_local=L, options={'sort_interval': 4}) for seed in (0, 1)]
    type(engs[0]).step_batch(engs, 0, 0, L, 0)
    for seed, eng in enumerate(engs):
        cot = S.random_cotangent(N, seed=60 + seed)
        eng.reset_grad(); eng.add_grad(L, cot['gx'], cot['gv'], cot['gC'], cot['gF'])
    type(engs[0]).step_grad_batch(engs, 0, 0, L, 0)
    for seed, eng in enumerate(engs):
        _check(f'batch, engine {seed}', S.get_state(eng, L), _grads(eng), _oracle(oracle64, seed))
        eng.close()


def _includes(path, seen):
    """the project's own files a source reaches through #include "..." (transitively), by name"""
    for inc in re.findall(r'^\s*#include "([^"]+)"', open(path).read(), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if p not in seen and os.path.exists(p):
            seen.add(p)
            _includes(p, seen)
    return seen


def test_source_hash_covers_every_header_of_both_units(tmp_path):
    import __graft_entry__ as g
    srcs = g.engine_sources()
    assert len(set(srcs)) == len(srcs)
    names = {os.path.normpath(s) for s in srcs}
    for unit in ('fe_particles.hip', 'fe_engine.hip'):
        unit_path = os.path.join(g.CSRC, unit)
        missing = sorted(p for p in _includes(unit_path, {os.path.normpath(unit_path)}) if p not in names)
        assert not missing, f'{unit} is built from files the recorded hash does not cover: {missing}'
    # a copy of the sources: the hash moves when any one of them does -- a header of the particle unit, one of the engine unit, the shared ones
    copies = []
    for s in srcs:
        copies.append(str(tmp_path / os.path.basename(s)))
        shutil.copy(s, copies[-1])
    base = g._source_hash(copies)
    assert base == g._source_hash(srcs) == g._source_hash(copies)
    for name in ('fe_particle_launch.h', 'fe_math.h', 'fe_grid_launch.h', 'fe_field_obs.h', 'fe_particles.hip', 'fe_engine.hip', 'fluidengine_ext.h'):
        path = str(tmp_path / name)
        assert path in copies, name
        text = open(path, 'rb').read()
        with open(path, 'ab') as f:
            f.write(b'\n// touched\n')
        assert g._source_hash(copies) != base, name
        with open(path, 'wb') as f:
            f.write(text)
        assert g._source_hash(copies) == base, name
    # ... and when a unit's flags do
    flags = g.UNITS
    try:
        g.UNITS = tuple((obj, src, list(extra) + (['-DX'] if obj == 'fe_particles' else [])) for obj, src, extra in flags)
        assert g._source_hash(copies) != base
    finally:
        g.UNITS = flags
