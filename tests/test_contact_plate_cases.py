"""The plate scene of tests/contact_plate_cases.py on the CPU: the fp64 oracle alone fixes the classification and satisfies the scene's conditions (at
least 100 sure contact particles, 20 of each of slide and separating -- and stick at friction 2 --, at most 15 % of the contacts unsure); the oracle's
forward velocity of frame 1 agrees per particle with the numpy restatement the classification is taken from; and the fp32 oracle's distance from the fp64
oracle in every compared quantity -- the yardstick of the GPU test -- is printed and finite."""
import numpy as np
import pytest

import contact_plate_cases as P


@pytest.mark.parametrize('vi', range(len(P.VARIANTS)))
def test_plate_scene_conditions_and_fp32_yardstick(oracle32, oracle64, vi):
    sc = P.plate_scene(vi)
    r64 = P.run_plate(oracle64, sc, classify=True)
    cls = r64['cls']
    counts = P.check_conditions(cls, vi)
    m = cls['contact'] & cls['sure']
    e_fwd = np.abs(r64['v1'] - cls['v1_ref'])[r64['used']].max()
    r32 = P.run_plate(oracle32, sc, sure=cls['sure'])
    e32, fl = P.errors(r32, r64, cls), P.floors(r64, cls)
    print(f'MEASURED plate {P.VARIANTS[vi]}: {counts}; fp64 oracle v\' vs numpy {e_fwd:.3g}; fp32 oracle vs fp64 {e32}; floors {fl}')
    # the restatement reads the plate's two poses through the ABI, which hands them over as float32: half a step at 0.5 (3e-8) in each, over dt = 2e-4
    assert e_fwd <= 2 * 3e-8 / sc['dt']
    assert np.abs(r64['gx']).max() > 0 and np.abs(r64['action_grad']).max() > 0 and m.sum() >= P.MIN_SURE
    assert all(np.isfinite(v) for v in e32.values())
    # zeroing the cotangent on the unsure particles takes their contact out of the adjoint: the fp32 oracle, whose unsure particles may sit on another
    # branch, stays within 1e-3 of the field's range of the fp64 oracle in every gradient (with them in, a single flipped particle moves gv by O(1))
    for k in ('gx', 'gv', 'action_grad'):
        assert e32[k] <= 1e-3 * fl[k] / 2.4e-7, (k, e32[k], fl[k])


def test_two_tool_scene_conditions_and_fp32_yardstick(oracle32, oracle64):
    """collide_type = 3, the sphere and the plate as two meshed effectors: the pose leaves NO massy node unsure (asserted: the count is 0), so the only contact
    Jacobians the classification cannot vouch for are particle-level ones, which act after the gather -- zeroing the cotangent on the unsure particles takes them
    out of the whole adjoint, and the fp32 oracle, free to sit on other branches there, stays within 1e-3 of each gradient's range of the fp64 oracle.  At least
    20 sure particles (and some nodes) hit both colliders: the chain runs twice and the adjoint walks it backwards."""
    sc = P.two_tool_scene()
    r64 = P.run_two(oracle64, sc, classify=True)
    cls = r64['cls']
    both = int((cls['both'] & cls['sure']).sum())
    unsure = float((cls['contact'] & ~cls['sure']).sum()) / int(cls['contact'].sum())
    e_fwd = np.abs(r64['v1'] - cls['v1_ref'])[r64['used']].max()
    r32 = P.run_two(oracle32, sc, sure=cls['sure'])
    e32, fl = P.errors(r32, r64, cls), P.floors(r64, cls)
    print(f'MEASURED two tools: nodes unsure {cls["node_unsure"]} in contact {cls["node_hits"]} with both {cls["node_both"]}; particles in contact {int(cls["contact"].sum())} '
          f'sure with both {both} unsure share {unsure:.3f}; fp64 oracle v\' vs numpy {e_fwd:.3g}; fp32 oracle vs fp64 {e32}; floors {fl}')
    assert cls['node_unsure'] == 0 and cls['node_hits'] >= 20 and cls['node_both'] >= 1
    assert both >= P.MIN_BOTH and unsure <= P.MAX_UNSURE
    assert e_fwd <= 2 * 2 * 3e-8 / sc['dt']                # two colliders, each with two poses read as float32 through the ABI
    assert np.abs(r64['action_grad'][:12]).max() > 0 and np.abs(r64['action_grad'][12:]).max() > 0          # both effectors take a gradient
    for k in ('gx', 'gv', 'action_grad'):
        assert np.isfinite(e32[k]) and e32[k] <= 1e-3 * fl[k] / 2.4e-7, (k, e32[k], fl[k])
