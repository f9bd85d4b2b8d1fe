"""The engine's hand-assembled collide adjoint (collide_chain_grad_row) on the thin plate, one substep forward and backward, particle by particle
(scene, classification and runner: tests/contact_plate_cases.py; the CPU half, tests/test_contact_plate_cases.py, fixes the classification from the fp64
oracle and holds the scene's conditions).  Every trajectory test that compares contact values uses a sphere; this one uses the box, with the cotangent of
frame 1 zero on the particles the fp64 classification calls unsure (flat cell layer, near a branch edge), so that what remains is well conditioned and a
wrong column of the adjoint shows as a per-particle error.  Bound on each quantity: 4 x what the oracle's own fp32 build loses against its fp64 build, plus
four float32 steps of the field's range -- the rule of tests/test_csrc_geom_hip.py with the oracle's fp32 build as the realisation measured against.
Not compared: eff_get_state_grad, which the oracle does not have.  The action gradient is a linear image of those 7-vectors (through t_move_quat and the
action_p map); what lies in that image's null space is NOT seen -- for one, the component of frame 1's quaternion adjoint along the quaternion itself, which
t_move_quat's normalisation annihilates."""
import numpy as np
import pytest

import contact_plate_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('vi', range(len(P.VARIANTS)))
def test_plate_one_substep_per_particle(hiplib, oracle32, oracle64, vi):
    sc = P.plate_scene(vi)
    r64 = P.run_plate(oracle64, sc, classify=True)
    cls = r64['cls']
    counts = P.check_conditions(cls, vi)
    r32 = P.run_plate(oracle32, sc, sure=cls['sure'])
    rh = P.run_plate(hiplib, sc, sure=cls['sure'])
    eh, e32, fl = P.errors(rh, r64, cls), P.errors(r32, r64, cls), P.floors(r64, cls)
    print(f'MEASURED plate {P.VARIANTS[vi]} {counts}: ' + ' '.join(f'{k} HIP {eh[k]:.3g} fp32 oracle {e32[k]:.3g} floor {fl[k]:.3g}' for k in eh))
    assert np.array_equal(rh['used'], r64['used'])
    for k in ('v1', 'gx', 'gv', 'action_grad'):
        assert np.isfinite(rh[k]).all(), k
        assert eh[k] <= 4.0 * e32[k] + fl[k], (P.VARIANTS[vi], k, eh[k], e32[k], fl[k])
    # the pose adjoints exist and the contact put something into both frames
    eng_ok = np.abs(rh['action_grad']).max() > 0 and np.abs(rh['gx'][cls['contact'] & cls['sure']]).max() > 0
    assert eng_ok


def test_two_tools_node_and_particle_chain(hiplib, oracle32, oracle64):
    """collide_type = 3 with the sphere and the plate as two meshed effectors of one agent: both collide at the grid nodes and at the particles, 86 sure
    particles and 10 nodes hit both -- the reversed chain loop and vin[ei] of collide_chain_grad_row, and the node-level collide adjoint on a box.  No massy
    node is unsure at this pose (tests/test_contact_plate_cases.py asserts the count is 0); the cotangent is zero on the unsure particles.  Same bound as above;
    the action gradient is both effectors' rows."""
    sc = P.two_tool_scene()
    r64 = P.run_two(oracle64, sc, classify=True)
    cls = r64['cls']
    assert cls['node_unsure'] == 0 and (cls['both'] & cls['sure']).sum() >= P.MIN_BOTH
    r32 = P.run_two(oracle32, sc, sure=cls['sure'])
    rh = P.run_two(hiplib, sc, sure=cls['sure'])
    eh, e32, fl = P.errors(rh, r64, cls), P.errors(r32, r64, cls), P.floors(r64, cls)
    m = cls['both'] & cls['sure']
    eh['v1_both'], e32['v1_both'] = (float(np.abs(a['v1'] - r64['v1'])[m].max()) for a in (rh, r32))          # v' of the particles that hit both
    fl['v1_both'] = fl['v1']
    print('MEASURED two tools: ' + ' '.join(f'{k} HIP {eh[k]:.3g} fp32 oracle {e32[k]:.3g} floor {fl[k]:.3g}' for k in eh))
    assert np.array_equal(rh['used'], r64['used'])
    for k in eh:
        assert eh[k] <= 4.0 * e32[k] + fl[k], (k, eh[k], e32[k], fl[k])
    assert np.isfinite(rh['gx']).all() and np.isfinite(rh['gv']).all() and np.isfinite(rh['action_grad']).all()
    assert np.abs(rh['action_grad'][:12]).max() > 0 and np.abs(rh['action_grad'][12:]).max() > 0


def test_collide_min_y_through_the_plate(hiplib):
    """collide_min_y set through the plate's centre (y = 0.47): the particles that end below it -- by more than 1e-6, sixteen float32 steps of y -- are as in a
    run without the mesh (the collider acts on particles only at collide_type = 1, so nothing reaches them through the grid); above it the plate still acts.
    F is equal bit by bit (it is made from frame 0's C and F alone).  v and C cannot be, between any two runs of this engine: the scatter's float atomics sum in another order each time, and two
    IDENTICAL mesh-free runs of this scene differ in v in 1,350 of 1,500 rows by up to 1.5e-8 and in C by up to 1.9e-6 (measured on an MI355X; cut against free
    below the cut: 1.5e-8 and 2.2e-6, the same steps).  v is held to four float32 steps of its range, C to what that spread in the node velocities makes of it, and x = x0 + dt v to one float32 step of a position
    below 1 (dt dv = 3e-12 moves x only where it crosses a rounding boundary); a particle the plate touches moves by O(1)."""
    sc = P.plate_scene(0)
    min_y = 0.47
    free = P.forward_frame(hiplib, sc, mesh=False)
    cut = P.forward_frame(hiplib, sc, options={'collide_min_y': min_y})
    full = P.forward_frame(hiplib, sc)
    used = free['used'].astype(bool)
    below = used & (free['x'][:, 1] <= min_y - 1e-6)
    above = used & (free['x'][:, 1] > min_y + 1e-6)
    step = {'v': 4 * 6e-8 * float(np.abs(free['v'][used]).max())}
    # C = 4 inv_dx sum_i w_i v_i (x_i - x_p) / dx with sum w = 1 and |x_i - x_p| / dx <= 1.5: a spread of step_v in the node velocities is 6 n_grid step_v in C
    step['C'] = 6 * sc['n_grid'] * step['v']
    touched = np.abs(full['v'] - free['v']).max(axis=1) > 1e-5
    dv, dC = (float(np.abs(cut[k][below].astype(np.float64) - free[k][below]).max()) for k in ('v', 'C'))
    print(f'MEASURED collide_min_y: {int(below.sum())} particles below, {int((touched & below).sum())} of them in contact without the cut, '
          f'{int((touched & above).sum())} in contact above; cut vs free below: v {dv:.3g} (allowed {step["v"]:.3g}) C {dC:.3g} (allowed {step["C"]:.3g})')
    assert below.sum() >= 100 and (touched & below).sum() >= 20 and (touched & above).sum() >= 20
    assert np.array_equal(cut['F'][below].view(np.uint32), free['F'][below].view(np.uint32))
    assert np.abs(cut['x'][below].astype(np.float64) - free['x'][below]).max() <= 6e-8
    assert dv <= step['v'] and dC <= step['C']
    assert np.abs(cut['v'][above].astype(np.float64) - full['v'][above]).max() <= step['v']          # above the cut: the plate as without it
    assert np.abs(cut['v'] - free['v'])[touched & above].max() > 1e-3          # (and it does act there)
