"""Cost and coverage of fe_contact_wrench (include/fluidengine_ext.h; kernels in csrc/fe_contact.h): the benchmark block (bench.py: 128^3 grid,
200,000 particles of water) beside one static sphere of a 128^3 SDF lattice, and Mixing-v0, Pouring-v0 and IceCreamDynamic-v0 as shipped.
Per scene: the call for one substep and for the substeps of a step, wall clock with the engine's stream drained before the clock starts and
again before it stops, 5 warm-up calls, then the median of 30; and the coverage -- the share of substeps whose grid the engine kept in its
store, the only ones the call reports -- over a 5-step rollout with random actions.
usage: python scripts/contact_wrench_cost.py [--commit TEXT] [--out FILE] [--only NAME]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fluidlab_amd import _capi, scenes as S  # noqa: E402
from fluidlab_amd.envs import make  # noqa: E402

STEPS = 5


def timed(sync, fn, warm=5, n=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        sync()
        t0 = time.perf_counter(); fn(); sync(); ts.append(time.perf_counter() - t0)
    return 1e6 * statistics.median(ts), 1e6 * min(ts), 1e6 * max(ts)


def report(emit, name, eng, f0, ns, valid, contacts):
    one = timed(eng.sync, lambda: eng.contact_wrench(f0, 1))
    step = timed(eng.sync, lambda: eng.contact_wrench(f0, ns))
    emit(f'{name}: {eng.contact_count()} colliders, N {eng.N}; coverage over {STEPS} steps of {ns} substeps {np.mean(valid):.3f} '
         f'(per step {" ".join(f"{v:.2f}" for v in valid)}); contacts counted {contacts}')
    emit(f'  one substep              {one[0]:9.1f} ({one[1]:.1f} .. {one[2]:.1f})')
    emit(f'  the {ns:3d} substeps of a step {step[0]:9.1f} ({step[1]:.1f} .. {step[2]:.1f})')


def block(emit):
    sc = S.water_block(n_grid=128, n_particles=200_000, seed=0)
    res = 128
    g = np.linspace(0.0, 1.0, res)
    X, Y, Z = np.meshgrid(g, g, g, indexing='ij')
    vox = S.f32(np.sqrt((X - 0.42) ** 2 + (Y - 0.30) ** 2 + (Z - 0.45) ** 2) - 0.12)      # a sphere that reaches into the block from below
    T = np.array([[res - 1, 0, 0, 0], [0, res - 1, 0, 0], [0, 0, res - 1, 0], [0, 0, 0, 1.0]])
    sc['statics'] = [dict(voxels=vox, T=T, friction=0.5)]
    ns = sc['n_substeps']
    eng = S.make_engine(_capi.load_hip(), sc, max_substeps_local=100)
    valid, contacts = [], 0
    for s in range(STEPS):
        eng.step(s * ns, s * ns, ns, 0)
        rec = eng.contact_wrench(s * ns, ns)
        valid.append(float((rec['valid'] != 0).all(1).mean()))
        contacts += int(rec['n_particles'].sum() + rec['n_nodes'].sum())
    report(emit, 'benchmark block + one res-128 static', eng, (STEPS - 1) * ns, ns, valid, contacts)
    eng.close()


def environment(emit, name):
    env = make(name, seed=0, loss=False)
    env._get_reward = lambda: 0.0                              # (no loss object: the rollout is what matters)
    te = env.taichi_env
    sim = te.simulator
    rng = np.random.RandomState(0)
    valid, contacts = [], 0
    for _ in range(STEPS):
        env.step(rng.uniform(env.action_range[0], env.action_range[1], env.action_space.shape))
        w = te.contact_wrench()
        valid.append(float(np.mean([c['coverage'] for c in w])) if w else 0.0)
        contacts += sum(c['n_contacts'] for c in w)
    ns = sim.n_substeps
    f0 = sim.f_global_to_f_local(sim.cur_substep_global - ns)
    report(emit, f'{name} (n_grid {sim.n_grid}, collide_type {int(sim.engine.get_option("collide_type"))})', sim.engine, f0, ns, valid, contacts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default='(not given)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--only', default=None)
    args = ap.parse_args()
    lines = []

    def emit(text):
        lines.append(text)
        print(text, flush=True)
        if args.out:                                              # (kept as it grows: a scene that fails leaves the others' figures)
            with open(args.out, 'w') as fh:
                fh.write('\n'.join(lines) + '\n')
    emit(f'commit {args.commit}')
    emit('fe_contact_wrench, microseconds per call, wall clock, stream drained before and after: median (min .. max) of 30 after 5 warm-up calls')
    emit('coverage: substeps of the rollout whose grid is in the store (valid == 1), the only ones reported')
    for name in ('block', 'Mixing-v0', 'Pouring-v0', 'IceCreamDynamic-v0'):
        if args.only and args.only != name:
            continue
        try:
            block(emit) if name == 'block' else environment(emit, name)
        except Exception as ex:                                    # noqa: BLE001 -- a scene that cannot be built here is reported, not hidden
            emit(f'{name}: FAILED {type(ex).__name__}: {ex}')


if __name__ == '__main__':
    main()
