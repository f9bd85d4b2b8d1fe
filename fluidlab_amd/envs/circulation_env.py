"""Circulation-v0 -- indoor air circulation (fluidlab/envs/circulation_env.py): an AirCon steers a smoke / temperature
field through a room; the loss reads the temperature at fifteen detector cells.

The room (`room.obj` in the reference) is needed as an SDF and mesh -> SDF conversion is not available here
(fluidengine/meshes.py), so it is an analytic stand-in in the same pose: outer walls plus two partition walls that leave
doorways.  `res`, `horizon`, `solver_iters`, `max_substeps_local` scale the scene for tests; the defaults are the
reference's (128^3 smoke grid, 50 Jacobi sweeps, 1000 steps, checkpoint window of 100 substeps on the host)."""
import numpy as np

from fluidlab_amd.configs.macros import PILLAR, WATER
from fluidlab_amd.fluidengine.losses import CirculationLoss
from fluidlab_amd.fluidengine.taichi_env import TaichiEnv
from fluidlab_amd.optimizer.policies import ActionsPolicy, CirculationPolicy
from fluidlab_amd.utils.config import CfgNode
from fluidlab_amd.utils.misc import get_cfg_path
from .fluid_env import FluidEnv


ROOM_SCALE = np.array([1.4, 3.0, 1.4])          # circulation_env.py's add_static(room.obj, scale=...), about (0.5, 0.5, 0.5)


def sdf_room():
    """Stand-in for room.obj, after the floor plan of the reference's mesh (mapped with fe_mesh_sdf on the asset): the free space
    is x in [0.05, 0.95], z in [0.22, 0.80] over the whole height, split into four rooms -- a wall at x = 0.38 with doorways at
    z in [0.29, 0.38] and [0.59, 0.71], a wall at z = 0.49 between the two rooms on its low-x side, and a wall at x = 0.68 with a
    doorway at z in [0.41, 0.56].  Written in world coordinates, returned in the mesh frame the SDF lattice samples (distances
    divided by the xz scale; only sign and direction matter to the colliders)."""
    def box(w, lo, hi):
        c, h = (np.asarray(lo) + np.asarray(hi)) / 2, (np.asarray(hi) - np.asarray(lo)) / 2
        q = np.abs(w - c) - h
        return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(axis=1), 0)

    walls = [((0.36, -1, 0.22), (0.40, 2, 0.29)), ((0.36, -1, 0.38), (0.40, 2, 0.59)), ((0.36, -1, 0.71), (0.40, 2, 0.80)),
             ((0.05, -1, 0.47), (0.38, 2, 0.51)),
             ((0.66, -1, 0.22), (0.70, 2, 0.41)), ((0.66, -1, 0.56), (0.70, 2, 0.80))]

    def fn(p):
        w = p * ROOM_SCALE + 0.5
        d = -box(w, (0.05, -1, 0.22), (0.95, 3, 0.80))              # solid outside the free space; open at the top (the lattice ends at y = 2.3):
                                                                    # the room can be looked into from above, and the slab at y = 0.5 is as it was
        for lo, hi in walls:
            d = np.minimum(d, box(w, lo, hi))
        return d / ROOM_SCALE[0]
    return fn


class CirculationEnv(FluidEnv):
    def __init__(self, version=0, loss=True, loss_type='diff', seed=None, renderer_type=None, res=128, horizon=1000, solver_iters=50,
                 max_substeps_local=100, ckpt_dest='cpu', detectors=None, engine_lib=None, device=0):
        if seed is not None:
            self.seed(seed)
        self.horizon = horizon
        self.horizon_action = horizon
        self.target_file = None
        self._n_obs_ptcls_per_body = 200
        self.loss = loss
        self.loss_type = loss_type
        self.renderer_type = renderer_type
        self.action_range = np.array([-0.1, 0.1])
        self._res, self._iters, self._detectors = res, solver_iters, detectors
        self.taichi_env = TaichiEnv(dim=3, particle_density=1e6, max_substeps_local=max_substeps_local, gravity=(0.0, -20.0, 0.0),
                                    horizon=self.horizon, ckpt_dest=ckpt_dest, engine_lib=engine_lib, device=device)
        self.build_env()
        self.gym_misc()

    def setup_renderer(self):
        """renderer_type='HIP': camera and lights of the reference's GGUI renderer for this scene (circulation_env.py:83-92, the GGUI block it keeps commented out)"""
        self.taichi_env.setup_renderer(type=self.renderer_type, res=(1280, 1280), camera_pos=(0.5, 12.0, 0.501), camera_lookat=(0.5, 0.5, 0.5), fov=8,
                                       lights=[{'pos': (0.5, 1.5, 0.5), 'color': (0.5, 0.5, 0.5)}, {'pos': (0.5, 1.5, 1.5), 'color': (0.5, 0.5, 0.5)}])

    def setup_agent(self):
        agent_cfg = CfgNode()
        agent_cfg.merge_from_file(get_cfg_path('agent_circulation.yaml'))
        self.taichi_env.setup_agent(agent_cfg)
        self.agent = self.taichi_env.agent

    def setup_statics(self):
        self.taichi_env.add_static(file='room.obj', pos=(0.5, 0.5, 0.5), euler=(0.0, 0.0, 0.0), scale=(1.4, 3.0, 1.4), material=PILLAR,
                                   sdf_res=min(128, self._res), has_dynamics=True, sdf=sdf_room())

    def setup_bodies(self):
        self.taichi_env.add_body(type='nowhere', n_particles=10, material=WATER)

    def setup_smoke_field(self):
        self.taichi_env.setup_smoke_field(res=self._res, dt=0.03, solver_iters=self._iters, decay=0.99, q_dim=1)
        if self._res != 128:                      # the free slab 60 < j < 68 (smoke_field.py:25-26) scaled with the grid
            sf = self.taichi_env.smoke_field
            sf.lower_y, sf.higher_y = int(round(60 * self._res / 128)), int(round(68 * self._res / 128))

    def setup_boundary(self):
        pass

    def setup_loss(self):
        self.taichi_env.setup_loss(loss_cls=CirculationLoss, type=self.loss_type, weights={'temp': 1.0}, detectors=self._detectors)

    OBS_LIST = 0                                                    # the engine cell list of the observation lattice (1: CirculationLoss's detectors)

    def enable_device_obs(self):
        """From here on _get_obs() reads only the lattice cells [::10, lower_y:higher_y, ::10] of v and q, gathered on the GPU (engine cell
        list), instead of downloading v, v_tmp, div, p and q whole.  The observation vector is the same.  HIP engine only."""
        self.taichi_env.smoke_field.set_cells(self.OBS_LIST, self._obs_cells())
        self._device_obs = True

    def enable_field_obs(self, fields, particles=True):
        raise RuntimeError('enable_field_obs: Circulation has no particles to observe (its ten are parked); its observation is the smoke field (enable_device_obs)')

    def _obs_cells(self):
        """the observation lattice as cells [n, 3], in the C order of [i][j][k]: the order .flatten() gives the slices of _get_obs"""
        sf = self.taichi_env.smoke_field
        n = sf.n_grid
        lattice = np.stack(np.meshgrid(np.arange(0, n, 10), np.arange(sf.lower_y, sf.higher_y), np.arange(0, n, 10), indexing='ij'), axis=-1)
        return lattice.reshape(-1, 3).astype(np.int32)

    def _diagnostics_record(self):
        """the smoke field is what Circulation simulates (its ten particles are parked): report its summary"""
        rec = self.taichi_env.smoke_summary()
        out = {k: rec[k] for k in ('courant', 'kinetic', 'n_nonfinite', 'q_min', 'q_max')}
        # The solver samples the grid's edge for a back-trace that is not finite (fe_smoke_index.h), so a step can swallow the non-finite
        # cells it was given instead of spreading them: the count covers the frame the step consumed as well.
        sim = self.taichi_env.simulator
        cur = sim.cur_step_local
        out['n_nonfinite'] += self.taichi_env.smoke_summary(cur - 1 if cur > 0 else sim.max_steps_local - 1)['n_nonfinite']
        return out

    def _get_obs(self):
        if self._device_obs:
            sim = self.taichi_env.simulator
            obs = [self.agent.get_state(sim.cur_substep_local)[0].flatten()] if self.agent is not None else []
            rows = self.taichi_env.smoke_field.cells_at(sim.cur_step_local, self.OBS_LIST)
            return np.concatenate(obs + [rows['v'].flatten(), rows['q'].flatten()])
        state = self.taichi_env.get_state_RL()
        obs = [state['agent'][0].flatten()] if 'agent' in state else []
        if 'smoke_field' in state:                                  # fluid_env.py:120-122
            sf = self.taichi_env.smoke_field
            obs.append(state['smoke_field']['v'][::10, sf.lower_y:sf.higher_y, ::10].flatten())
            obs.append(state['smoke_field']['q'][::10, sf.lower_y:sf.higher_y, ::10].flatten())
        return np.concatenate(obs)

    # ---- closed-loop policies (optimizer/closed_loop.py): the vector's layout, its device form and its cotangent
    def obs_layout(self):
        """The slices of the vector _get_obs() builds: 'bodies' is empty (the ten parked particles are not observed), 'agent' / 'extra' as in
        FluidEnv.obs_layout (the AirCon's pose; its s and r), 'smoke' = {'v', 'q': slices of the lattice's rows, 'cells': the lattice
        [n, 3], 'list': the engine cell list enable_device_obs() registers it as}, 'size'."""
        te = self.taichi_env
        at, agent, extra = 0, [], []
        for e in (te.agent.effectors if te.agent is not None else []):
            agent.append(slice(at, at + 7))
            extra.append(slice(at + 7, at + e.state_dim) if e.state_dim > 7 else None)
            at += e.state_dim
        cells, qd = self._obs_cells(), te.smoke_field.q_dim
        n = len(cells)
        smoke = dict(v=slice(at, at + 3 * n), q=slice(at + 3 * n, at + (3 + qd) * n), cells=cells, list=self.OBS_LIST)
        return dict(bodies=[], agent=agent, extra=extra, smoke=smoke, size=at + (3 + qd) * n)

    def _device_road(self):
        eng = self.taichi_env.simulator.engine
        return bool(self._device_obs) and eng.elib.backend.startswith('hip') and eng.elib.has_ext

    def observe_dev(self):
        """the observation of the current frame as a float32 torch tensor on the engine's GPU, from one launch (fe_smoke_obs_get_dev); needs
        enable_device_obs()"""
        import torch
        assert self._device_road(), 'observe_dev: enable_device_obs() on the HIP engine first'
        te = self.taichi_env
        sim, eng = te.simulator, te.simulator.engine
        out = torch.empty((eng.smoke_obs_size(self.OBS_LIST),), dtype=torch.float32, device=torch.device('cuda', eng.device))
        te.smoke_field.obs_at(sim.cur_step_local, self.OBS_LIST, self.agent.effectors[0], sim.cur_substep_local, out=out)
        eng.sync()                                               # (the entry enqueues on the engine's stream; torch reads the tensor on its own)
        return out

    def obs_backward(self, g_obs, f=None):
        """Route the cotangent of an observation vector into the simulation: the v / q slices are added to the smoke adjoint of frame
        s = f // n_substeps at the lattice cells, the pose slice to the AirCon's state adjoint of local frame f (default: the current
        frame), the s / r entries to its strength / radius adjoints.  With enable_device_obs() on the HIP engine that is one engine call
        (a torch tensor on the engine's GPU does not leave it).  Otherwise dense fields are built on the host and handed to
        fe_smoke_add_grad, which every engine has; an engine without the extension has no entry for the pose, s and r adjoints: a non-zero
        cotangent there raises."""
        te = self.taichi_env
        sim, sf = te.simulator, te.smoke_field
        eng = sim.engine
        f = sim.cur_substep_local if f is None else int(f)
        s = f // sim.n_substeps
        layout = self.obs_layout()
        assert len(layout['agent']) == 1, 'Circulation observes one AirCon'
        g = g_obs.detach().reshape(-1) if hasattr(g_obs, 'detach') else np.asarray(g_obs).reshape(-1)
        assert g.shape[0] == layout['size'], f"obs_backward: the cotangent has {g.shape[0]} entries, the observation {layout['size']}"
        aircon = self.agent.effectors[0]
        if self._device_road():
            if getattr(g, 'is_cuda', False):
                import torch
                g = g.to(torch.float32).contiguous()
            else:
                g = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)
            sf.add_obs_grad(s, self.OBS_LIST, aircon, f, g)
            return
        g = np.asarray(g.cpu() if hasattr(g, 'cpu') else g)
        g_pose, g_sr = np.array(g[layout['agent'][0]]), np.array(g[layout['extra'][0]])
        if np.any(g_pose != 0) or np.any(g_sr != 0):             # (the oracle ABI has no such entry: only a zero cotangent can be dropped -- refused before anything is added)
            eng._need_ext("the adjoints of an AirCon's pose, strength and radius")
        sm = layout['smoke']
        c, qd = sm['cells'], sf.q_dim
        gv, gq = np.zeros((*sf.res, 3), eng.dtype), np.zeros((*sf.res, qd), eng.dtype)
        np.add.at(gv, (c[:, 0], c[:, 1], c[:, 2]), g[sm['v']].reshape(-1, 3).astype(eng.dtype))
        np.add.at(gq, (c[:, 0], c[:, 1], c[:, 2]), g[sm['q']].reshape(-1, qd).astype(eng.dtype))
        eng.smoke_add_grad(s, gv=gv, gq=gq)
        if eng.elib.has_ext:
            aircon.add_state_grad(f, g_pose)
            aircon.add_sr_grad(f, g_sr[0], g_sr[1])

    def action_bounds(self):
        """What a closed-loop policy may command, after trainable_policy's fix_dim: the seven fixed entries are the demo's row (strength 0.02,
        radius 0.04, the rest 0) with lo == hi, entry 4 (the yaw rate) keeps action_range.  The radius cannot be <= 0: the impulse is
        exp(-dist / r)."""
        lo, hi = np.zeros((self.agent.action_dim,)), np.zeros((self.agent.action_dim,))
        lo[6] = hi[6] = 0.02
        lo[7] = hi[7] = 0.04
        lo[4], hi[4] = float(self.action_range[0]), float(self.action_range[1])
        return lo, hi

    def demo_policy(self):
        comp_actions_p = np.zeros((1, self.agent.action_dim))
        comp_actions_v = np.zeros((self.horizon_action, self.agent.action_dim))
        comp_actions_p[0] = np.array([0.55, 0.5, 0.27, 0.0, 0.0, 0.0, 0.0, 0.0])
        comp_actions_v[:] = np.array([0.0, 0.0, 0.0, 0.0, 0.1, 0.0, 0.02, 0.04])
        return ActionsPolicy(np.vstack([comp_actions_v, comp_actions_p]))

    def trainable_policy(self, optim_cfg, init_range):
        return CirculationPolicy(optim_cfg, init_range, self.agent.action_dim, self.horizon_action, self.action_range,
                                 fix_dim=[0, 1, 2, 3, 5, 6, 7])
