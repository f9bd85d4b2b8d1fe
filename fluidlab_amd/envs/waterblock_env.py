"""WaterBlock-v0 -- BASELINE config 2: a single-material water block, no agent.
Not a reference env; it is the scene the headline metric is quoted on, packaged like one."""
import numpy as np

from fluidlab_amd.configs.macros import WATER
from fluidlab_amd.fluidengine.taichi_env import TaichiEnv
from .fluid_env import FluidEnv


class WaterBlockEnv(FluidEnv):
    def __init__(self, version=0, loss=False, loss_type='diff', seed=None, renderer_type=None, quality=2, n_particles=200000,
                 horizon=100, max_substeps_local=None, engine_lib=None, device=0):
        if seed is not None:
            self.seed(seed)
        self.horizon = self.horizon_action = horizon
        self.target_file = None
        self._n_obs_ptcls_per_body = 200
        self.loss = loss
        self.loss_type = loss_type
        self.renderer_type = renderer_type            # (the reference has no such environment: 'HIP' takes FluidEnv.setup_renderer's default camera and lights)
        self.action_range = np.array([-1.0, 1.0])
        lo, hi = 0.30, 0.53
        self._box = (lo, hi)
        self.taichi_env = TaichiEnv(dim=3, quality=quality, particle_density=n_particles / (hi - lo) ** 3,
                                    max_substeps_local=max_substeps_local, gravity=(0.0, -10.0, 0.0), horizon=horizon,
                                    engine_lib=engine_lib, device=device)
        self.build_env()
        self.gym_misc()

    def setup_bodies(self):
        lo, hi = self._box
        self.taichi_env.add_body(type='cube', lower=(lo, lo, lo), upper=(hi, hi, hi), material=WATER)

    def setup_boundary(self):
        self.taichi_env.setup_boundary(type='cube', lower=(0.05, 0.05, 0.05), upper=(0.95, 0.95, 0.95))

    def _get_reward(self):
        return 0.0
