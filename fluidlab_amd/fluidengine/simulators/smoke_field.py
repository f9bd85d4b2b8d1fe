"""SmokeField -- the Eulerian smoke / temperature solver of Circulation-v0 (fluidlab/fluidengine/simulators/smoke_field.py).

Every Taichi kernel of the reference (compute_free_space, advect_and_impulse, divergence, pressure_jacobi x solver_iters,
subtract_gradient and the adjoints Taichi derives from them) lives in the engine (fluidlab_amd/csrc/fe_smoke.h); this
class keeps the reference's method surface and its state / checkpoint dict layouts.  colorize() and the vis_particles
fields feed the renderer only and have no counterpart."""
import numpy as np


class SmokeField:
    def __init__(self, dim, ckpt_dest, res=128, dt=0.03, solver_iters=500, q_dim=3, decay=0.99):
        self.dim = dim
        self.ckpt_dest = ckpt_dest
        self.n_grid = res
        self.dx = 1 / self.n_grid
        self.res = (res,) * self.dim
        self.dt = dt
        self.solver_iters = solver_iters
        self.q_dim = q_dim
        self.decay = decay
        self.high_T = 1.0
        self.low_T = 0.0
        self.lower_y = 60                 # smoke_field.py:25-26: the free slab, in cells of a 128^3 grid
        self.higher_y = 68
        print(f'===>  Smoke field of {self.res} initialized.')

    def build(self, mpm_sim, agent):
        self.mpm_sim = mpm_sim
        self.max_steps_local = mpm_sim.max_steps_local
        self.agent = mpm_sim.agent
        self.engine = mpm_sim.engine
        self.engine.smoke_create(res=self.n_grid, dt=self.dt, solver_iters=self.solver_iters, q_dim=self.q_dim, decay=self.decay,
                                 max_steps_local=self.max_steps_local, high_T=self.high_T, low_T=self.low_T,
                                 lower_y=self.lower_y, higher_y=self.higher_y)
        if self.ckpt_dest in ('cpu', 'gpu'):
            self.ckpt_ram = dict()

    # ---- stepping (smoke_field.py:95-128)
    def step(self, s, f):
        self.engine.smoke_step(s, f)

    def step_grad(self, s, f):
        self.engine.smoke_step_grad(s, f)

    # ---- frames and adjoints (145-171)
    def copy_frame(self, source, target):
        self.engine.smoke_copy_frame(source, target)

    def copy_grad(self, source, target):
        self.engine.smoke_copy_grad(source, target)

    def reset_grad(self):
        self.engine.smoke_reset_grad()

    def reset_grad_till_frame(self, s):
        self.engine.smoke_reset_grad_till_frame(s)

    # ---- state / checkpoints (384-439): dicts of v, v_tmp, div, p, q
    FIELDS = ('v', 'v_tmp', 'div', 'p', 'q')

    def get_state(self, s):
        return self.engine.smoke_get_frame(s, self.FIELDS)

    def set_state(self, s, state):
        self.engine.smoke_set_frame(s, **{k: state[k] for k in self.FIELDS})

    def get_ckpt(self, ckpt_name=None):
        ckpt = self.get_state(0)
        if self.ckpt_dest in ('cpu', 'gpu'):
            self.ckpt_ram[ckpt_name] = ckpt
        return ckpt

    def set_ckpt(self, ckpt=None, ckpt_name=None):
        if self.ckpt_dest in ('cpu', 'gpu') and ckpt is None:
            ckpt = self.ckpt_ram[ckpt_name]
        self.set_state(0, ckpt)

    # ---- what CirculationLoss reads / seeds (circulation_loss.py:99-105): the temperature q[...,0] at a few cells
    def q_at(self, s, cells):
        q = self.engine.smoke_get_frame(s, ('q',))['q']
        c = np.asarray(cells)
        return q[c[:, 0], c[:, 1], c[:, 2], 0].astype(np.float64)

    def add_q_grad_at(self, s, cells, grads):
        gq = np.zeros((*self.res, self.q_dim), self.engine.dtype)
        c = np.asarray(cells)
        np.add.at(gq, (c[:, 0], c[:, 1], c[:, 2], 0), np.asarray(grads))
        self.engine.smoke_add_grad(s, gq=gq)

    # ---- reads that stay on the GPU (include/fluidengine_ext.h: fe_smoke_cells_*, fe_smoke_summary; HIP engine only)
    def set_cells(self, list_id, cells):
        """register cells [n,3] of (i, j, k) as cell list `list_id`; None removes it"""
        self.engine.smoke_cells_set(list_id, cells)

    def cells_at(self, s, list_id):
        """{'v' [n,3], 'q' [n,q_dim]} of the listed cells in frame s, gathered on the device: n rows cross PCIe, not the fields"""
        return self.engine.smoke_cells_get(list_id, s)

    def add_grad_at_cells(self, s, list_id, gv=None, gq=None):
        """the adjoint of cells_at: rows gv [n,3] / gq [n,q_dim] added to the v / q adjoint of frame s at the listed cells (None = skip);
        numpy arrays or float32 torch tensors on the engine's GPU, which stay there"""
        self.engine.smoke_cells_add_grad(list_id, s, gv=gv, gq=gq)

    def obs_at(self, s, list_id, effector, f, out=None):
        """Circulation's observation vector from one launch: the AirCon's state at local frame f (pos, quat, s, r), then the v rows and the q
        rows of the listed cells in frame s.  out=None: a numpy array; a float32 torch tensor on the engine's GPU is filled there and returned."""
        return self.engine.smoke_obs_get(list_id, s, effector.index, f, out=out)

    def add_obs_grad(self, s, list_id, effector, f, g):
        """the adjoint of obs_at in one launch: g laid out like the vector (numpy, or a float32 torch tensor on the engine's GPU, which stays there)"""
        self.engine.smoke_obs_add_grad(list_id, s, effector.index, f, g)

    def summary(self, s=None):
        """Diagnostics of frame s (default: the current step's) over the free slab, reduced on the device in fp64: cell and non-finite
        counts, v_max, Courant number, kinetic energy, sum and range of q (fields of FeSmokeSummary)."""
        return self.engine.smoke_summary(self.mpm_sim.cur_step_local if s is None else s)
