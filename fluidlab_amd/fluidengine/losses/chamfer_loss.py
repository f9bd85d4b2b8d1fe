"""ChamferMatchingLoss: the Chamfer distance between the matching material's used particles and a target cloud without correspondence,
w_t * sum_p min_j |m.(x_p - t_j)|^2 + w_p * sum_j min_p |m.(t_j - x_p)|^2 -- every particle is pulled to its nearest target point and
every target point pulls its nearest particle, so a target that does not overlap the fluid still has a gradient (DensityMatchingLoss has
none there).  The reference has no counterpart: the kernel it calls "chamfer" (shapematching_loss.py:80) is index-to-index.

A HostLoss with one NEAREST_SQ and one COVER_SQ term.  The host path is the fp64 interpreter of the loss-term programs on a downloaded
frame (all pairs; it works against the oracle too); enable_device_loss() uploads the cloud and evaluates the two terms in the engine
(include/fluidengine_ext.h: fe_cloud_set, FE_TERM_NEAREST_SQ, FE_TERM_COVER_SQ)."""
import numpy as np

from .host_loss import HostLoss
from .term_program import AXIS_ALL, COVER_SQ, NEAREST_SQ, Sel, Term, cloud_point_ok, eval_terms_numpy


class ChamferMatchingLoss(HostLoss):
    cloud_id = 0

    def __init__(self, matching_mat, axis_mask=AXIS_ALL, temporal_range_type='last', type=None, **kwargs):
        super().__init__(**kwargs)
        assert temporal_range_type in ('last', 'all'), temporal_range_type
        assert 1 <= int(axis_mask) <= 7, axis_mask
        self.matching_mat = matching_mat
        self.axis_mask = int(axis_mask)
        self.temporal_range_type = temporal_range_type
        self.target = None

    def build(self, sim):
        self.to_target_weight = self.weights['to_target']
        self.to_particles_weight = self.weights['to_particles']
        super().build(sim)
        self._mat_np = np.asarray(self.sim.particles_i.mat.to_numpy())

    def load_target(self, target):
        """target_file of the constructor: an array of points [M, 3] (there is no file format of its own)"""
        self.set_target_points(target)

    def set_target_points(self, x):
        """the target cloud x [M, 3]: float32 words, every coordinate finite and within FE_CLOUD_COORD_MAX"""
        t = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
        assert len(t) > 0, 'the target cloud is empty'
        assert cloud_point_ok(t, AXIS_ALL).all(), 'the target cloud has a coordinate that is not finite or beyond FE_CLOUD_COORD_MAX'
        self.target = t.copy()
        if self._device_loss:
            self.engine.cloud_set(self.cloud_id, self.target)

    def device_terms(self):
        sel = Sel(0, self.n_particles, self.matching_mat, True)
        return [Term(NEAREST_SQ, self.axis_mask, sel, weight=self.to_target_weight, cloud=self.cloud_id, name='to_target'),
                Term(COVER_SQ, self.axis_mask, sel, weight=self.to_particles_weight, cloud=self.cloud_id, name='to_particles')]

    def step_value(self, s, f, x, used, want_grad):
        assert self.target is not None, 'no target: set_target_points first'
        if self.xp.name == 'torch':
            x, used = x.detach().cpu().numpy(), used.detach().cpu().numpy()
        vals, g = eval_terms_numpy(self.device_terms(), x, used, self._mat_np, None, want_grad, clouds={self.cloud_id: self.target})
        return float(vals.sum()), (self.xp.asarray(g) if want_grad else None)

    def enable_device_loss(self):
        assert self.target is not None, 'no target: set_target_points first'
        self.engine.cloud_set(self.cloud_id, self.target)               # (raises on an oracle engine: HIP engine only)
        super().enable_device_loss()

    def get_step_loss(self):
        cur = self.cur_step_loss()
        return {'reward': -cur, 'loss': cur}
