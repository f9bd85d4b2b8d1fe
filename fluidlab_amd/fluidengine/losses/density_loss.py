"""DensityMatchingLoss: squared distance between the density field of the matching material's used particles and a target field,
w * sum_c (D_c - T_c)^2 -- a shape objective that needs no recorded trajectory: the target is an array (a picture, a voxel grid) or a
point cloud of any resolution rasterised with the same weights (term_program.density_of_points).  The reference has no counterpart;
its shape losses all measure particle p against target['x'][s][p].

A HostLoss with a single DENSITY_SQ term.  The host path is the fp64 interpreter of the loss-term programs on a downloaded frame (it
works against the oracle too); enable_device_loss() uploads the field and the target and evaluates the term in the engine
(include/fluidengine_ext.h: fe_density_*, FE_TERM_DENSITY_SQ)."""
import numpy as np

from .host_loss import HostLoss
from .term_program import AXIS_ALL, DENSITY_SQ, DensityField, Sel, Term, density_of_points, eval_terms_numpy


class DensityMatchingLoss(HostLoss):
    field_id = 0

    def __init__(self, matching_mat, field, temporal_range_type='last', type=None, **kwargs):
        super().__init__(**kwargs)
        assert isinstance(field, DensityField), 'field: a term_program.DensityField'
        assert temporal_range_type in ('last', 'all'), temporal_range_type
        self.matching_mat = matching_mat
        self.field = field
        self.temporal_range_type = temporal_range_type
        self.target = None

    def build(self, sim):
        self.density_weight = self.weights['density']
        super().build(sim)
        self._mat_np = np.asarray(self.sim.particles_i.mat.to_numpy())

    def load_target(self, target):
        """target_file of the constructor: an array shaped like the field (there is no file format of its own)"""
        self.set_target_field(target)

    # ---- the target
    def set_target_field(self, array):
        """the target as an array with the field's cell count (shaped n, or flat in the order (i n1 + j) n2 + k)"""
        t = np.ascontiguousarray(array, np.float64)
        assert t.size == int(np.prod(self.field.shape)), f'the target has {t.size} values, the field {self.field.shape} cells'
        self.target = t.reshape(self.field.shape).copy()
        if self._device_loss:
            self.engine.density_set_target(self.field_id, self.target)

    def set_target_points(self, x):
        """the target as a point cloud x [M, 3] of any size, rasterised onto the field"""
        self.set_target_field(density_of_points(np.asarray(x, np.float64), self.field))

    # ---- the loss
    def device_terms(self):
        return [Term(DENSITY_SQ, AXIS_ALL, Sel(0, self.n_particles, self.matching_mat, True), weight=self.density_weight, field=self.field_id)]

    def step_value(self, s, f, x, used, want_grad):
        assert self.target is not None, 'no target: set_target_field / set_target_points first'
        if self.xp.name == 'torch':
            x, used = x.detach().cpu().numpy(), used.detach().cpu().numpy()
        vals, g = eval_terms_numpy(self.device_terms(), x, used, self._mat_np, None, want_grad,
                                   fields={self.field_id: self.field}, targets={self.field_id: self.target})
        return float(vals[0]), (self.xp.asarray(g) if want_grad else None)

    def enable_device_loss(self):
        self.engine.density_set_field(self.field_id, self.field)          # (raises on an oracle engine: HIP engine only)
        assert self.target is not None, 'no target: set_target_field / set_target_points first'
        self.engine.density_set_target(self.field_id, self.target)
        super().enable_device_loss()

    def get_step_loss(self):
        cur = self.cur_step_loss()
        return {'reward': -cur, 'loss': cur}
