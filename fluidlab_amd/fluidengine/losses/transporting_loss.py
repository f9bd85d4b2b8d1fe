"""TransportingLoss (fluidlab/fluidengine/losses/transporting_loss.py): drive the RIGID_HEAVY cube towards x = 0.9 (L1 on
every particle of the cube, :88-91) and, in the 'diff' variant, attract the used WATER particles to it -- 1e-4 times the L1
distance of every (water, cube) particle pair (:94-99), summed here without forming the pairs (host_loss.pairwise_l1)."""
import numpy as np

from fluidlab_amd.configs.macros import RIGID_HEAVY, WATER
from .host_loss import HostLoss, pairwise_l1


class TransportingLoss(HostLoss):
    temporal_range_type = 'all'               # the reference overrides its own 'expand' setting (:33-34)

    def __init__(self, type, **kwargs):
        super().__init__(**kwargs)
        assert type in ('diff', 'default')
        self.type = type

    def build(self, sim):
        self.dist_weight = self.weights['dist']
        self._dist = np.zeros((self.max_loss_steps,), np.float64)
        self._attraction = np.zeros((self.max_loss_steps,), np.float64)
        super().build(sim)
        mat = self.particle_mat
        self.n_particles_water = self.xp.count(mat == WATER)         # the water pool comes first (transporting_env.py:47-52)
        self.obj_start = self.n_particles_water
        self.obj_end = self.obj_start + self.xp.count(mat == RIGID_HEAVY)

    def clear_loss(self):
        super().clear_loss()
        if hasattr(self, '_dist'):
            self._dist[:] = 0; self._attraction[:] = 0

    def step_value(self, s, f, x, used, want_grad):
        xp = self.xp
        obj = x[self.obj_start:self.obj_end]
        dist = xp.to_float(xp.abs(obj[:, 0] - 0.9).sum())
        g = xp.zeros_like(x) if want_grad else None
        if want_grad:
            g[self.obj_start:self.obj_end, 0] = xp.sign(obj[:, 0] - 0.9) * self.dist_weight
        attraction = 0.0
        if self.type == 'diff':
            w = xp.where(used[:self.n_particles_water])
            attraction, gw, gobj = pairwise_l1(x[w], obj, xp=xp)
            attraction *= 1e-4
            if want_grad:
                g[w] += gw * 1e-4
                g[self.obj_start:self.obj_end] += gobj * 1e-4
        if not want_grad:
            self._dist[s] += dist; self._attraction[s] += attraction
        return dist * self.dist_weight + attraction, g

    def device_terms(self):
        from .term_program import AXIS_ALL, AXIS_X, L1_CONST, PAIR_L1, Sel, Term
        cube = Sel(self.obj_start, self.obj_end)
        terms = [Term(L1_CONST, AXIS_X, cube, c=(0.9, 0.0, 0.0), weight=self.dist_weight)]
        if self.type == 'diff':
            terms.append(Term(PAIR_L1, AXIS_ALL, Sel(0, self.n_particles_water, -1, True), cube, weight=1e-4))
        return terms

    def final_loss_info(self):
        if self._device_loss:                                    # _dist is the unweighted sum: term 0 is dist_weight times it
            tl = self.device_term_loss()
            dist = float(tl[0].sum()) / self.dist_weight if self.dist_weight != 0 else 0.0
            return {'dist_loss': dist, 'attraction_loss': float(tl[1].sum()) if len(tl) > 1 else 0.0}
        return {'dist_loss': float(self._dist.sum()), 'attraction_loss': float(self._attraction.sum())}

    def get_step_loss(self):
        cur = self.cur_step_loss()
        return {'reward': 0.05 * (135 - cur), 'loss': cur}                 # :149-156
