"""MixingLoss (fluidlab/fluidengine/losses/mixing_loss.py): spread the milk -- minus 1e-4 times the L1 distance over all
ordered pairs of the first tenth of the MILK_VIS particles (:47, 72-75; no `used` test), summed without forming the pairs."""
from fluidlab_amd.configs.macros import MILK_VIS
from .host_loss import HostLoss, pairwise_l1


class MixingLoss(HostLoss):
    temporal_range_type = 'all'
    plateau_count_limit = 5
    temporal_expand_speed = 80
    temporal_init_range_end = 80

    def __init__(self, type, **kwargs):
        super().__init__(**kwargs)
        assert type in ('diff', 'default')

    def build(self, sim):
        self.dist_weight = self.weights['dist']
        super().build(sim)
        self.n_particles_milk = int(self.xp.count(self.particle_mat == MILK_VIS) * 0.1)

    def step_value(self, s, f, x, used, want_grad):
        total, ga, _ = pairwise_l1(x[:self.n_particles_milk], xp=self.xp)
        g = None
        if want_grad:
            g = self.xp.zeros_like(x)
            g[:self.n_particles_milk] = -1e-4 * self.dist_weight * ga
        return -1e-4 * total * self.dist_weight, g

    def device_terms(self):
        from .term_program import AXIS_ALL, PAIR_L1, Sel, Term
        return [Term(PAIR_L1, AXIS_ALL, Sel(0, self.n_particles_milk), None, weight=-1e-4 * self.dist_weight)]

    def get_step_loss(self):
        cur = self.cur_step_loss()
        return {'reward': 0.1 * (-cur - 41), 'loss': cur}                   # :121-129
