"""PouringLoss (fluidlab/fluidengine/losses/pouring_loss.py): keep the MILK where it started (L1 to the initial positions,
:131-135), pull the WATER towards the floor y = 0.05 ('default' only: dist_scale 0.2, :30-33) and, in the 'diff' variant, on
the last step attract the 100 WATER particles nearest to the lowest one towards it (:101-118, 137-146)."""
from fluidlab_amd.configs.macros import MILK, WATER
from .host_loss import HostLoss


class PouringLoss(HostLoss):
    temporal_range_type = 'all'

    def __init__(self, type, **kwargs):
        super().__init__(**kwargs)
        self.type = type
        assert type in ('diff', 'default')
        self.dist_scale = 0.0 if type == 'diff' else 0.2

    def build(self, sim):
        self.dist_weight = self.weights['dist']
        self.attraction_weight = self.weights['attraction']
        self.init_particle_pos = None
        super().build(sim)

    def _attraction(self, x, used, want_grad):
        """find_best_particle + compute_attraction_loss_kernel + scale_attraction_loss_kernel (:101-146)"""
        xp = self.xp
        water = used & (self.particle_mat == WATER)
        if xp.count(water) == 0:
            return 0.0, None
        loss = xp.abs(x[:, 1] - 0.05); loss[~water] = 1000
        best = x[xp.argmin(loss)] + 0.0                         # best_particle_pos is a constant copy (:108)
        dist = xp.norm_rows(x - best); dist[~water] = 1000
        near = water & (xp.rank(dist) < 100)
        scale = float(xp.count(water & (x[:, 1] > 0.55))) / 12500
        value = xp.to_float(xp.abs(x[near] - best).sum()) * 5000 * scale
        if not want_grad:
            return value, None
        g = xp.zeros_like(x)
        g[near] = xp.sign(x[near] - best) * 5000 * scale
        return value, g

    def step_value(self, s, f, x, used, want_grad):
        xp = self.xp
        if s == 0 and not want_grad:
            self.init_particle_pos = x + 0.0                     # get_init_particles, :97-99
        water = used & (self.particle_mat == WATER)
        milk = used & (self.particle_mat == MILK)
        dw, dm = x[water, 1] - 0.05, x[milk] - self.init_particle_pos[milk]
        value = (xp.to_float(xp.abs(dw).sum()) * self.dist_scale + xp.to_float(xp.abs(dm).sum())) * self.dist_weight
        g = None
        if want_grad:
            g = xp.zeros_like(x)
            g[water, 1] = xp.sign(dw) * self.dist_scale * self.dist_weight
            g[milk] = xp.sign(dm) * self.dist_weight
        if self.type == 'diff' and s == self.max_loss_steps - 1:
            av, ag = self._attraction(x, used, want_grad)
            value += av
            if ag is not None:
                g += ag
        # sum_up_loss_kernel adds the attraction WEIGHT as a constant (`+ self.attraction_weight`, :150): kept, it shifts the
        # reported loss by one per step and has no gradient
        value += self.attraction_weight
        return value, g

    def device_terms(self):
        from .term_program import AXIS_ALL, AXIS_Y, L1_CONST, L1_REF, Sel, Term
        N = self.n_particles
        return [Term(L1_CONST, AXIS_Y, Sel(0, N, WATER, True), c=(0.0, 0.05, 0.0), weight=self.dist_scale * self.dist_weight),
                Term(L1_REF, AXIS_ALL, Sel(0, N, MILK, True), weight=self.dist_weight)]

    def device_before_step(self, s, f):
        if s == 0:                                               # get_init_particles, :97-99
            self.engine.task_loss_set_ref(f)
            self.init_particle_pos = self.frame(f)[0] + 0.0

    def extra_step_value(self, s, f, want_grad):
        """the per-step constant and, for 'diff' on the last step, the attraction (argmin + the 100 nearest: not a term)"""
        value, g = self.attraction_weight, None
        if self.type == 'diff' and s == self.max_loss_steps - 1:
            av, g = self._attraction(*self.frame(f), want_grad)
            value += av
        return value, g

    def get_step_loss(self):
        cur = self.cur_step_loss()
        return {'reward': 0.001 * (5000 - cur), 'loss': 0.001 * cur}             # :196-202
