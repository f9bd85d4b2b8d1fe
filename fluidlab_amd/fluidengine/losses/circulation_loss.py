"""CirculationLoss -- room-temperature objective of Circulation-v0 (fluidlab/fluidengine/losses/circulation_loss.py):
|T - 1| at five detector cells, |T - target_temp| at ten others, every step (circulation_loss.py:97-109).  Fifteen cells
per step: the reduction and its adjoint run on the host; the temperature field and its adjoint stay in the engine."""
import numpy as np

from .loss import Loss


class CirculationLoss(Loss):
    def __init__(self, type, detectors=None, **kwargs):
        super().__init__(**kwargs)
        self.plateau_count_limit = 10
        self.temporal_expand_speed = 0
        self.temporal_init_range_end = 0
        self.temporal_range_type = 'all'
        self.plateau_thresh = [1e-6, 0.1]
        self._detectors = detectors

    def build(self, sim):
        self.temp_weight = self.weights['temp']
        self.temporal_range = [0, self.max_loss_steps]                                   # 'all' (circulation_loss.py:33-41)
        self.target_temp = 0.0
        self.detector_h = 64
        h = self.detector_h
        default = [[25, h, 85], [35, h, 85], [15, h, 85], [25, h, 75], [25, h, 95],      # circulation_loss.py:46-65
                   [25, h, 42], [35, h, 42], [15, h, 42], [25, h, 32], [25, h, 52],
                   [107, h, 65], [115, h, 65], [99, h, 65], [107, h, 45], [107, h, 85]]
        self.detector_array = np.asarray(default if self._detectors is None else self._detectors, np.int32)
        self.detector_array_N = len(self.detector_array)
        self.smoke_field = sim.smoke_field                                               # loss.py:41-42
        self.temp_loss = np.zeros((self.max_loss_steps,), np.float64)
        self._step_loss = np.zeros((self.max_loss_steps,), np.float64)
        self.total_loss = 0.0
        super().build(sim)

    _device_loss = False                                  # enable_device_loss(): the detector sum and its adjoint run in the engine
    DETECTOR_LIST = 1                                     # the engine cell list the detectors are registered as (0: CirculationEnv's observation lattice)

    # _step_loss / temp_loss: the host arrays -- or, with the device loss on, the engine's step_loss (read lazily, cached until the next loss
    # call) and that divided by the weight
    @property
    def _step_loss(self):
        if not self._device_loss:
            return self._step_loss_host
        if self._dev_cache is None:
            self._dev_cache = self.engine.smoke_loss_get(self.max_loss_steps)
        return self._dev_cache

    @_step_loss.setter
    def _step_loss(self, a):
        self._step_loss_host = a

    @property
    def temp_loss(self):
        if not self._device_loss:
            return self._temp_loss_host
        return self._step_loss / self.temp_weight if self.temp_weight != 0 else np.zeros((self.max_loss_steps,), np.float64)

    @temp_loss.setter
    def temp_loss(self, a):
        self._temp_loss_host = a

    @property
    def step_loss(self):
        return self._step_loss

    def clear_loss(self):
        super().clear_loss()
        if hasattr(self, '_step_loss_host'):
            self._step_loss_host[:] = 0
            self.total_loss = 0.0
        if self._device_loss:
            self.engine.smoke_loss_clear()
            self._send_detectors()                        # (a changed target_temp takes effect here)
            self._dev_cache = None

    def clear_losses(self):
        if hasattr(self, '_temp_loss_host'):
            self._temp_loss_host[:] = 0

    def _targets(self):
        t = np.full(self.detector_array_N, self.target_temp)
        t[:5] = 1.0
        return t

    # ---- the loss in the engine (include/fluidengine_ext.h: fe_smoke_loss_*; HIP engine only)
    def _send_detectors(self):
        self.engine.smoke_loss_set(self.DETECTOR_LIST, self._targets(), weight=self.temp_weight)

    def enable_device_loss(self):
        """From here on step() / step_grad() evaluate the detector sum and add its adjoint in the engine (fe_smoke_loss_step / _step_grad): no
        field crosses PCIe, nothing waits per step; step_loss is read from the device when asked for.  Call after build()."""
        self.engine.smoke_loss_alloc(self.max_loss_steps)         # (raises on an oracle engine: HIP engine only)
        self.smoke_field.set_cells(self.DETECTOR_LIST, self.detector_array)
        self._dev_cache = None
        self._device_loss = True
        self.clear_loss()                                         # (sends targets and weight)

    def step(self):
        """circulation_loss.py:77-79: loss of step cur_step_global - 1, read at local step frame cur_step_local"""
        s_global, s_local = self.sim.cur_step_global - 1, self.sim.cur_step_local
        if self._device_loss:
            self._dev_cache = None
            self.engine.smoke_loss_step(s_global, s_local)
            return
        q = self.smoke_field.q_at(s_local, self.detector_array)
        self.temp_loss[s_global] += np.abs(q - self._targets()).sum()
        self._step_loss[s_global] += self.temp_loss[s_global] * self.temp_weight

    def step_grad(self):
        s_global, s_local = self.sim.cur_step_global - 1, self.sim.cur_step_local
        if not (self.temporal_range[0] <= s_global < self.temporal_range[1]):
            return
        if self._device_loss:
            self.engine.smoke_loss_step_grad(s_global, s_local, self.total_loss_grad)
            return
        q = self.smoke_field.q_at(s_local, self.detector_array)
        g = np.sign(q - self._targets()) * self.temp_weight * self.total_loss_grad       # d|.| = sign (0 at the kink, as Taichi)
        self.smoke_field.add_q_grad_at(s_local, self.detector_array, g)

    def get_final_loss(self):
        self.total_loss = float(self._step_loss[self.temporal_range[0]:self.temporal_range[1]].sum())
        # temporal_range_type is 'all' (circulation_loss.py:25): expand_temporal_range has nothing to expand
        return {'loss': self.total_loss, 'last_step_loss': float(self._step_loss[self.max_loss_steps - 1]),
                'temporal_range': self.temporal_range[1]}

    def get_final_loss_grad(self):
        pass                                            # step_loss.grad[s] = total_loss.grad for s in the range: applied in step_grad

    def get_step_loss(self):
        cur = float(self._step_loss[self.sim.cur_step_global - 1])
        return {'reward': 1.0 * (11 - cur), 'loss': 1.0 * cur}
