"""Recorder -- rolls out the demo policy and stores the particle trajectory as the loss target
(fluidlab/optimizer/recorder.py); also replays a stored policy.  With `frames_dir` set (off by default) and a renderer in the
environment (renderer_type='HIP') every recorded or replayed step is also written as a PNG, the reference's image output -- drawn as the
environment draws it: with the scene after enable_scene_render(), with the liquid surface after enable_liquid_surface()."""
import os
import pickle as pkl


class Recorder:
    def __init__(self, env, frames_dir=None):
        self.env = env
        self.frames_dir = frames_dir
        if frames_dir is not None:
            if env.taichi_env.renderer is None:
                raise RuntimeError("Recorder(frames_dir=...): the environment has no renderer (make it with renderer_type='HIP')")
            os.makedirs(frames_dir, exist_ok=True)
        self.target_file = env.target_file
        if self.target_file is not None:
            os.makedirs(os.path.dirname(self.target_file), exist_ok=True)

    def _write_frame(self, i):
        if self.frames_dir is not None:
            from fluidlab_amd.utils.image import write_png
            write_png(os.path.join(self.frames_dir, f'{i:04d}.png'), self.env.taichi_env.render('rgb_array'))

    def record(self, user_input=False, write=True):
        policy = self.env.demo_policy(user_input)
        taichi_env = self.env.taichi_env
        init = taichi_env.get_state()
        target = {'x': [], 'used': [], 'mat': None}
        taichi_env.set_state(**init)
        action_p = policy.get_actions_p()
        if action_p is not None:
            taichi_env.apply_agent_action_p(action_p)
        for i in range(self.env.horizon):
            action = policy.get_action_v(i) if i < self.env.horizon_action else None
            taichi_env.step(action)
            self._write_frame(i)
            if taichi_env.has_particles:
                cur = taichi_env.get_state()['state']
                target['x'].append(cur['x'])
                target['used'].append(cur['used'])
        target['mat'] = taichi_env.simulator.particles_i.mat.to_numpy()
        if write and self.target_file is not None:
            if os.path.exists(self.target_file):
                os.remove(self.target_file)
            with open(self.target_file, 'wb') as fh:
                pkl.dump(target, fh)
            print(f'===> New target generated and dumped to {self.target_file}.')
        return target

    def replay_policy(self, policy_path):
        taichi_env = self.env.taichi_env
        with open(policy_path, 'rb') as fh:
            policy = pkl.load(fh)
        taichi_env.apply_agent_action_p(policy.get_actions_p())
        for i in range(self.env.horizon):
            action = policy.get_action_v(i, agent=taichi_env.agent, update=True) if i < self.env.horizon_action else None
            taichi_env.step(action)
            self._write_frame(i)


def record_target(env, path=None, user_input=False, frames_dir=None):
    env.reset()
    return Recorder(env, frames_dir).record(user_input)


def replay_policy(env, path=None, frames_dir=None):
    env.reset()
    Recorder(env, frames_dir).replay_policy(path)
