"""safe_adaptation_gym_amd: batched SafeAdaptationGym.step() on MI355X.

`make()` mirrors the reference factory (safe_adaptation_gym/__init__.py:6-24) with
an extra `n_envs` (batch size), `devices` (GPU ordinals to shard over) and `device_buffers` (step() / reset() return
views of HBM instead of NumPy copies: envs.BatchedSafeAdaptationGym.step) and `device_reset` (reset() samples the layouts on
the device, throughput mode only, and accepts a mask of envs to reset: envs.BatchedSafeAdaptationGym.reset)."""
from typing import Dict, Optional


def __getattr__(name):
  if name == 'ShootingPlanner':   # sag.ShootingPlanner(env, ...): a constrained CEM planner on the device (planner.py)
    from safe_adaptation_gym_amd.planner import ShootingPlanner
    return ShootingPlanner
  if name == 'RolloutBuffer':   # sag.RolloutBuffer(env, steps): time-major storage written in place, final rows, GAE (rollout_buffer.py)
    from safe_adaptation_gym_amd.rollout_buffer import RolloutBuffer
    return RolloutBuffer
  if name == 'MLPPolicy':   # sag.MLPPolicy(env, hidden): a Gaussian actor-critic MLP whose forward runs on the device (policy.py)
    from safe_adaptation_gym_amd.policy import MLPPolicy
    return MLPPolicy
  if name == 'PPOLearner':   # sag.PPOLearner(pi, buf): the PPO-Lagrangian update of an MLPPolicy on the device (learner.py)
    from safe_adaptation_gym_amd.learner import PPOLearner
    return PPOLearner
  raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def make(robot_name: str,
         task_name: Optional[str] = None,
         seed: int = 666,
         config: Optional[Dict] = None,
         rgb_observation: bool = False,
         render_options: Optional[Dict] = None,
         render_lidar_and_collision=True,
         n_envs: int = 1,
         devices=None,
         parity_rng: bool = False,
         device_buffers: bool = False,
         device_reset: bool = False,
         time_limit: Optional[int] = None,
         auto_reset: bool = False,
         final_observation: bool = False):
  from safe_adaptation_gym_amd.benchmark import ROBOTS_BASENAMES, TASKS
  from safe_adaptation_gym_amd.envs import BatchedSafeAdaptationGym
  env = BatchedSafeAdaptationGym(
      ROBOTS_BASENAMES[robot_name.lower()],
      n_envs=n_envs,
      config=config,
      rgb_observation=rgb_observation,
      devices=devices,
      parity_rng=parity_rng,
      device_buffers=device_buffers,
      device_reset=device_reset,
      time_limit=time_limit,
      auto_reset=auto_reset,
      final_observation=final_observation,
      render_lidars_and_collision=render_lidar_and_collision,
      render_options=render_options)
  env.seed(seed)
  if task_name is not None:
    env.set_task(TASKS[task_name.lower()])
  return env
