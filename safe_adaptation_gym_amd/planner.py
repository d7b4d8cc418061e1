"""ShootingPlanner: a constrained cross-entropy planner over the simulator itself, on the device.

Every real env is broadcast to K candidate envs of an internal context (sag_fork_device); each iteration draws K action
sequences per real env around the current mean (sag_plan_sample_device), rolls them out for H steps without forming an
observation while return and cost accumulate (sag_plan_score_device), ranks them under the cost budget and refits mean and
sigma to the elites (sag_plan_refit_device).  Everything is enqueued on the planner context's stream, ordered against the
env's stream by events: plan() does not wait and copies nothing to the host.  NumPy only; no torch."""
import math

import numpy as np

from safe_adaptation_gym_amd import _native as nat


class ShootingPlanner:
  """planner = ShootingPlanner(env, candidates=64, horizon=12, iterations=3, elites=8, gamma=0.99, cost_budget=0.0,
                                init_sigma=0.5, min_sigma=0.05, common_noise=False)
     act = planner.plan()                      # DeviceArray [n_envs, nu]: the first action of the final mean
     obs, r, done, info = env.step(act)

  env: made with device_buffers=True and device_reset=True, without parity_rng, on one device, with a task set
  (rgb_observation envs are fine: the planner never forms an observation); ValueError otherwise.
  cost_budget: the discounted cost a candidate may collect over the horizon and still count as feasible - a float, an array
  [n_envs] (one budget per real env) or None for no constraint.  Feasible candidates rank by return; when a group has fewer
  than `elites` of them, the infeasible ones with the lowest cost fill up.
  common_noise: the candidates take their real env's id in the fork (SAG_FORK_SAME_STREAM), so all K rollouts of a group
  see the action noise and in-step draws the real env will see; otherwise each candidate draws its own."""

  def __init__(self, env, candidates=64, horizon=12, iterations=3, elites=8, gamma=0.99, cost_budget=0.0, init_sigma=0.5,
               min_sigma=0.05, common_noise=False):
    from safe_adaptation_gym_amd.envs import BatchedSafeAdaptationGym
    if not isinstance(env, BatchedSafeAdaptationGym):
      raise ValueError('ShootingPlanner: env must be a BatchedSafeAdaptationGym')
    if not (env.device_buffers and env.device_reset) or env.parity_rng:
      raise ValueError('ShootingPlanner needs an env made with device_buffers=True and device_reset=True, without parity_rng')
    if len(env._ctx) != 1:
      raise ValueError(f'ShootingPlanner: the env is sharded over {len(env._ctx)} contexts; one planner serves one shard')
    if env._tasks is None:
      raise ValueError('ShootingPlanner: a task should be first set')
    K, H, I, E = int(candidates), int(horizon), int(iterations), int(elites)
    if K < 1 or H < 1 or I < 1 or E < 1 or E > K:
      raise ValueError(f'ShootingPlanner: candidates={candidates}, horizon={horizon}, iterations={iterations}, elites={elites}: '
                       'each at least 1, and no more elites than candidates')
    if not (0 < gamma <= 1):
      raise ValueError(f'ShootingPlanner: gamma={gamma} is outside (0, 1]')
    for name, v in (('init_sigma', init_sigma), ('min_sigma', min_sigma)):
      if not (math.isfinite(v) and v >= 0):
        raise ValueError(f'ShootingPlanner: {name}={v} must be finite and not negative')
    self.env, self.K, self.H, self.I, self.E = env, K, H, I, E
    self.G, self.nu = env.n_envs, env.robot.nu
    self.gamma, self.init_sigma, self.min_sigma = float(gamma), float(init_sigma), float(min_sigma)
    self.common_noise = bool(common_noise)
    budget = None
    if cost_budget is not None:
      budget = np.asarray(cost_budget, np.float32)
      if budget.ndim == 0:
        budget = np.full(self.G, budget, np.float32)
      if budget.shape != (self.G,) or np.isnan(budget).any():
        raise ValueError(f'ShootingPlanner: cost_budget is a float, an array of shape ({self.G},) or None')
    self._src_ctx = env._ctx[0]
    G, n, nu = self.G, self.G * K, self.nu
    # the planner context: the env's records K times over, each candidate with an env id (= a noise stream) of its own
    rf, ri = env.get_state()
    rf, ri = np.repeat(rf, K, axis=0), np.repeat(ri, K, axis=0)
    ri[:, nat.I_ENV_ID] = np.arange(n)
    self._ctx = c = nat.Context(env.robot.name, n, device=self._src_ctx.device, seed=self._key())
    self._bufs = nat.DeviceBuffers(c)
    try:
      c.set_layout(rf, ri)
      alloc = self._bufs.alloc
      alloc('src', 4 * n); alloc('plans', 4 * H * n * nu); alloc('mean', 4 * H * G * nu); alloc('sigma', 4 * H * G * nu)
      alloc('score', 16 * n); alloc('best', 4 * G); alloc('best_score', 16 * G); alloc('mask', G)
      if budget is not None:
        alloc('budget', 4 * G)
        c.dev_upload(self._bufs['budget'], budget)
      c.dev_upload(self._bufs['src'], (np.arange(n) // K).astype(np.int32))
      c.dev_upload(self._bufs['best'], np.zeros(G, np.int32))
      c.dev_upload(self._bufs['best_score'], np.zeros((G, 4), np.float32))
      c.plan_clear(G, H, None, self._bufs['mean'], self._bufs['sigma'], self.init_sigma)
    except Exception:
      self.close()
      raise
    self._draw = 0          # word 1 of the sampling counter: advances with every sample call
    self._planned = False   # the mean holds a plan whose first action was handed out: the next plan() shifts it

  def _key(self):
    env = self.env
    return env._base_seed if env._device_seed is None else env._device_seed

  def plan(self):
    """-> DeviceArray [n_envs, nu] float32, a view of the first action of the refitted mean.  Enqueued on the planner's
    stream; the env's stream is made to wait for it, so env.step(act) may follow at once.  The view is overwritten by the
    next plan() (which first waits, on the device, for the env's stream).  plan() is begin(), `iterations` times
    iterate(), then action()."""
    self.begin()
    for _ in range(self.I):
      self.iterate()
    return self.action()

  def begin(self):
    """The receding-horizon warm start: once an action was handed out, the mean moves up by one step (the last row 0) and
    sigma returns to init_sigma."""
    c, b = self._ctx, self._bufs
    c.set_seed(self._key())   # (env.seed() / reset(seed=...) re-key the env's generator)
    if self._planned:
      c.wait_for(self._src_ctx)   # a step of the env may still be reading the first action of the old mean
      c.plan_shift(self.G, self.H, b['mean'], b['sigma'], self.init_sigma)
      self._planned = False

  def iterate(self):
    """One iteration: fork the env's current state into the K candidates of every env, sample, score, refit."""
    c, b, K, H = self._ctx, self._bufs, self.K, self.H
    c.fork_device(b['src'], self._src_ctx, same_stream=self.common_noise)
    c.plan_sample(K, H, b['mean'], b['sigma'], self._draw, b['plans'])
    self._draw = (self._draw + 1) & 0xffffffff
    c.plan_score(b['plans'], H, self.gamma, b['score'])
    c.plan_refit(K, H, self.E, b['plans'], b['score'], b.get('budget'), self.min_sigma, b['mean'], b['sigma'], b['best'],
                 b['best_score'])

  def action(self):
    """The view of the mean's first action, with the env's stream made to wait for the planner's."""
    self._src_ctx.wait_for(self._ctx)
    self._planned = True
    return nat.DeviceArray(self._ctx, self._bufs['mean'].value, (self.G, self.nu), np.float32)

  def best(self):
    """-> (k [n_envs] int32, score [n_envs, 4] float32) of the last refit, as device views: the candidate ranked first in
    each group and its {discounted return, discounted cost, steps alive, goals met}.  Written on the planner's stream:
    numpy() joins it."""
    c, b = self._ctx, self._bufs
    return nat.DeviceArray(c, b['best'].value, (self.G,), np.int32), nat.DeviceArray(c, b['best_score'].value, (self.G, 4), np.float32)

  def mean(self):
    """-> (mean, sigma), device views [horizon, n_envs, nu] of the sampling distribution."""
    c, b, shape = self._ctx, self._bufs, (self.H, self.G, self.nu)
    return nat.DeviceArray(c, b['mean'].value, shape, np.float32), nat.DeviceArray(c, b['sigma'].value, shape, np.float32)

  def reset(self, mask=None):
    """mean = 0, sigma = init_sigma for every env or for the envs of `mask` (a host bool / uint8 array [n_envs], or a device
    array of uint8 [n_envs] such as step()'s `done` view): call it when episodes restart."""
    c, b = self._ctx, self._bufs
    d_mask = None
    if mask is not None:
      if nat.is_device_array(mask):
        d_mask = nat.C.c_void_p(nat.device_pointer(mask, (self.G,), c.device, np.uint8))
      else:
        m = np.asarray(mask)
        if m.shape != (self.G,) or m.dtype not in (np.bool_, np.uint8):
          raise ValueError(f'mask: bool / uint8 of shape ({self.G},), not {m.dtype} {m.shape}')
        c.dev_upload(b['mask'], m.astype(np.uint8))
        d_mask = b['mask']
    c.wait_for(self._src_ctx)   # (a device mask written by the env's step; a step still reading the old first action)
    c.plan_clear(self.G, self.H, d_mask, b['mean'], b['sigma'], self.init_sigma)

  def wait(self):
    self._ctx.wait()

  def close(self):
    self._bufs.close()
    self._ctx.close()
