"""RolloutBuffer: T steps of experience of a device env, written in place.

The step kernels take arbitrary device pointers, so step t of a rollout writes plane t of time-major arrays instead of the
env's one set of output buffers (sag_step_device, sag_episode_track_device), the final observations of the episodes that end
are compacted into a small store before the stream-ordered reset overwrites them (sag_append_rows_device), and after T steps
one kernel turns rewards, costs, `ended` bytes and the learner's values into advantages and returns of the reward and the cost
channel (sag_gae_device).  Everything is enqueued on the env's context stream: nothing waits and nothing is copied to the host
but where a method says so.  NumPy only; no torch."""
import numpy as np

from safe_adaptation_gym_amd import _native as nat

PITCH = 256   # envs per plane are rounded up to this: every per-step plane starts 256-byte aligned, as the library's own buffers


class TimeMajorArray(nat.DeviceArray):
  """A DeviceArray whose first axis is the step: a[t] is the view of step t (contiguous where only the env axis is pitched)."""

  def __getitem__(self, t):
    if not isinstance(t, (int, np.integer)):
      raise TypeError('a time-major device view takes one integer step index')
    t = int(t)
    if not -self.shape[0] <= t < self.shape[0]:
      raise IndexError(f'step {t} of {self.shape[0]}')
    t %= self.shape[0]
    shape, strides = self.shape[1:], tuple(self.strides[1:])
    ptr = self.ptr + t * self.strides[0]
    if strides == nat.dense_strides(shape, self.dtype):
      return nat.DeviceArray(self.ctx, ptr, shape, self.dtype)
    return nat.DeviceArray(self.ctx, ptr, shape, self.dtype, strides=strides, base=self._base)


class RolloutBuffer:
  """buf = RolloutBuffer(env, steps=T, final_capacity=None)
     buf.begin()                                   # obs[0] <- the env's current observation, or obs[T] of the last rollout
     for t in range(T):                            # == buf.collect(policy)
       policy(buf.obs[t], buf.actions[t]); buf.step(t)
     rows, count = buf.final_observations()        # joins the stream once; rows: DeviceArray [count, obs_dim]
     out = buf.advantages(value, cost_value, final_value, final_cost_value, gamma=0.99, lam=0.95)

  env: a BatchedSafeAdaptationGym made with device_buffers=True, device_reset=True and auto_reset=True (with or without
  time_limit), without parity_rng, in one context, with a task set and vector observations; ValueError otherwise, and the env is
  left untouched.

  Device views, time-major (TimeMajorArray: a[t] is step t's view), N = env.n_envs:
    obs [T+1, N, obs_dim] f32      obs[t] is what the policy sees at step t; for an env that ended at step t, obs[t+1] is the
                                   first observation of its new episode
    actions [T, N, nu] f32         reward [T, N] f32       cost, done, terminated, goal_met [T, N] u8
                                   done is the tracker's `ended` byte: 0, 1 (terminated) or 2 (truncated at time_limit)
    episode [T, N, 4] f32          return, cost, length, goals met of the episode that ended; meaningful where done != 0
    final_slot [T, N] int32        where done != 0: the row of final_observations() that holds the observation the final
                                   transition reached, or -1 if the store was full; -1 elsewhere
    value, cost_value [T+1, N], logp [T, N], final_value, final_cost_value [final_capacity] f32: owned views made on first use,
                                   which a policy on the device fills (MLPPolicy.act_into / evaluate) and advantages() reads
  final_capacity: rows of the final-observation store; default N * (T // time_limit + 1) with a time limit, else N.  A row
  that does not fit is counted (final_dropped()), not an error.

  The buffer shares the context's episode accumulators with env.step(): mixing the two is legal (begin(from_env=True) after
  steps of the env's own).  The env's own output buffers - the views env.step() returned - are stale after a rollout."""

  def __init__(self, env, steps, final_capacity=None):
    from safe_adaptation_gym_amd.envs import BatchedSafeAdaptationGym
    if not isinstance(env, BatchedSafeAdaptationGym):
      raise ValueError('RolloutBuffer: env must be a BatchedSafeAdaptationGym')
    if env.parity_rng:
      raise ValueError('RolloutBuffer: parity_rng draws and resets on the host every step')
    if not (env.device_buffers and env.device_reset and env.auto_reset):
      raise ValueError('RolloutBuffer needs an env made with device_buffers=True, device_reset=True and auto_reset=True')
    if env._rgb_observation:
      raise ValueError('RolloutBuffer: rgb_observation is not supported - an image row of 12 KiB per step and env is another '
                       'design (a buffer of images would hold 50 GB for 16 steps of a million envs)')
    if len(env._ctx) != 1:
      raise ValueError(f'RolloutBuffer: the env is sharded over {len(env._ctx)} contexts; one buffer serves one context')
    if env._tasks is None:
      raise ValueError('RolloutBuffer: a task should be first set')
    T = int(steps)
    if T < 1:
      raise ValueError(f'RolloutBuffer: steps={steps}')
    N = env.n_envs
    if final_capacity is None:
      final_capacity = N * (T // env.time_limit + 1) if env.time_limit else N
    cap = int(final_capacity)
    if cap < 1:
      raise ValueError(f'RolloutBuffer: final_capacity={final_capacity}')
    self.env, self.T, self.N, self.final_capacity = env, T, N, cap
    self.P = P = (N + PITCH - 1) // PITCH * PITCH
    self.obs_dim, self.nu = env.robot.obs_dim, env.robot.nu
    self._ctx = c = env._ctx[0]
    od, nu = self.obs_dim, self.nu
    self._bufs = nat.DeviceBuffers(c)
    self._t = None         # the step to enqueue next; None before begin()
    self._rollouts = 0
    self._restart = True   # the next append zeroes the store's counter
    try:
      alloc = self._bufs.alloc
      alloc('obs', (T + 1) * P * od * 4); alloc('actions', T * P * nu * 4); alloc('reward', T * P * 8)
      for k in ('cost', 'done', 'terminated', 'goal_met'):
        alloc(k, T * P)
      alloc('episode', T * P * 16); alloc('final_slot', T * P * 4)
      alloc('store', cap * od * 4); alloc('count', 256, zero=True)
    except Exception:
      self.close()
      raise
    A = TimeMajorArray
    b = {k: self._bufs[k].value for k in ('obs', 'actions', 'reward', 'cost', 'done', 'terminated', 'goal_met', 'episode', 'final_slot')}
    self.obs = A(c, b['obs'], (T + 1, N, od), np.float32, strides=(P * od * 4, od * 4, 4), base=(b['obs'], (T + 1, P, od)))
    self.actions = A(c, b['actions'], (T, N, nu), np.float32, strides=(P * nu * 4, nu * 4, 4), base=(b['actions'], (T, P, nu)))
    self.reward = A(c, b['reward'], (T, N), np.float32, strides=(P * 8, 8), base=(b['reward'], (T, P, 2)))
    for k in ('cost', 'done', 'terminated', 'goal_met'):
      setattr(self, k, A(c, b[k], (T, N), np.uint8, strides=(P, 1), base=(b[k], (T, P))))
    self.episode = A(c, b['episode'], (T, N, 4), np.float32, strides=(P * 16, 16, 4), base=(b['episode'], (T, P, 4)))
    self.final_slot = A(c, b['final_slot'], (T, N), np.int32, strides=(P * 4, 4), base=(b['final_slot'], (T, P)))

  # -- addresses -----------------------------------------------------------------------------------------------------
  def _at(self, key, t, elem_bytes):
    """Device pointer of plane t of a [.][P][...] array whose env rows are elem_bytes wide."""
    return nat.C.c_void_p(self._bufs[key].value + t * self.P * elem_bytes)

  def _plane(self, key, shape, dtype=np.float32):
    """An owned [rows][P] (or [rows]) buffer made on first use, zero-filled."""
    if key not in self._bufs:
      self._bufs.alloc(key, int(np.prod(shape)) * np.dtype(dtype).itemsize, zero=True)
    return self._bufs[key]

  def _tm(self, key, rows):
    P = self.P
    self._plane(key, (rows, P))
    p = self._bufs[key].value
    return TimeMajorArray(self._ctx, p, (rows, self.N), np.float32, strides=(P * 4, 4), base=(p, (rows, P)))

  # the learner's values, as device views it may write itself (then pass the view to advantages())
  @property
  def value(self):
    return self._tm('value', self.T + 1)

  @property
  def cost_value(self):
    return self._tm('cvalue', self.T + 1)

  @property
  def logp(self):
    """[T, N] f32: the log-probability of actions[t] under the policy that drew them (MLPPolicy.act_into writes it)."""
    return self._tm('logp', self.T)

  @property
  def final_value(self):
    return nat.DeviceArray(self._ctx, self._plane('fvalue', (self.final_capacity,)).value, (self.final_capacity,), np.float32)

  @property
  def final_cost_value(self):
    return nat.DeviceArray(self._ctx, self._plane('fcvalue', (self.final_capacity,)).value, (self.final_capacity,), np.float32)

  # -- the rollout -----------------------------------------------------------------------------------------------------
  def begin(self, from_env=None):
    """Starts a rollout: obs[0] <- the env's current observation on the first call, obs[T] of the last rollout afterwards
    (from_env=True: the env's current observation again, after env.step() / env.reset() calls of the caller's own), and the
    final-observation store restarts.  Enqueued on the stream, but for an env that was never reset or stepped."""
    c, env, row = self._ctx, self.env, self.obs_dim * 4
    if from_env is None:
      from_env = self._rollouts == 0
    if not from_env:
      c.copy_rows(None, row, self._at('obs', self.T, row), self._at('obs', 0, row))
    elif env._dev is not None:
      c.copy_rows(None, row, env._dev[0]['obs'], self._at('obs', 0, row))
    else:   # set_task() alone forms no observation
      c.dev_upload(self._at('obs', 0, row), c.observe())
    self._t, self._restart = 0, True
    self._rollouts += 1

  def set_actions(self, t, actions):
    """Host actions [N, nu] of step t, uploaded into actions[t] (as env.step() uploads host actions)."""
    a = np.ascontiguousarray(np.asarray(actions, np.float32).reshape(self.N, self.nu))
    if not 0 <= int(t) < self.T:
      raise ValueError(f'RolloutBuffer.set_actions: step {t} of {self.T}')
    self._ctx.dev_upload(self._at('actions', int(t), self.nu * 4), a)

  def step(self, t):
    """Enqueues step t on the env's context: the step from actions[t] into obs[t+1], reward[t], cost[t], terminated[t] and
    goal_met[t]; the episode tracker into done[t] and episode[t]; the append of the final observations of the envs that ended
    (final_slot[t]); their reset, which writes the first observations of the new episodes into obs[t+1].  No wait.  Steps go
    in order 0 ... T-1 after begin(); ValueError otherwise.  actions[t] is read on the context's stream: whoever writes it on
    another stream orders that against it, as for env.step(device_action)."""
    if self._t is None:
      raise ValueError('RolloutBuffer.step: call begin() first')
    if not isinstance(t, (int, np.integer)) or int(t) != self._t or self._t >= self.T:
      raise ValueError(f'RolloutBuffer.step({t}): steps are enqueued in order, the next one is '
                       f'{self._t if self._t < self.T else "begin()"}')
    t, c, env, at = int(t), self._ctx, self.env, self._at
    row = self.obs_dim * 4
    obs1, rew, cost, term, met, done = at('obs', t + 1, row), at('reward', t, 8), at('cost', t, 1), at('terminated', t, 1), \
        at('goal_met', t, 1), at('done', t, 1)
    c.step_device(at('actions', t, self.nu * 4), None, -1, obs1, rew, cost, term, met)
    c.episode_track(rew, cost, term, met, env.time_limit or 0, done, at('episode', t, 16))
    c.append_rows(done, row, obs1, self._bufs['store'], self.final_capacity, self._bufs['count'], self._restart, at('final_slot', t, 4))
    c.reset_device_async(done, obs1)
    self._restart = False
    self._t = t + 1

  def collect(self, policy):
    """begin(), then T times policy(obs[t], actions[t]) - which fills the action rows, on the device or with set_actions - and
    step(t).  A policy with an act_into(buf, t) method (MLPPolicy) is asked through it instead: it also writes logp[t], value[t]
    and cost_value[t]."""
    self.begin()
    act_into = getattr(policy, 'act_into', None)
    for t in range(self.T):
      if act_into is not None:
        act_into(self, t)
      else:
        policy(self.obs[t], self.actions[t])
      self.step(t)

  def wait(self):
    self._ctx.wait()

  def _count(self):
    if self._restart:   # (begin() was called and no step has restarted the counter on the stream yet)
      return 0
    return int(self._ctx.dev_download(self._bufs['count'], (1,), np.int32)[0])

  def final_observations(self):
    """-> (rows, count): rows is a DeviceArray [count, obs_dim] of the final observations kept in this rollout so far, row
    final_slot[t][i] that of the episode env i ended at step t.  Joins the stream once (4 bytes come to the host)."""
    count = min(self._count(), self.final_capacity)
    return nat.DeviceArray(self._ctx, self._bufs['store'].value, (count, self.obs_dim), np.float32), count

  def final_dropped(self):
    """Final observations of this rollout that did not fit the store (their final_slot is -1).  Joins the stream."""
    return max(0, self._count() - self.final_capacity)

  # -- advantages --------------------------------------------------------------------------------------------------
  def _values(self, key, x, rows, what):
    """Device pointer of a [rows][P] value array: host values are uploaded into the owned buffer, a device array must have
    the buffer's pitch (the owned views `value` / `cost_value` have it)."""
    N, P = self.N, self.P
    if nat.is_device_array(x):
      v = nat.device_view(x, f'RolloutBuffer.advantages: {what}', self._ctx.device)
      if v.dtype != np.dtype('<f4') or v.shape != (rows, N) or v.strides != (P * 4, 4) or v.ptr % 4:
        raise ValueError(f'RolloutBuffer.advantages: a device {what} must be float32 of shape ({rows}, {N}) with strides '
                         f'({P * 4}, 4) - write into the buffer\'s own view')
      return nat.C.c_void_p(v.ptr)
    h = np.asarray(x, np.float32)
    if h.shape != (rows, N):
      raise ValueError(f'RolloutBuffer.advantages: {what} of shape {h.shape}, not ({rows}, {N})')
    full = np.zeros((rows, P), np.float32)
    full[:, :N] = h
    self._ctx.dev_upload(self._plane(key, (rows, P)), full)
    return self._bufs[key]

  def _finals(self, key, x, what):
    cap = self.final_capacity
    if nat.is_device_array(x):
      return nat.C.c_void_p(nat.device_pointer(x, (cap,), self._ctx.device))
    h = np.asarray(x, np.float32)
    if h.ndim != 1 or len(h) > cap:
      raise ValueError(f'RolloutBuffer.advantages: {what} of shape {h.shape}: one value per kept final row, at most {cap}')
    full = np.zeros(cap, np.float32)
    full[:len(h)] = h
    self._ctx.dev_upload(self._plane(key, (cap,)), full)
    return self._bufs[key]

  def advantages(self, value, cost_value=None, final_value=None, final_cost_value=None, gamma=0.99, lam=0.95, cost_gamma=None,
                 cost_lam=None):
    """Generalised advantage estimation over the T stored steps (sag_gae_device; include/sag.h has the recurrence), enqueued
    on the stream -> {'adv', 'ret'} and, with cost_value, {'cadv', 'cret'}: device views [T, N] float32, overwritten by the
    next call.
    value, cost_value: [T+1, N], the learner's values of obs[0 ... T]; final_value, final_cost_value: its values of the rows
    of final_observations(), [count] or [final_capacity].  Host arrays are uploaded into buffers the object owns; device
    arrays are read in place (the views buf.value, buf.cost_value, buf.final_value, buf.final_cost_value have the required
    layout).  An episode that ended by termination bootstraps from 0, one truncated at time_limit from its final value -
    from 0 when no final values are given or its row was dropped.  cost_gamma / cost_lam default to gamma / lam."""
    if self._t != self.T:
      raise ValueError('RolloutBuffer.advantages: the rollout is not complete')
    T, P, b = self.T, self.P, self._bufs
    for name, v in (('gamma', gamma), ('lam', lam), ('cost_gamma', cost_gamma), ('cost_lam', cost_lam)):
      if v is not None and not (0 <= v <= 1):
        raise ValueError(f'RolloutBuffer.advantages: {name}={v} is outside [0, 1]')
    d_value = self._values('value', value, T + 1, 'value')
    d_cvalue = None if cost_value is None else self._values('cvalue', cost_value, T + 1, 'cost_value')
    d_fv = None if final_value is None else self._finals('fvalue', final_value, 'final_value')
    d_fcv = None if final_cost_value is None or cost_value is None else self._finals('fcvalue', final_cost_value, 'final_cost_value')
    keys = ('adv', 'ret') + (('cadv', 'cret') if d_cvalue is not None else ())
    for k in keys:
      self._plane(k, (T, P))
    self._ctx.gae(T, P, b['reward'], b['cost'], b['done'], d_value, b['adv'], b['ret'], gamma, lam, d_cvalue=d_cvalue,
                  d_cadv=b.get('cadv') if d_cvalue is not None else None, d_cret=b.get('cret') if d_cvalue is not None else None,
                  cost_gamma=cost_gamma, cost_lam=cost_lam, d_slot=b['final_slot'], capacity=self.final_capacity,
                  d_final_value=d_fv, d_final_cvalue=d_fcv)
    return {k: TimeMajorArray(self._ctx, b[k].value, (T, self.N), np.float32, strides=(P * 4, 4), base=(b[k].value, (T, P)))
            for k in keys}

  def close(self):
    self._bufs.close()
    self._ctx = None
