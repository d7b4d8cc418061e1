"""Batched SafeAdaptationGym: the reference's make / reset / step / set_task surface
(safe_adaptation_gym.py:21-257) over N independent environments stepped by the HIP
kernels of libsag.so.  NumPy only; no torch.

Environments never interact, so a batch is split into contiguous shards, one
native context (= one GPU, one stream) per shard, with no collective anywhere."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from safe_adaptation_gym_amd import _native as nat
from safe_adaptation_gym_amd.robot import Robot
from safe_adaptation_gym_amd.tasks.task import Task
from safe_adaptation_gym_amd.utils import ResamplingError
from safe_adaptation_gym_amd import consts

TAPE_WORDS = 1024  # raw generator words offered to the device per env per step (parity mode)


class Box:
  """Minimal stand-in for gym.spaces.Box (gym is not a dependency)."""

  def __init__(self, low, high, shape, dtype=np.float32, seed=None):
    self.low = np.broadcast_to(np.asarray(low, dtype), shape).copy()
    self.high = np.broadcast_to(np.asarray(high, dtype), shape).copy()
    self.shape, self.dtype = tuple(shape), dtype
    self._rs = np.random.RandomState(seed)

  def sample(self):
    return self._rs.uniform(self.low, self.high).astype(self.dtype)

  def contains(self, x):
    x = np.asarray(x)
    return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))


def shard_ranges(n, parts):
  """Contiguous [start, stop) ranges splitting n envs over `parts` devices."""
  base, rem = divmod(n, parts)
  out, s = [], 0
  for p in range(parts):
    e = s + base + (1 if p < rem else 0)
    out.append((s, e))
    s = e
  return out


class BatchedSafeAdaptationGym:
  NUM_LIDAR_BINS = 16
  LIDAR_MAX_DIST = 5.
  BASE_SENSORS = ['accelerometer', 'velocimeter', 'gyro', 'magnetometer']

  def __init__(self, robot_base, n_envs=1, rgb_observation=False, config=None, devices=None,
               parity_rng=False, device_seed=None, render_lidars_and_collision=False, render_options=None,
               device_buffers=False, device_reset=False, time_limit=None, auto_reset=False, final_observation=False):
    # rgb_observation: the observation is the robot camera's 64 x 64 x 3 uint8 image
    # (safe_adaptation_gym.py:122-126,148-149), ray-cast on the device
    self._rgb_observation = bool(rgb_observation)
    # human view (safe_adaptation_gym.py:37-38,109-111): render(**render_options) of the scene's cameras, with the
    # lidar rings / cost sphere of render.py when render_lidars_and_collision
    self._render_lidars_and_collision = bool(render_lidars_and_collision)
    self._render_options = dict(render_options) if render_options else {}
    self.robot = Robot(robot_base)
    self.n_envs = int(n_envs)
    self.base_config = config
    self.parity_rng = bool(parity_rng)
    # device_buffers: step() / reset() leave their results in HBM and return _native.DeviceArray views of them (see
    # step()); actions may be device arrays too.  The reference's API, without the PCIe round trip per step.
    self.device_buffers = bool(device_buffers)
    if self.device_buffers and self.parity_rng:
      raise ValueError('device_buffers: the reference-order host generators of parity_rng draw on the host every step')
    # device_reset: reset() samples the new layouts on the device (sag_reset_device, throughput mode only): no record
    # download / upload, and reset(mask=...) resets some envs only
    self.device_reset = bool(device_reset)
    if self.device_reset and self.parity_rng:
      raise ValueError('device_reset: parity_rng reproduces the reference\'s host MT19937 layout stream')
    # time_limit / auto_reset: the episode loop on the contexts' streams (sag_episode_track_device after every step, then
    # sag_reset_device_async of the envs that ended); final_observation: the observation rows of the envs that ended are
    # saved (sag_copy_rows_device) before that reset overwrites them; see step()
    if (time_limit is not None or auto_reset or final_observation) and self._rgb_observation:
      # (the constructor's refusal is kept as it was; the loop itself handles images: episode_loop())
      raise ValueError('time_limit / auto_reset with rgb_observation is not supported by make(): call '
                       'env.episode_loop(time_limit, auto_reset) on the env')
    self._set_episode_loop(time_limit, auto_reset, final_observation)
    self._last_obs = None   # device_reset, host buffers: what the last step() returned (rows kept by a masked reset)
    self._mask_bufs = None  # device_reset: per-shard device copies of a host reset mask
    self._fork_bufs = None  # fork(): per-shard device copies of a host source-index array
    # rgb_observation with device_buffers: every row of the image buffers shows its env's current state or, for an env kept
    # by a masked reset, what the last step returned - only then may a reset render the rows of its mask alone
    self._img_valid = False
    self.devices = [0] if devices is None else list(devices)
    if self.n_envs < len(self.devices):
      self.devices = self.devices[:self.n_envs]
    self._ranges = shard_ranges(self.n_envs, len(self.devices))
    # throughput mode: the device-side generator is keyed by the env seed (seed() / reset(seed=...)) unless
    # device_seed pins it; counter = (global env id, step, draw, episode), so noise and in-step draws differ
    # between envs, steps, episodes and seeds
    self._device_seed = device_seed
    self._ctx = [
        nat.Context(self.robot.name, e - s, device=d, seed=0 if device_seed is None else device_seed)
        for (s, e), d in zip(self._ranges, self.devices)
    ]
    self._own = [nat.DeviceBuffers(c) for c in self._ctx]   # every shard's allocations: _dev, _mask_bufs, _fork_bufs
    self._pool = ThreadPoolExecutor(len(self._ctx)) if len(self._ctx) > 1 else None
    self._dev = None   # device_buffers: per-shard output / action buffers, allocated on first use
    self._tasks = None
    self._episode = 0
    self._base_seed = int(np.random.randint(2**31))
    self._seeds = self._base_seed + np.arange(self.n_envs, dtype=np.int64)
    self._rs = None
    self._key_device()
    self.action_space = Box(-1, 1, (self.robot.nu,), np.float32)
    self._observation_space = None
    self._reward_dim = 1

  def _set_episode_loop(self, time_limit, auto_reset, final_observation=False):
    self.time_limit = None if time_limit is None else int(time_limit)
    self.auto_reset = bool(auto_reset)
    self.final_observation = bool(final_observation)
    if self.final_observation and not self.auto_reset:
      raise ValueError('final_observation needs auto_reset=True: without it the observation a step returns is the final one')
    self._track = self.time_limit is not None or self.auto_reset
    if self._track:
      if self.parity_rng:
        raise ValueError('time_limit / auto_reset: parity_rng resets on the host, in the reference\'s order')
      if not (self.device_buffers and self.device_reset):
        raise ValueError('time_limit / auto_reset need device_buffers=True and device_reset=True')
      if self.time_limit is not None and self.time_limit <= 0:
        raise ValueError(f'time_limit must be positive, not {time_limit}')

  def episode_loop(self, time_limit=None, auto_reset=False, final_observation=False):
    """Turns on what make(..., time_limit=, auto_reset=, final_observation=) turns on - the episode tracker, the stream-ordered
    reset of the envs that ended and the copy of their final observations, see step() - on an env that exists.  This is how
    an rgb_observation env gets them: make() refuses that combination, the loop does not.  Same requirements (device_buffers, device_reset, no parity_rng), ValueError otherwise
    and the env stays as it was; to be called before the first reset() / step() (the device buffers are laid out then)."""
    if self._dev is not None:
      raise ValueError('episode_loop(): call it before the first reset() / step()')
    old = self.time_limit, self.auto_reset, self.final_observation
    try:
      self._set_episode_loop(time_limit, auto_reset, final_observation)
    except ValueError:
      self._set_episode_loop(*old)
      raise
    if self._track and self._tasks is not None:
      self._map(lambda c, s, e: c.episode_clear())

  # -- reference surface ----------------------------------------------------------
  @property
  def rs(self):
    """Per-env host generators (safe_adaptation_gym.py:33,113-118).  Only parity mode draws from
    them, so they are built on first use (a RandomState costs ~0.1 ms: 100 s per million envs)."""
    if self._rs is None:
      self._rs = [np.random.RandomState(int(s) % 2**32) for s in self._seeds]
    return self._rs

  @property
  def observation_space(self):
    if self._observation_space is None and self._rgb_observation:
      self._observation_space = Box(0, 255, (64, 64, 3), np.uint8)
    if self._observation_space is None:
      d = self.robot.obs_dim
      lidar = 3 * self.NUM_LIDAR_BINS
      low = np.array([0.] * lidar + [-np.inf] * (d - lidar), np.float32)
      high = np.array([1.] * lidar + [np.inf] * (d - lidar), np.float32)
      self._observation_space = Box(low, high, (d,), np.float32)
    return self._observation_space

  def seed(self, seed=None):
    """Env i uses seed + i (the reference's single env uses `seed`,
    safe_adaptation_gym.py:113-118)."""
    self._base_seed = int(np.random.randint(2**31)) if seed is None else int(seed)
    self._seeds = self._base_seed + np.arange(self.n_envs, dtype=np.int64)
    self._rs = None
    self._key_device()

  def _key_device(self):
    if self._device_seed is None:
      for c in self._ctx:
        c.set_seed(self._base_seed)

  def set_task(self, task):
    """A Task instance / class (every env gets its own instance of that class) or a
    sequence of n_envs instances (heterogeneous batch)."""
    self._tasks = self._expand_tasks(task)
    unknown = set(self.base_config or {}) - set(consts.WORLD_DEFAULT)   # the reference accepts anything (world.py:43-44)
    if unknown:
      raise KeyError(f'unknown world config keys: {sorted(unknown)}')
    # the native sampler draws from what the Task objects say about themselves (tasks/task.py: obstacles,
    # placement_extents, setup_placements(), attributes), deduplicated: env j uses descriptor _desc_of_env[j]
    self._descs, self._desc_of_env, seen = [], np.zeros(self.n_envs, np.int32), {}
    for j, t in enumerate(self._tasks):
      d = t.descriptor()
      key = repr(sorted(d.items()))
      if key not in seen:
        seen[key] = len(self._descs)
        self._descs.append(d)
      self._desc_of_env[j] = seen[key]
    self._task_ids = np.array([t.TASK_ID for t in self._tasks], np.int32)
    self._reward_dim = max(t.REWARD_DIM for t in self._tasks)
    self._persist = None  # task attributes that outlive an episode (filled by _pull_task_state)
    self._img_valid = False
    if self._track:
      self._map(lambda c, s, e: c.episode_clear())
    if self.device_reset:
      self._map(lambda c, s, e: c.set_tasks(self._descs, self._desc_of_env[s:e], self.base_config, env_id0=s))
      self._reset_device(first_episode=True)
    else:
      self._build_world(first_episode=True)

  def reset(self, *, seed=None, return_info=False, options=None, mask=None, sync=True):
    """mask (device_reset only): the envs to reset - a host bool / uint8 array [n_envs], or one device array of uint8
    [n_shard] per shard (a DeviceArray such as step()'s `done` view, or any torch / cupy array on the shard's
    device; a list when there are several shards).  The other envs keep their state, and their rows of the returned
    observation are what the last step() returned.  A device mask written on another stream must be complete before
    the call (as device actions).

    sync=False (device_reset and device_buffers): the same reset enqueued on the contexts' streams
    (sag_reset_device_async) - the observation view comes back without waiting, the rows of the reset envs are written
    by the stream; mask=None resets every env.  No ResamplingError is raised: an env whose layout cannot be sampled keeps
    its state and observation row and gets bit 0 of its flags, and reset_counts() tells how many there were.

    rgb_observation: the observation is the image view [n, 64, 64, 3] uint8.  A masked reset renders the envs of the mask
    only (sag_render_rows_device), each into its own row; the other rows are not written.  The masked render takes no
    status: an env of the mask whose layout could not be sampled kept its state, so rendering it again writes the bytes its
    row already holds - it keeps its observation row by value.  With sync=False the vector observation is not formed at
    all."""
    assert self._tasks is not None or (options is not None and 'task' in options), (
        'A task should be first set before reset.')
    if mask is not None and not self.device_reset:
      raise ValueError('reset(mask=...) needs device_reset=True')
    if mask is not None and options is not None and 'task' in options:
      raise ValueError('reset(mask=...) with a new task: a task is set for the whole batch')
    ptrs = None
    if not sync:
      if not (self.device_buffers and self.device_reset):
        raise ValueError('reset(sync=False) needs device_buffers=True and device_reset=True')
      if options is not None and 'task' in options:
        raise ValueError('reset(sync=False): not with a new task')
      if self._tasks is None:
        raise ValueError('reset(sync=False): a task should be first set')
    if mask is not None:
      ptrs, hmask = self._mask_ptrs(mask)   # (checked before anything changes)
    self._episode += 1
    if seed is not None:
      self._base_seed = int(seed)
      self._seeds = int(seed) + np.arange(self.n_envs, dtype=np.int64)
      self._key_device()
    else:
      # the reference's single env moves to seed + 1 (safe_adaptation_gym.py:97-101);
      # a batch moves every env past the whole batch so episodes never share a seed.
      self._seeds = self._seeds + self.n_envs
    self._rs = None
    if options is not None and 'task' in options:
      self.set_task(options['task'])
      return self._observe()
    if not sync:
      bufs = self._dev_bufs()
      for k, (c, b) in enumerate(zip(self._ctx, bufs)):
        d_mask = None if ptrs is None else nat.C.c_void_p(ptrs[k])
        if self._rgb_observation:
          # no vector observation is returned, so none is formed (the Doggo's is a pass over the whole batch); the image
          # needs the state alone
          c.reset_device_async(d_mask, None)
          c.render_rows_device(d_mask if self._img_valid else None, b['img'])
        else:
          c.reset_device_async(d_mask, b['obs'])
      if self._rgb_observation:
        self._img_valid = True
      outs = [self._views(k)[0] for k in range(len(self._ctx))]
      return outs[0] if len(outs) == 1 else outs
    if self.device_reset:
      if mask is not None:
        return self._reset_masked(ptrs, hmask)
      self._reset_device(first_episode=False)
      if self._track:
        self._map(lambda c, s, e: c.episode_clear())
      return self._observe()
    self._pull_task_state()
    self._build_world(first_episode=False)
    return self._observe()

  def reset_counts(self, clear=False):
    """(envs reset, envs whose layout could not be sampled) by reset(sync=False) / auto_reset since the last clear,
    summed over the shards.  Joins the streams."""
    outs = [c.reset_counts(clear) for c in self._ctx]
    return sum(o[0] for o in outs), sum(o[1] for o in outs)

  def fork(self, src, same_stream=False, source=None):
    """Env i takes the complete state of env src[i] of `source` (default: this env) on the device (sag_fork_device): no
    record leaves the GPU.  For shooting planners (every real env broadcast to K candidates), evaluation of many action
    sequences from one state, rewinding to a saved state (fork into a second env of the same size, fork back) and cloning
    the best members of a population.  Needs device_reset=True (throughput mode).

    src: an int array [n_envs] of global env indices into `source`, negative = keep the env as it is; or, already on the
    device, one int32 array [n_shard] per shard with shard-LOCAL indices (a DeviceArray or any torch / cupy
    array on the shard's device; a list when there are several shards).  A host src is checked before anything is
    launched - ValueError for a wrong shape or dtype, an index out of range, a source that the same call overwrites
    (src[src[i]] must be negative or src[i] itself) and a source on another shard than its destination.  A device src is
    downloaded once (4 B per env and a join of the stream) so that the host mirrors follow; there the device rejects what
    a host src would raise for, env by env: fork_counts().
    source: another env of the same robot, devices, task descriptors and world config; shard k forks from its shard k.
    same_stream: the copy also takes the source's env id, so both draw the same action noise and in-step numbers from
    the next step on and sample the same next layout (common random numbers); otherwise a copy keeps its own stream.

    info['bound'], the task mirrors and, with host buffers, the last observation row follow the fork.  With
    device_buffers=True the call does not wait (the next wait() or synchronous step joins it), and the views returned by
    the last step() are not touched: a caller that needs the copies' rows gathers them itself (obs[src]); the next step
    writes them anyway."""
    if not self.device_reset or self.parity_rng:
      raise ValueError('fork() needs device_reset=True (throughput mode)')
    other = self if source is None else source
    if other is not self:
      if not isinstance(other, BatchedSafeAdaptationGym) or not other.device_reset or other.parity_rng:
        raise ValueError('fork(source=...): an env made with device_reset=True')
      if other.robot.name != self.robot.name or other.devices != self.devices:
        raise ValueError('fork(source=...): another robot or other devices')
    if self._tasks is None or other._tasks is None:
      raise ValueError('fork(): a task should be first set (in both envs)')
    if other is not self and (other._descs != self._descs or
                              bytes(nat.world_config(other.base_config)) != bytes(nat.world_config(self.base_config))):
      raise ValueError('fork(source=...): the envs differ in their task descriptors or world config')
    on_device = nat.is_device_array
    dsrc = None
    if isinstance(src, (list, tuple)) and len(src) == len(self._ctx) and all(on_device(x) for x in src):
      dsrc = list(src)
    elif on_device(src):
      if len(self._ctx) != 1:
        raise ValueError(f'{len(self._ctx)} shards: pass one device src per shard')
      dsrc = [src]
    if dsrc is not None:
      ptrs = [nat.device_pointer(x, (e - s,), c.device, np.int32) for c, (s, e), x in zip(self._ctx, self._ranges, dsrc)]
      local = [c.dev_download(nat.C.c_void_p(p), (e - s,), np.int32) for c, (s, e), p in zip(self._ctx, self._ranges, ptrs)]
    else:
      h = np.asarray(src)
      if h.shape != (self.n_envs,) or h.dtype.kind not in 'iu':
        raise ValueError(f'src: integers of shape ({self.n_envs},), not {h.dtype} {h.shape}')
      h = h.astype(np.int64)
      if (h >= other.n_envs).any():
        raise ValueError(f'src: index {int(h.max())} out of range ({other.n_envs} envs in the source)')
      local = []
      for (s, e), (ss, se) in zip(self._ranges, other._ranges):
        part = h[s:e]
        if ((part >= 0) & ((part < ss) | (part >= se))).any():
          raise ValueError('src: a source on another shard than its destination')
        local.append(np.where(part < 0, -1, part - ss).astype(np.int32))
    # the commit rule of the device (include/sag.h), per shard
    commit = []
    for k, loc in enumerate(local):
      n_src = other._ranges[k][1] - other._ranges[k][0]
      ok = (loc >= 0) & (loc < n_src)
      if other is self:
        j = np.where(ok, loc, 0)
        jj = loc[j]
        ok &= (j == np.arange(len(loc))) | (jj < 0) | (jj == j)
      if dsrc is None and (ok != (loc >= 0)).any():
        raise ValueError('src: a source env is itself overwritten by this call')
      commit.append(ok)
    if dsrc is None:
      if self._fork_bufs is None:
        self._fork_bufs = [o.alloc('fork', 4 * (e - s)) for o, (s, e) in zip(self._own, self._ranges)]
      for c, buf, loc in zip(self._ctx, self._fork_bufs, local):
        c.dev_upload(buf, loc)
      ptrs = [buf.value for buf in self._fork_bufs]
    for c, oc, p in zip(self._ctx, other._ctx, ptrs):
      c.fork_device(nat.C.c_void_p(p), oc, same_stream=same_stream)
    self._img_valid = False
    # host mirrors
    dst = np.concatenate([np.flatnonzero(ok) + s for ok, (s, e) in zip(commit, self._ranges)])
    frm = np.concatenate([loc[ok].astype(np.int64) + ss for loc, ok, (ss, se) in zip(local, commit, other._ranges)])
    if dst.size:
      self._bounds = self._bounds.copy()
      self._bounds[dst] = other._bounds[frm]
      tasks = list(self._tasks)
      for i, j in zip(dst.tolist(), frm.tolist()):
        tasks[i] = other._tasks[j]
      self._tasks = tasks
      self._task_ids[dst] = other._task_ids[frm]
      self._desc_of_env[dst] = other._desc_of_env[frm]
      self._reward_dim = max(t.REWARD_DIM for t in self._tasks)
      if self._last_obs is not None and other._last_obs is not None:
        rows = other._last_obs[frm]
        self._last_obs[dst] = rows
    if not self.device_buffers:
      self.wait()

  def fork_counts(self, clear=False):
    """(envs copied, envs rejected) by fork() since the last clear, summed over the shards.  Joins the streams."""
    outs = [c.fork_counts(clear) for c in self._ctx]
    return sum(o[0] for o in outs), sum(o[1] for o in outs)

  def step(self, action, sync=True):
    """-> (obs [N, obs_dim] f32, reward [N] (or [N, 2]) f32, done [N] bool,
    info {'cost': [N] f32, 'bound': [N] f32, 'goal_met': [N] bool})

    With device_buffers=True the step is enqueued with sag_step_device and the same tuple comes back as
    _native.DeviceArray views of HBM (obs f32, reward f32, done / cost / goal_met uint8 flags; `bound` stays a host
    array): no copy in either direction.  `action` may be a host array (uploaded) or a device array - a DeviceArray or
    anything that exports the CUDA array interface, e.g. a torch tensor on the GPU - of shape [N, nu] float32 (one per shard, in
    a list, when the batch is sharded over several `devices`; the results are then lists, one entry per shard).
    sync=False returns as soon as the launches are enqueued on the contexts' streams: call env.wait() before the
    results are read on another stream.  The views are overwritten by the next step.

    time_limit=T: every step also runs the episode tracker on the stream.  `done` is then the `ended` byte - 0, 1
    (terminated: the step's own done flag) or 2 (truncated: the episode reached T steps) -, info['terminated'] the step's
    own done flags and info['episode'] a [N, 4] float32 device view: return, cost, length and goals met of each env's
    last finished episode (rows of envs that have not finished one are zero).
    auto_reset=True (time_limit=None: no limit): after the tracker the envs that ended are reset on the stream, and
    their rows of the returned observation are the FIRST observation of the new episode; reward, cost and goal_met are
    the final transition's.
    final_observation=True (needs auto_reset): between the tracker and the reset the observation rows of the envs that ended
    are copied on the stream (sag_copy_rows_device), and info['final_observation'] is a device view of that buffer, shaped as
    `obs` (a list of views, one per shard, when the batch is sharded).  The rows of envs whose `done` is non-zero in this
    step hold the observation of the state the final transition reached - what a learner bootstraps from after a
    truncation.  Every other row keeps what it held: zeros until the env first ends an episode, then the final observation
    of its most recent one (as info['episode']).  The view is overwritten by the next step.  An env whose resampling fails
    keeps its state: its observation row and its final row are then the same.

    rgb_observation=True (the loop turned on with episode_loop()): `obs` is the image view [N, 64, 64, 3] uint8 and the
    same contract holds.  With time_limit alone the stream runs step, render, tracker: the image is the final observation.
    With auto_reset it runs step, tracker, reset of the ended envs (no vector observation is formed), then one render of
    the whole batch: each env is rendered once per step and an ended env's image is the first of its new episode.  With
    final_observation the envs that ended, and only they, are rendered a second time: before the reset, into their rows of
    info['final_observation'] ([N, 64, 64, 3] uint8, sag_render_rows_device)."""
    if self.device_buffers:
      return self._step_device(action, sync)
    a = np.asarray(action, np.float32).reshape(self.n_envs, self.robot.nu)
    noise = tapes = None
    if self.parity_rng:
      noise = np.stack([rs.normal(size=self.robot.nu) for rs in self.rs]).astype(np.float32)
      tapes = np.stack([_peek_words(rs, TAPE_WORDS) for rs in self.rs])
    outs = self._map(lambda c, s, e: c.step(a[s:e], None if noise is None else noise[s:e],
                                            None if tapes is None else tapes[s:e]))
    obs = np.concatenate([o[0] for o in outs])
    if self._rgb_observation:
      obs = self._render_rgb()
    rew = np.concatenate([o[1] for o in outs])
    cost = np.concatenate([o[2] for o in outs]).astype(np.float32)
    done = np.concatenate([o[3] for o in outs]).astype(bool)
    met = np.concatenate([o[4] for o in outs]).astype(bool)
    if self.parity_rng:
      used = np.concatenate([o[5] for o in outs])
      for rs, n in zip(self.rs, used):
        if n > TAPE_WORDS:
          raise RuntimeError('in-step random draws exceeded the tape; raise TAPE_WORDS')
        if n:
          rs.randint(0, 2**32, size=int(n), dtype=np.uint32)
    reward = rew if self._reward_dim == 2 else rew[:, 0]
    info = {'cost': cost, 'bound': self._bounds, 'goal_met': met}
    if self.device_reset:
      self._last_obs = obs.copy()
    return obs, reward, done, info

  # -- device-resident path (device_buffers=True) ---------------------------------------------------
  def _dev_bufs(self):
    if self._dev is None:
      self._dev = []
      od, nu = self.robot.obs_dim, self.robot.nu
      for own, (s, e) in zip(self._own, self._ranges):
        n = e - s
        sizes = {'act': n * nu * 4, 'obs': n * od * 4, 'rew': n * 2 * 4, 'cost': n, 'done': n, 'met': n}
        b = {k: own.alloc(k, nbytes) for k, nbytes in sizes.items()}
        if self._track:
          b['ended'], b['episode'] = own.alloc('ended', n, zero=True), own.alloc('episode', n * 16, zero=True)
        if self._rgb_observation:
          b['img'] = own.alloc('img', n * 64 * 64 * 3)
        if self.final_observation:
          b['final'] = own.alloc('final', n * 64 * 64 * 3 if self._rgb_observation else n * od * 4, zero=True)
        self._dev.append(b)
    return self._dev

  def _views(self, k):
    c, (s, e), b = self._ctx[k], self._ranges[k], self._dev[k]
    n = e - s
    A = nat.DeviceArray
    if self._rgb_observation:
      obs = A(c, b['img'].value, (n, 64, 64, 3), np.uint8)
    else:
      obs = A(c, b['obs'].value, (n, self.robot.obs_dim), np.float32)
    rew = (A(c, b['rew'].value, (n, 2), np.float32) if self._reward_dim == 2 else
           A(c, b['rew'].value, (n,), np.float32, strides=(8,), base=(b['rew'].value, (n, 2))))
    return obs, rew, A(c, b['done'].value, (n,), np.uint8), A(c, b['cost'].value, (n,), np.uint8), A(c, b['met'].value, (n,), np.uint8)

  def _step_device(self, action, sync):
    bufs = self._dev_bufs()
    on_device = nat.is_device_array
    if isinstance(action, (list, tuple)) and len(action) == len(self._ctx) and all(on_device(x) for x in action):
      acts = list(action)          # one device array per shard
    elif on_device(action):
      if len(self._ctx) != 1:
        raise ValueError(f'{len(self._ctx)} shards: pass one device action array per shard')
      acts = [action]
    else:                          # host actions for the whole batch: split over the shards
      a = np.asarray(action, np.float32).reshape(self.n_envs, self.robot.nu)
      acts = [a[s:e] for s, e in self._ranges]
    ptrs = [nat.device_pointer(a, (e - s, self.robot.nu), c.device) if on_device(a) else None
            for c, (s, e), a in zip(self._ctx, self._ranges, acts)]   # every shard's actions checked before any launch
    for c, b, a, p in zip(self._ctx, bufs, acts, ptrs):
      if p is not None:
        d_act = nat.C.c_void_p(p)
      else:
        c.dev_upload(b['act'], np.ascontiguousarray(a, np.float32))
        d_act = b['act']
      c.step_device(d_act, None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
      rgb = self._rgb_observation
      if rgb and not self.auto_reset:   # (before the tracker: the final image of an episode that ends here)
        c.render_rgb_device(b['img'])
      if self._track:
        c.episode_track(b['rew'], b['cost'], b['done'], b['met'], self.time_limit or 0, b['ended'], b['episode'])
        if self.final_observation:   # (before the reset: the state, and the observation rows, of the final transition)
          if rgb:
            c.render_rows_device(b['ended'], b['final'])
          else:
            c.copy_rows(b['ended'], self.robot.obs_dim * 4, b['obs'], b['final'])
        if self.auto_reset:   # every env is rendered once, after the resets: an ended env shows its new episode
          c.reset_device_async(b['ended'], None if rgb else b['obs'])
          if rgb:
            c.render_rgb_device(b['img'])
    if self._rgb_observation:
      self._img_valid = True
    if sync:
      self.wait()
    outs = [self._views(k) for k in range(len(self._ctx))]
    one = len(outs) == 1
    pick = (lambda j: outs[0][j]) if one else (lambda j: [o[j] for o in outs])
    info = {'cost': pick(3), 'bound': self._bounds, 'goal_met': pick(4)}
    if not self._track:
      return pick(0), pick(1), pick(2), info
    A = nat.DeviceArray
    ended = [A(c, b['ended'].value, (e - s,), np.uint8) for c, b, (s, e) in zip(self._ctx, bufs, self._ranges)]
    episode = [A(c, b['episode'].value, (e - s, 4), np.float32) for c, b, (s, e) in zip(self._ctx, bufs, self._ranges)]
    info.update(terminated=pick(2), episode=episode[0] if one else episode)
    if self.final_observation:
      final = [A(c, b['final'].value, o[0].shape, o[0].dtype) for c, b, o in zip(self._ctx, bufs, outs)]
      info['final_observation'] = final[0] if one else final
    return pick(0), pick(1), ended[0] if one else ended, info

  def wait(self):
    """Joins the contexts' streams (after step(sync=False))."""
    for c in self._ctx:
      c.wait()

  def _render_rgb(self):
    return np.concatenate(self._map(lambda c, s, e: c.render_rgb()))

  def render(self, mode='human', envs=None, **options):
    """Images of every env from one of the scene's cameras, ray-cast on the device: [N, height, width, 3] uint8.
    Options as the reference passes to physics.render (render_options: camera_id 'vision' | 'fixednear' |
    'fixedfar' | 'track', height, width); defaults 'fixedfar', 256 x 256.  There is no window: mode 'human' and
    'rgb_array' both return the array (a viewer can show it).

    envs: a 1-D integer sequence of global env indices, any order, duplicates allowed -> [len(envs), height, width, 3] in
    that order (sag_render_envs).  Only these envs are ray-cast, staged and copied: each shard renders its own entries and
    a shard with none launches nothing.  ValueError, before anything is launched, for an index outside [0, n_envs), a
    dtype that is not an integer (bool included) and an array that is not 1-D.

    depth=True -> [N, height, width] float32: the distance of the nearest surface (translucent ones included) from the
    camera plane in metres; sky pixels hold 50.0 (Context.DEPTH_SKY).  segmentation=True -> [N, height, width, 2] int32:
    (instance, class) of that surface, mirroring dm_control's (objid, objtype) with the classes of include/sag.h enum
    sag_seg_class; the sky is (-1, -1).  Both true: ValueError, as dm_control, before anything is launched."""
    opt = dict(self._render_options)
    opt.update(options)
    cam, h, w = opt.get('camera_id', 'fixedfar'), int(opt.get('height', 256)), int(opt.get('width', 256))
    if isinstance(cam, str) and cam not in nat.Context.CAMERAS:
      raise KeyError(f'unknown camera {cam!r}: one of {sorted(nat.Context.CAMERAS)}')
    if opt.get('depth') and opt.get('segmentation'):
      raise ValueError('render: depth and segmentation are mutually exclusive')
    output = 'depth' if opt.get('depth') else ('segmentation' if opt.get('segmentation') else 'rgb')
    tail, dtype = {'rgb': ((3,), np.uint8), 'depth': ((), np.float32), 'segmentation': ((2,), np.int32)}[output]
    ov = self._render_lidars_and_collision
    if envs is None:
      return np.concatenate(self._map(lambda c, s, e: c.render(cam, w, h, overlays=ov, output=output)))
    ids = np.asarray(envs)
    if ids.ndim != 1:
      raise ValueError(f'envs: a 1-D sequence of env indices, not shape {ids.shape}')
    if ids.size == 0:
      return np.zeros((0, h, w) + tail, dtype)
    if ids.dtype.kind not in 'iu':
      raise ValueError(f'envs: integer indices, not {ids.dtype}')
    ids = ids.astype(np.int64)
    if ids.min() < 0 or ids.max() >= self.n_envs:
      raise ValueError(f'envs: index {int(ids.min() if ids.min() < 0 else ids.max())} out of range ({self.n_envs} envs)')
    out = np.zeros((len(ids), h, w) + tail, dtype)

    def part(c, s, e):
      sel = np.flatnonzero((ids >= s) & (ids < e))
      if sel.size:
        out[sel] = c.render(cam, w, h, overlays=ov, envs=(ids[sel] - s).astype(np.int32), output=output)
    self._map(part)
    return out

  def close(self):
    for own in self._own:
      own.close()
    self._dev = self._mask_bufs = self._fork_bufs = None
    for c in self._ctx:
      c.close()
    if self._pool:
      self._pool.shutdown()

  # -- state access (checkpoint / tests) ---------------------------------------------
  def get_state(self):
    outs = self._map(lambda c, s, e: c.get_state())
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])

  def set_state(self, rec_f, rec_i):
    self._img_valid = False
    self._map(lambda c, s, e: c.set_state(rec_f[s:e], rec_i[s:e]))

  # -- internals ------------------------------------------------------------------------
  def _expand_tasks(self, task):
    if isinstance(task, type) and issubclass(task, Task):
      return [task() for _ in range(self.n_envs)]
    if isinstance(task, Task):
      return [task] + [type(task)() for _ in range(self.n_envs - 1)]
    tasks = list(task)
    assert len(tasks) == self.n_envs, 'one task per env'
    return tasks

  def _map(self, fn):
    jobs = list(zip(self._ctx, self._ranges))
    if self._pool is None:
      return [fn(c, s, e) for c, (s, e) in jobs]
    return list(self._pool.map(lambda j: fn(j[0], j[1][0], j[1][1]), jobs))

  def _build_world(self, first_episode):
    """World.sample_layout + World.reset for every env (safe_adaptation_gym.py:170-172) on the
    native sampler: env i draws from RandomState(seed_i) in the reference's order."""
    out = nat.sample_layouts(self.robot.name, self._seeds, self._desc_of_env, config=self.base_config,
                             first_episode=first_episode, want_rng=self.parity_rng, descs=self._descs)
    rf, ri, status = out[:3]
    states = out[3] if self.parity_rng else None
    if status.any():
      bad = np.flatnonzero(status)
      raise ResamplingError(f'Failed to generate layout for envs {bad[:8].tolist()} (seeds '
                            f'{self._seeds[bad[:8]].tolist()})')
    if self.parity_rng:  # continue the same streams on the host (noise, in-step draws)
      for rs, st in zip(self.rs, states):
        rs.set_state(st)
    cs = slice(nat.F_CTRL_SCALE, nat.F_CTRL_SCALE + nat.MAX_NU)
    if first_episode:  # drawn once per Task object (tasks/task.py:85-94), kept across resets
      self._ctrl_scale, self._bound0 = rf[:, cs].copy(), rf[:, nat.F_BOUND].copy()
    else:
      rf[:, cs], rf[:, nat.F_BOUND] = self._ctrl_scale, self._bound0
    if self._persist is not None:
      ri[:, nat.I_BTN_STATE] = self._persist['btn_state']
      ri[:, nat.I_CATCH_TIMER] = self._persist['catch_timer']
      rf[:, nat.F_CATCH + 2] = self._persist['catch_cur']
      rf[:, nat.F_CATCH + 3] = self._persist['catch_next']
    self._bounds = rf[:, nat.F_BOUND].copy()
    ri[:, nat.I_EPISODE] = self._episode & 0xffffff   # episode nonce of the device-side generator
    self._map(lambda c, s, e: c.set_layout(rf[s:e], ri[s:e]))

  def _reset_device(self, first_episode, masks=None):
    """World.sample_layout + World.reset on the device (sag_reset_device) for every env, or for the envs of the
    per-shard device masks (pointers).  Failures raise ResamplingError; a shard with a failure installs nothing."""
    masks = masks or [None] * len(self._ctx)
    outs = self._map(lambda c, s, e: c.reset_device(first_episode, self._episode & 0xffffff,
                                                     masks[self._ctx.index(c)]))
    bad = np.concatenate([np.flatnonzero(st) + s for (rc, st, _), (s, e) in zip(outs, self._ranges)])
    if bad.size:
      raise ResamplingError(f'Failed to generate layout for envs {bad[:8].tolist()}')
    self._bounds = np.concatenate([b for _, _, b in outs])

  def _mask_ptrs(self, mask):
    """-> (device pointer of every shard's mask bytes, the host mask as uint8 or None); ValueError for anything that is not
    a mask, before anything is reset."""
    on_device = nat.is_device_array
    if isinstance(mask, (list, tuple)) and len(mask) == len(self._ctx) and all(on_device(x) for x in mask):
      dmasks = list(mask)
    elif on_device(mask):
      if len(self._ctx) != 1:
        raise ValueError(f'{len(self._ctx)} shards: pass one device mask per shard')
      dmasks = [mask]
    else:
      dmasks = None
      hmask = np.asarray(mask)
      if hmask.shape != (self.n_envs,) or hmask.dtype not in (np.bool_, np.uint8):
        raise ValueError(f'mask: bool / uint8 of shape ({self.n_envs},), not {hmask.dtype} {hmask.shape}')
      hmask = hmask.astype(np.uint8)
    if dmasks is not None:
      return [nat.device_pointer(m, (e - s,), c.device, np.uint8) for c, (s, e), m in zip(self._ctx, self._ranges, dmasks)], None
    # a host mask travels in a buffer of each shard
    if self._mask_bufs is None:
      self._mask_bufs = [o.alloc('mask', e - s) for o, (s, e) in zip(self._own, self._ranges)]
    for c, (s, e), buf in zip(self._ctx, self._ranges, self._mask_bufs):
      c.dev_upload(buf, hmask[s:e])
    return [buf.value for buf in self._mask_bufs], hmask

  def _reset_masked(self, ptrs, hmask):
    self._reset_device(first_episode=False, masks=[nat.C.c_void_p(p) for p in ptrs])
    if self._track:
      for c, p in zip(self._ctx, ptrs):
        c.episode_clear(nat.C.c_void_p(p))
    # the observation: rows of reset envs are formed at their new state, the others are what the last step returned
    if hmask is not None:
      rows = [hmask[s:e].astype(bool) for s, e in self._ranges]
    else:
      rows = [c.dev_download(nat.C.c_void_p(p), (e - s,), np.uint8).astype(bool) for c, (s, e), p in zip(self._ctx, self._ranges, ptrs)]
    if self.device_buffers:
      bufs = self._dev_bufs()
      for c, b, r, (s, e), p in zip(self._ctx, bufs, rows, self._ranges, ptrs):
        if self._rgb_observation:   # the image is a function of the state: the kept rows hold what the step rendered
          c.render_rows_device(nat.C.c_void_p(p) if self._img_valid else None, b['img'])
        else:
          last = c.dev_download(b['obs'], (e - s, self.robot.obs_dim), np.float32)
          last[r] = c.observe()[r]
          c.dev_upload(b['obs'], last)
      self.wait()
      self._img_valid = self._rgb_observation
      outs = [self._views(k)[0] for k in range(len(self._ctx))]
      return outs[0] if len(outs) == 1 else outs
    new = self._render_rgb() if self._rgb_observation else np.concatenate(self._map(lambda c, s, e: c.observe()))
    r = np.concatenate(rows)
    if self._last_obs is None or self._rgb_observation:
      obs = new
    else:
      obs = self._last_obs.copy()
      obs[r] = new[r]
    self._last_obs = obs.copy()
    return obs

  def _pull_task_state(self):
    """Task attributes that outlive an episode in the reference because they live on
    the Task object, not in the simulator: PressButtons._state (press_buttons.py:23),
    CatchGoal radii and timer (catch_goal.py:14-18)."""
    rf, ri = self.get_state()
    self._persist = {
        'btn_state': ri[:, nat.I_BTN_STATE].copy(),
        'catch_timer': ri[:, nat.I_CATCH_TIMER].copy(),
        'catch_cur': rf[:, nat.F_CATCH + 2].copy(),
        'catch_next': rf[:, nat.F_CATCH + 3].copy(),
    }

  def _observe(self):
    if self.device_buffers:   # reset is the cold path: the observation is formed as usual and parked in the obs buffer
      bufs = self._dev_bufs()
      for c, b in zip(self._ctx, bufs):
        if self._rgb_observation:
          c.render_rgb_device(b['img'])
        else:
          c.dev_upload(b['obs'], c.observe())
      self._img_valid = self._rgb_observation
      self.wait()
      outs = [self._views(k)[0] for k in range(len(self._ctx))]
      return outs[0] if len(outs) == 1 else outs
    obs = self._render_rgb() if self._rgb_observation else np.concatenate(self._map(lambda c, s, e: c.observe()))
    if self.device_reset:
      self._last_obs = obs.copy()
    return obs


def _peek_words(rs, n):
  c = np.random.RandomState()
  c.set_state(rs.get_state())
  return c.randint(0, 2**32, size=n, dtype=np.uint32)
