"""MLPPolicy: a Gaussian actor-critic MLP whose forward runs on the env's context stream (sag_policy_forward_device).

With a RolloutBuffer it closes the model-free loop on the device - observe, policy and critics, step, track, append, reset and
GAE are all enqueued on one stream, and nothing goes through the host between them:

  buf.collect(pi)
  pi.evaluate(buf)
  buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)

The network is obs -> hidden -> hidden -> nu + 2 outputs (action mean, reward value, cost value) with a state-independent
standard deviation; include/sag.h defines its arithmetic.  NumPy only; no torch."""
import numpy as np

from safe_adaptation_gym_amd import _native as nat

ACTIVATIONS = {'relu': nat.POLICY_RELU, 'tanh': nat.POLICY_TANH}
KEYS = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'std')
F32, I32 = np.dtype('<f4'), np.dtype('<i4')


def plane_range(view, t0, t1):
  """Planes t0 ... t1 - 1 of a time-major device view (a RolloutBuffer's arrays), as a view of the same kind: what
  MLPPolicy.backward takes as one minibatch."""
  t0, t1 = int(t0), int(t1)
  if not 0 <= t0 < t1 <= view.shape[0]:
    raise ValueError(f'plane_range: planes {t0} ... {t1} of {view.shape[0]}')
  strides = view.strides if view.strides is not None else nat.dense_strides(view.shape, view.dtype)
  return type(view)(view.ctx, view.ptr + t0 * strides[0], (t1 - t0,) + tuple(view.shape[1:]), view.dtype, strides=tuple(strides),
                    base=view._base)


class MLPPolicy:
  """pi = MLPPolicy(env, hidden=64, activation='relu', seed=0, log_std=-0.5)

  env: a BatchedSafeAdaptationGym in one context with vector observations; ValueError otherwise.
  hidden: a multiple of 32 from 32 to 256.  Weights and biases are uniform in +-1 / sqrt(fan_in) from
  np.random.RandomState(seed); std = exp(log_std).

  params: {'W1' [obs_dim, hidden], 'b1', 'W2' [hidden, hidden], 'b2', 'W3' [hidden, nu + 2], 'b3', 'std' [nu]} - DeviceArray
  views of ONE device buffer in the ABI's layout, which a learner may overwrite in place on the context's stream (after writing
  'std' that way, call refresh() - the log-probability's constant is formed on the host).  set_params() / get_params() go
  through the host.

  grad: {the keys of `params`, 'stats' [8]} - DeviceArray views of ONE buffer of n_params + 8 floats that backward() fills
  (sag_policy_backward_device) and an optimiser reads in place (PPOLearner; Context.adam).

  normalize_observations=True: the policy owns running per-column moments of the observations (float64 {count, mean, M2}) and
  the float32 table made from them (mean, 1 / sqrt(var + obs_eps)) on the device, and forward / backward - hence act_into,
  evaluate, __call__ and PPOLearner - read every observation element as clamp((x - mean) * rstd, -obs_clip, obs_clip), applied
  where the kernels stage the row (sag_policy_forward_norm_device, sag_policy_backward_norm_device): no normalised copy of the
  observations is written.  The moments start empty, which is the identity table; update_obs_stats(buf) folds a rollout in
  (PPOLearner.update() does so once per update, after its last round).  So the first collect runs under the identity table
  unless update_obs_stats is called on a warm-up rollout first.  get_obs_norm() / set_obs_norm() carry the state through a
  checkpoint; obs_norm_frozen = True stops the statistics (evaluation).  With the switch off none of this exists and
  update_obs_stats / get_obs_norm / set_obs_norm raise ValueError.

  Every method but set_params / get_params / refresh / evaluate / get_obs_norm / set_obs_norm only enqueues work: no wait, no
  host copy."""

  def __init__(self, env, hidden=64, activation='relu', seed=0, log_std=-0.5, normalize_observations=False, obs_clip=10.0, obs_eps=1e-8):
    from safe_adaptation_gym_amd.envs import BatchedSafeAdaptationGym
    if not isinstance(env, BatchedSafeAdaptationGym):
      raise ValueError('MLPPolicy: env must be a BatchedSafeAdaptationGym')
    if env._rgb_observation:
      raise ValueError('MLPPolicy: rgb_observation is not supported - the network reads vector observations')
    if len(env._ctx) != 1:
      raise ValueError(f'MLPPolicy: the env is sharded over {len(env._ctx)} contexts; one policy serves one context')
    H = int(hidden)
    if H != hidden or H < 32 or H > 256 or H % 32:
      raise ValueError(f'MLPPolicy: hidden={hidden} is not a multiple of 32 from 32 to 256')
    if activation not in ACTIVATIONS:
      raise ValueError(f'MLPPolicy: activation={activation!r}: one of {sorted(ACTIVATIONS)}')
    if not np.isfinite(log_std):
      raise ValueError(f'MLPPolicy: log_std={log_std}')
    if normalize_observations and (not obs_clip > 0 or not (np.isfinite(obs_eps) and obs_eps > 0)):
      raise ValueError(f'MLPPolicy: obs_clip={obs_clip}, obs_eps={obs_eps}')
    self.normalize_observations, self.obs_clip, self.obs_eps = bool(normalize_observations), float(obs_clip), float(obs_eps)
    self.obs_norm_frozen = False
    self._obs_state = self._obs_table = None
    self.env, self.hidden, self.activation = env, H, activation
    self.obs_dim, self.nu = od, nu = env.robot.obs_dim, env.robot.nu
    self._ctx = c = env._ctx[0]
    self.draw = 0   # counter word 1 of the next sampled forward
    self.shapes = {'W1': (od, H), 'b1': (H,), 'W2': (H, H), 'b2': (H,), 'W3': (H, nu + 2), 'b3': (nu + 2,), 'std': (nu,)}
    self.n_params = sum(int(np.prod(s)) for s in self.shapes.values())
    self._own = own = nat.DeviceBuffers(c)
    self._buf = own.alloc('params', self.n_params * 4)
    self.params, off = {}, 0
    for k in KEYS:
      self.params[k] = nat.DeviceArray(c, self._buf.value + 4 * off, self.shapes[k], np.float32)
      off += int(np.prod(self.shapes[k]))
    self._gbuf = own.alloc('grad', (self.n_params + nat.POLICY_GRAD_STATS) * 4)
    self.grad, off = {}, 0
    for k in KEYS:
      self.grad[k] = nat.DeviceArray(c, self._gbuf.value + 4 * off, self.shapes[k], np.float32)
      off += int(np.prod(self.shapes[k]))
    self.grad['stats'] = nat.DeviceArray(c, self._gbuf.value + 4 * off, (nat.POLICY_GRAD_STATS,), np.float32)
    rng = np.random.RandomState(seed)
    init = {}
    for k in KEYS[:-1]:
      bound = 1.0 / np.sqrt(self.shapes['W' + k[1]][0])   # a bias takes its layer's fan-in
      init[k] = rng.uniform(-bound, bound, self.shapes[k]).astype(np.float32)
    init['std'] = np.full(nu, np.exp(log_std), np.float32)
    self.set_params(init)
    if self.normalize_observations:
      self._obs_state, self._obs_table = own.alloc('obs_state', (1 + 2 * od) * 8), own.alloc('obs_table', 2 * od * 4)
      self.set_obs_norm(0.0, np.zeros(od), np.zeros(od))   # the empty state: the identity table

  # -- parameters ------------------------------------------------------------------------------------------------------
  def set_params(self, params):
    """Uploads a dict of NumPy arrays (every key of `params`, the shapes of `shapes`)."""
    if set(params) != set(KEYS):
      raise ValueError(f'MLPPolicy.set_params: the keys are {list(KEYS)}, not {sorted(params)}')
    flat = []
    for k in KEYS:
      a = np.asarray(params[k], np.float32)
      if a.shape != self.shapes[k]:
        raise ValueError(f'MLPPolicy.set_params: {k} of shape {a.shape}, not {self.shapes[k]}')
      flat.append(a.reshape(-1))
    std = flat[-1]
    if not (np.isfinite(std).all() and (std > 0).all()):
      raise ValueError('MLPPolicy.set_params: std must be positive and finite')
    self._ctx.dev_upload(self._buf, np.concatenate(flat))
    self._set_const(std)

  def get_params(self):
    """Downloads the parameters -> dict of NumPy arrays.  Joins the stream."""
    self._ctx.wait()
    flat = self._ctx.dev_download(self._buf, (self.n_params,), np.float32)
    out, off = {}, 0
    for k in KEYS:
      n = int(np.prod(self.shapes[k]))
      out[k] = flat[off:off + n].reshape(self.shapes[k]).copy()
      off += n
    return out

  def _set_const(self, std):
    std = np.asarray(std, np.float64)
    self.logp_const = float(np.float32(np.log(std).sum() + len(std) * 0.5 * np.log(2 * np.pi)))

  def refresh(self):
    """Forms the log-probability's constant again from the 'std' on the device (after a learner wrote it in place).  Joins
    the stream."""
    self._ctx.wait()
    self._set_const(self.params['std'].numpy())

  # -- the forward -------------------------------------------------------------------------------------------------------
  def _rows(self, obs):
    """(pointer, rows, pitch in floats) of a device view [rows, obs_dim] float32 whose rows are contiguous."""
    v = nat.device_view(obs, 'MLPPolicy', self._ctx.device)
    if v.dtype != F32 or len(v.shape) != 2 or v.shape[1] != self.obs_dim:
      raise ValueError(f'MLPPolicy: observations must be float32 of shape (rows, {self.obs_dim}), not {v.dtype.str} {v.shape}')
    pitch = v.strides[0]
    if v.strides[1] != 4 or pitch < self.obs_dim * 4 or pitch % 16 or v.ptr % 16:
      raise ValueError('MLPPolicy: observation rows must be contiguous, 16-byte aligned and a multiple of 16 bytes apart')
    return v.ptr, int(v.shape[0]), pitch // 4

  def _out(self, x, shape, what):
    if x is None:
      return None
    try:
      return nat.device_pointer(x, shape, self._ctx.device)
    except ValueError as e:
      raise ValueError(f'MLPPolicy: {what}: {e}') from None

  def forward(self, obs, actions=None, logp=None, value=None, cost_value=None, deterministic=False, row0=0):
    """One fused forward of the rows of `obs` (a device view [rows, obs_dim]) into the device views that are given: actions
    [rows, nu], logp, value, cost_value [rows].  Actions are mean + std * z, unclamped - with deterministic=True, or without
    `actions`, nothing is sampled: the actions are the mean and logp = -logp_const.  `draw` advances by one per sampled call.
    row0 is added to the row index in the generator's counter (the rows of a second call that continue those of a first)."""
    ptr, rows, pitch = self._rows(obs)
    if rows < 1:
      return
    sampled = actions is not None and not deterministic
    kw = dict(logp_const=self.logp_const, d_actions=self._out(actions, (rows, self.nu), 'actions'), d_logp=self._out(logp, (rows,), 'logp'),
              d_value=self._out(value, (rows,), 'value'), d_cvalue=self._out(cost_value, (rows,), 'cost_value'),
              activation=ACTIVATIONS[self.activation], flags=0 if sampled or actions is None else nat.POLICY_MEAN,
              draw=self.draw, row0=row0, obs_pitch=pitch)
    if self.normalize_observations:
      self._ctx.policy_forward_norm(rows, self.hidden, self._buf, ptr, self._obs_table, self.obs_clip, **kw)
    else:
      self._ctx.policy_forward(rows, self.hidden, self._buf, ptr, **kw)
    if sampled:
      self.draw = (self.draw + 1) & 0xffffffff

  def __call__(self, obs, actions):
    """policy(obs[t], actions[t]): what RolloutBuffer.collect() asks of any policy."""
    self.forward(obs, actions, deterministic=getattr(self, 'deterministic', False))

  deterministic = False   # set on the object: act_into() and __call__ write the mean

  def act_into(self, buf, t):
    """The forward of buf.obs[t] into buf.actions[t], buf.logp[t], buf.value[t] and buf.cost_value[t]."""
    self.forward(buf.obs[t], buf.actions[t], buf.logp[t], buf.value[t], buf.cost_value[t], deterministic=self.deterministic)

  def evaluate(self, buf):
    """After buf.collect(pi): the values of buf.obs[T] into row T of buf.value and buf.cost_value, and the values of the rows of
    buf.final_observations() into buf.final_value and buf.final_cost_value - what buf.advantages() bootstraps from.  Joins the
    stream once (the number of final rows comes to the host)."""
    T = buf.T
    self.forward(buf.obs[T], value=buf.value[T], cost_value=buf.cost_value[T])
    rows, count = buf.final_observations()
    if count:
      fv, fcv = buf.final_value, buf.final_cost_value
      self.forward(rows, value=nat.DeviceArray(fv.ctx, fv.ptr, (count,), np.float32),
                   cost_value=nat.DeviceArray(fcv.ctx, fcv.ptr, (count,), np.float32))

  # -- the backward ------------------------------------------------------------------------------------------------------
  def _planes(self, x, tail, what):
    """(pointer, planes, rows, pitch in rows) of a time-major float32 device view [planes, rows] + tail whose rows are
    contiguous and whose planes are a whole number of rows apart."""
    v, tail = nat.device_view(x, f'MLPPolicy.backward: {what}', self._ctx.device), tuple(tail)
    if v.dtype != F32 or len(v.shape) != 2 + len(tail) or v.shape[2:] != tail:
      raise ValueError(f'MLPPolicy.backward: {what} must be float32 of shape (planes, rows{"".join(", %d" % t for t in tail)}), '
                       f'not {v.dtype.str} {v.shape}')
    row = nat.dense_strides((1,) + tail, F32)   # row[0]: the bytes of one row
    if v.strides[1:] != row or v.strides[0] % row[0] or v.strides[0] < v.shape[1] * row[0]:
      raise ValueError(f'MLPPolicy.backward: {what}: rows must be contiguous and planes a whole number of rows apart')
    return v.ptr, int(v.shape[0]), int(v.shape[1]), v.strides[0] // row[0]

  def _row_list(self, rows):
    """(pointer, count) of a row list: a contiguous device int32 view [count], or such a pair itself."""
    if isinstance(rows, tuple) and len(rows) == 2:
      p, count = rows
      p, count = int(p.value if hasattr(p, 'value') else p), int(count)
    else:
      v = nat.device_view(rows, 'MLPPolicy.backward: rows', self._ctx.device)
      if not v.contiguous:
        raise ValueError('MLPPolicy.backward: rows: the list must be contiguous')
      if v.dtype != I32 or len(v.shape) != 1:
        raise ValueError(f'MLPPolicy.backward: rows must be int32 of shape (count,), not {v.dtype.str} {v.shape}')
      p, count = v.ptr, int(v.shape[0])
    if count < 1 or p % 4:
      raise ValueError(f'MLPPolicy.backward: rows: {count} entries at a pointer that must be 4-byte aligned')
    return p, count

  def backward(self, obs, actions, logp_old, adv, ret, cadv=None, cret=None, *, clip, vf_coef, cost_vf_coef, ent_coef,
               adv_affine=(1.0, 0.0), cadv_affine=(0.0, 0.0), scale, accumulate=False, rows=None):
    """The gradient of the PPO-Lagrangian loss over stored rows into `grad` (sag_policy_backward_device; include/sag.h defines
    the loss), enqueued on the stream.  Every input is a time-major device view [planes, rows, ...] - a RolloutBuffer's obs,
    actions, logp and the views advantages() returns, or a range of their planes (plane_range) - and all must share planes, rows
    and the pitch between planes; ValueError otherwise, or for a hidden size the backward does not support (> 128).  The
    advantage is adv_affine[0] * (adv - adv_affine[1]) - cadv_affine[0] * (cadv - cadv_affine[1]); scale is 1 / (rows of the
    whole batch); accumulate=True adds to what `grad` holds.
    rows: a contiguous device int32 view [count], or (pointer, count) - the batch is then the `count` rows that the list names,
    entry e being row e % rows of plane e // rows of the views, gathered in place (sag_policy_backward_rows_device; an entry
    outside the views is a row that is absent).  A slice of the list sag_permutation_device wrote is a shuffled minibatch."""
    listed = None if rows is None else self._row_list(rows)
    if self.hidden > 128:
      raise ValueError(f'MLPPolicy.backward: hidden={self.hidden}: the backward pass supports hidden <= 128')
    given = [('obs', obs, (self.obs_dim,)), ('actions', actions, (self.nu,)), ('logp_old', logp_old, ()), ('adv', adv, ()),
             ('ret', ret, ()), ('cadv', cadv, ()), ('cret', cret, ())]
    ptr, geom = {}, None
    for name, x, tail in given:
      if x is None:
        if name not in ('cadv', 'cret'):
          raise ValueError(f'MLPPolicy.backward: {name} is required')
        ptr[name] = None
        continue
      ptr[name], *g = self._planes(x, tail, name)
      if geom is None:
        geom = g
      elif g != geom:
        raise ValueError(f'MLPPolicy.backward: {name} has (planes, rows, pitch) = {tuple(g)}, obs has {tuple(geom)}')
    if ptr['obs'] % 16:
      raise ValueError('MLPPolicy.backward: observation rows must be 16-byte aligned')
    planes, rows, pitch = geom
    args = (rows, planes, pitch, self.hidden, self._buf, ptr['obs'], ptr['actions'], ptr['logp_old'], ptr['adv'], ptr['ret'], self._gbuf, scale)
    kw = dict(d_cadv=ptr['cadv'], d_cret=ptr['cret'], clip=clip, vf_coef=vf_coef, cvf_coef=cost_vf_coef, ent_coef=ent_coef,
              adv_affine=adv_affine, cadv_affine=cadv_affine, activation=ACTIVATIONS[self.activation],
              flags=nat.POLICY_GRAD_ACCUMULATE if accumulate else 0)
    if listed is not None:
      kw['rows'] = listed
    if self.normalize_observations:
      self._ctx.policy_backward_norm(*args, self._obs_table, self.obs_clip, **kw)
    else:
      self._ctx.policy_backward(*args, **kw)

  # -- observation normalisation -----------------------------------------------------------------------------------------
  def _need_norm(self, who):
    if not self.normalize_observations:
      raise ValueError(f'MLPPolicy.{who}: the policy was built without normalize_observations=True')

  def update_obs_stats(self, rows):
    """Folds observation rows into the running moments and rewrites the table (sag_obs_stats_device), enqueued on the stream.
    `rows`: a RolloutBuffer - its stored steps buf.obs[0:T], without the row of the last observation - or any time-major
    float32 device view [planes, rows, obs_dim].  Does nothing while obs_norm_frozen is set."""
    self._need_norm('update_obs_stats')
    if self.obs_norm_frozen:
      return
    obs = plane_range(rows.obs, 0, rows.T) if hasattr(rows, 'obs') and hasattr(rows, 'T') else rows
    ptr, planes, n, pitch = self._planes(obs, (self.obs_dim,), 'obs')
    if ptr % 16:
      raise ValueError('MLPPolicy.update_obs_stats: observation rows must be 16-byte aligned')
    self._ctx.obs_stats(self._obs_state, self._obs_table, ptr, n, planes, pitch, eps=self.obs_eps)

  def get_obs_norm(self):
    """-> {'count': float, 'mean': [obs_dim], 'var': [obs_dim]} as float64 NumPy (var = M2 / count, the population variance; zeros
    while the state is empty).  Joins the stream."""
    self._need_norm('get_obs_norm')
    self._ctx.wait()
    od = self.obs_dim
    s = self._ctx.dev_download(self._obs_state, (1 + 2 * od,), np.float64)
    n = float(s[0])
    return {'count': n, 'mean': s[1:1 + od].copy(), 'var': s[1 + od:] / n if n > 0 else np.zeros(od)}

  def set_obs_norm(self, count, mean=None, var=None):
    """Uploads a state - set_obs_norm(count, mean, var) or set_obs_norm(the dict of get_obs_norm()) - and rewrites the table from
    it on the device (SAG_OBS_STATS_TABLE_ONLY), so that a restored table comes from the same arithmetic as a running one."""
    self._need_norm('set_obs_norm')
    if isinstance(count, dict):
      count, mean, var = count['count'], count['mean'], count['var']
    od = self.obs_dim
    n, mean, var = float(count), np.asarray(mean, np.float64), np.asarray(var, np.float64)
    if mean.shape != (od,) or var.shape != (od,) or not n >= 0 or not np.isfinite(mean).all() or not (np.isfinite(var).all() and (var >= 0).all()):
      raise ValueError(f'MLPPolicy.set_obs_norm: count >= 0, mean and var >= 0 of shape ({od},), all finite')
    self._ctx.dev_upload(self._obs_state, np.concatenate([[n], mean, var * n]))
    self._ctx.obs_stats(self._obs_state, self._obs_table, eps=self.obs_eps, table_only=True)

  def close(self):
    self._own.close()
    self._buf = self._gbuf = self._obs_state = self._obs_table = self._ctx = None
