"""PPOLearner: the PPO-Lagrangian update of an MLPPolicy from a RolloutBuffer, on the env's context stream.

  buf.collect(pi); pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  stats = learner.update(out)

Every round is two enqueued calls - the gradient of one minibatch read in place from the buffer's views
(sag_policy_backward_device) and one Adam step on the policy's parameters (sag_adam_device), with the global-norm clip
(sag_grad_clip_device) between them where asked for; the advantage's moments, the Lagrange multiplier's step and the mixed
advantage (sag_moments_device, sag_lagrange_device, sag_advantage_mix_device) are enqueued once ahead of the rounds and stay on
the device.  With shuffle=True every epoch starts with one more enqueued call, the permutation of all T x N rows
(sag_permutation_device), and a round's minibatch is a slice of it (sag_policy_backward_rows_device).  The update joins the
stream once, at its end.  NumPy only; no torch."""
import numpy as np

from safe_adaptation_gym_amd import _native as nat
from safe_adaptation_gym_amd.policy import plane_range

STATS = ('policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl', 'clip_fraction')
COST_ADVANTAGE = {'raw': nat.ADV_RAW, 'center': nat.ADV_CENTER, 'standardize': nat.ADV_STANDARDIZE}
# the learner's device words: the moments of adv, cadv and the ended episodes' costs, the multiplier's state, the clip's output
_ADV_MOM, _CADV_MOM, _EP_MOM, _LAG, _CLIP, _WORDS = 0, 4, 8, 12, 16, 20
MOMENTS_EPS = 1e-8


class PPOLearner:
  """learner = PPOLearner(pi, buf, lr=3e-4, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0,
                          cost_weight=0.0, betas=(0.9, 0.999), eps=1e-8, std_min=1e-3, normalize_advantage=False,
                          cost_advantage='center', max_grad_norm=None, cost_budget=None, lagrange_lr=0.05, lagrange_max=inf,
                          update_obs_stats=True, shuffle=False, shuffle_draw=0)

  pi: an MLPPolicy (hidden <= 128), buf: a RolloutBuffer of the same env.  The learner owns the Adam moments and the step count.

  update(out): `out` is what buf.advantages() returned.  epochs x minibatches rounds of backward then Adam; a minibatch is a
  contiguous range of the buffer's T planes (sizes differ by at most one; ValueError if minibatches > T), the old
  log-probabilities are buf.logp, the advantage is adv - cost_weight * cadv (without a cost channel in `out`: adv), and std is
  kept at or above std_min.  Then pi.refresh() - the update's single host join - and the statistics of the last minibatch come
  back as floats: policy_loss, value_loss, cost_value_loss, approx_kl, clip_fraction.

  Three switches, each off by default (then update() enqueues the two calls per round above and nothing else):
    normalize_advantage=True   the reward advantage is standardised over the whole T x N of `out` - (adv - mean) / (std + 1e-8),
                               moments taken once per update() - and the cost advantage is centred (cost_advantage='center',
                               the safety-starter-agents convention), standardised ('standardize') or left alone ('raw').
                               Statistics: adv_mean, adv_std.
    max_grad_norm=g            every round's gradient is scaled by min(1, g / (norm + 1e-6)) ahead of Adam.  Statistic:
                               grad_norm, the last round's norm before the clip.
    cost_budget=d              the Lagrange multiplier lives on the device and takes one step per update(), ahead of the rounds:
                               cost_weight = clip(cost_weight + lagrange_lr * (mean cost - d), 0, lagrange_max), the mean over
                               the episodes that ended inside the buffer (buf.episode[..., 1] where buf.done); no step where
                               none ended.  Statistics: cost_weight (the value this update used), episode_cost, episodes.
                               The constructor's cost_weight is the initial value; learner.cost_weight reads the value cached
                               at the last join, and assigning to it uploads.
  Without cost_budget, cost_weight is a plain attribute and stays what it was set to.

  A policy built with normalize_observations=True normalises inside its backward pass (sag_policy_backward_norm_device), and
  update() enqueues pi.update_obs_stats(buf) once, after the last round and ahead of pi.refresh(): collect, evaluate and every
  epoch of one update see one table - so buf.logp and the first epoch's ratio agree - and the next collect sees statistics
  that include this batch.  Still one host join per update.  The very first collect runs under the identity table unless
  pi.update_obs_stats() was called on a warm-up rollout.  update_obs_stats=False turns the hook off; so does
  pi.obs_norm_frozen.  With a policy that does not normalise, update() enqueues what it did before.

  shuffle=True draws every epoch's minibatches from a fresh random permutation of all n = T x N stored rows, as a textbook
  PPO does, instead of cutting the buffer into ranges of planes: the learner owns an int32 device array of n entries, every
  epoch enqueues one sag_permutation_device(n, shuffle_draw) into it and advances shuffle_draw by one, and minibatch m is the
  list slice [n m // M, n (m + 1) // M), read in place through sag_policy_backward_rows_device with scale = 1 / its length -
  no upload, no gathered copy (ValueError if minibatches > T x N).  learner.shuffle_draw is the next epoch's draw: save it
  with a checkpoint and pass it back as shuffle_draw= (or assign it) to continue the same sequence of permutations.  The
  permutation is a keyed pseudo-random one under the env's seed (include/sag.h).  Everything else - the mixed advantage, the
  clip, Adam, the observation statistics, the single host join - is as without it; ranges() describes shuffle=False only."""

  def __init__(self, pi, buf, lr=3e-4, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0,
               cost_weight=0.0, betas=(0.9, 0.999), eps=1e-8, std_min=1e-3, normalize_advantage=False, cost_advantage='center',
               max_grad_norm=None, cost_budget=None, lagrange_lr=0.05, lagrange_max=float('inf'), update_obs_stats=True,
               shuffle=False, shuffle_draw=0):
    self.update_obs_stats = bool(update_obs_stats)
    self.shuffle, self.shuffle_draw = bool(shuffle), int(shuffle_draw) & 0xffffffff
    if buf.env is not pi.env:
      raise ValueError('PPOLearner: the policy and the buffer belong to different envs')
    if pi.hidden > 128:
      raise ValueError(f'PPOLearner: hidden={pi.hidden}: the backward pass supports hidden <= 128')
    epochs, minibatches = int(epochs), int(minibatches)
    if epochs < 1 or minibatches < 1:
      raise ValueError(f'PPOLearner: epochs={epochs}, minibatches={minibatches}')
    if self.shuffle and buf.T * buf.N >= 2**31:
      raise ValueError(f'PPOLearner: shuffle=True over {buf.T} x {buf.N} rows: the row list is int32')
    if self.shuffle and pi.normalize_observations and not np.isfinite(pi.obs_clip):
      raise ValueError('PPOLearner: shuffle=True with a normalising policy needs a finite obs_clip (sag_policy_backward_rows_device)')
    if minibatches > (buf.T * buf.N if self.shuffle else buf.T):
      raise ValueError(f'PPOLearner: minibatches={minibatches} of a buffer of T={buf.T} planes' +
                       (f' x N={buf.N} rows' if self.shuffle else ''))
    if not (0 < clip < 1) or not lr > 0 or not eps > 0 or not std_min > 0 or not all(0 <= b < 1 for b in betas):
      raise ValueError(f'PPOLearner: lr={lr}, clip={clip}, betas={betas}, eps={eps}, std_min={std_min}')
    if cost_advantage not in COST_ADVANTAGE:
      raise ValueError(f"PPOLearner: cost_advantage={cost_advantage!r}: 'center', 'standardize' or 'raw'")
    if max_grad_norm is not None and not (np.isfinite(max_grad_norm) and max_grad_norm > 0):
      raise ValueError(f'PPOLearner: max_grad_norm={max_grad_norm}')
    if cost_budget is not None and not (np.isfinite(cost_budget) and np.isfinite(lagrange_lr) and lagrange_lr >= 0 and lagrange_max >= 0):
      raise ValueError(f'PPOLearner: cost_budget={cost_budget}, lagrange_lr={lagrange_lr}, lagrange_max={lagrange_max}')
    self.pi, self.buf = pi, buf
    self.lr, self.clip, self.epochs, self.minibatches = float(lr), float(clip), epochs, minibatches
    self.vf_coef, self.cost_vf_coef, self.ent_coef = float(vf_coef), float(cost_vf_coef), float(ent_coef)
    self.betas, self.eps, self.std_min = (float(betas[0]), float(betas[1])), float(eps), float(std_min)
    self.normalize_advantage, self.cost_advantage = bool(normalize_advantage), cost_advantage
    self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
    self.cost_budget = None if cost_budget is None else float(cost_budget)
    self.lagrange_lr, self.lagrange_max = float(lagrange_lr), float(lagrange_max)
    self.t = 0   # Adam steps taken
    self._ctx = c = pi._ctx
    n = pi.n_params
    self._own = own = nat.DeviceBuffers(c)
    self._m, self._v = own.alloc('m', n * 4, zero=True), own.alloc('v', n * 4, zero=True)
    self._words = self._mixed = self._index = None
    if self.shuffle:
      self._index = own.alloc('index', buf.T * buf.N * 4)   # [T x N] int32: the epoch's permutation
    if self.normalize_advantage or self.max_grad_norm is not None or self.cost_budget is not None:
      self._words = own.alloc('words', _WORDS * 4, zero=True)
    if self._mixes():
      self._mixed = own.alloc('mixed', buf.T * buf.P * 4)   # [T][P]: the advantage the backward pass is given
    self.cost_weight = float(cost_weight)

  def _mixes(self):
    return self.normalize_advantage or self.cost_budget is not None

  def _word(self, k):
    return self._words.value + 4 * k

  @property
  def cost_weight(self):
    return self._cost_weight

  @cost_weight.setter
  def cost_weight(self, value):
    self._cost_weight = float(value)
    if self.cost_budget is not None:
      self._ctx.dev_upload(self._word(_LAG), np.array([value], np.float32))

  def _prepare(self, out, cost):
    """The calls ahead of the rounds: moments, the multiplier's step, the mixed advantage -> the view the rounds read."""
    buf, c = self.buf, self._ctx
    ptr, planes, rows, pitch = self.pi._planes(out['adv'], (), 'adv')
    if (planes, rows, pitch) != (buf.T, buf.N, buf.P):
      raise ValueError(f'PPOLearner.update: adv has (planes, rows, pitch) = {(planes, rows, pitch)}, the buffer {(buf.T, buf.N, buf.P)}')
    cptr = None
    if cost:
      cptr, *g = self.pi._planes(out['cadv'], (), 'cadv')
      if tuple(g) != (planes, rows, pitch):
        raise ValueError(f'PPOLearner.update: cadv has (planes, rows, pitch) = {tuple(g)}, adv has {(planes, rows, pitch)}')
    adv_mode = nat.ADV_STANDARDIZE if self.normalize_advantage else nat.ADV_RAW
    cadv_mode = COST_ADVANTAGE[self.cost_advantage] if self.normalize_advantage and cost else nat.ADV_RAW
    if adv_mode:
      c.moments(rows, planes, pitch, ptr, self._word(_ADV_MOM), eps=MOMENTS_EPS)
    if cadv_mode:
      c.moments(rows, planes, pitch, cptr, self._word(_CADV_MOM), eps=MOMENTS_EPS)
    if self.cost_budget is not None:
      c.moments(buf.N, buf.T, buf.P, buf.episode.ptr + 4, self._word(_EP_MOM), d_mask=buf.done.ptr, stride=4, eps=MOMENTS_EPS)
      c.lagrange(self._word(_EP_MOM), self._word(_LAG), self.lagrange_lr, self.cost_budget, self.lagrange_max)
    c.advantage_mix(rows, planes, pitch, ptr, self._mixed, d_cadv=cptr, adv_mode=adv_mode, cadv_mode=cadv_mode,
                    d_adv_mom=self._word(_ADV_MOM), d_cadv_mom=self._word(_CADV_MOM),
                    d_lambda=self._word(_LAG) if self.cost_budget is not None else None, cost_weight=self._cost_weight)
    p = self._mixed.value
    return type(out['adv'])(c, p, (planes, rows), np.float32, strides=(pitch * 4, 4), base=(p, (planes, pitch)))

  def ranges(self):
    """The minibatches as (first plane, one past the last)."""
    T, M = self.buf.T, self.minibatches
    edges = [T * i // M for i in range(M + 1)]
    return list(zip(edges[:-1], edges[1:]))

  def step_size(self, t):
    b1, b2 = self.betas
    return float(np.float32(self.lr * np.sqrt(1.0 - b2**t) / (1.0 - b1**t)))

  def update(self, out):
    pi, buf, c = self.pi, self.buf, self._ctx
    if 'adv' not in out or 'ret' not in out:
      raise ValueError("PPOLearner.update: pass the dict of buf.advantages(): 'adv', 'ret' and, with a cost channel, 'cadv', 'cret'")
    cost = 'cadv' in out and 'cret' in out
    b1, b2 = self.betas
    mixed = self._prepare(out, cost) if self._mixes() else None
    n, M = buf.T * buf.N, self.minibatches
    for _ in range(self.epochs):
      if self.shuffle:   # minibatch m: entries n m // M ... n (m + 1) // M - 1 of this epoch's permutation, over all T planes
        c.permutation(n, self.shuffle_draw, self._index)
        self.shuffle_draw = (self.shuffle_draw + 1) & 0xffffffff
        rounds = [(0, buf.T, (self._index.value + 4 * (n * m // M), n * (m + 1) // M - n * m // M)) for m in range(M)]
      else:
        rounds = [(t0, t1, None) for t0, t1 in self.ranges()]
      for t0, t1, rows in rounds:
        cut = lambda v: plane_range(v, t0, t1)   # noqa: E731
        kw = dict(scale=1.0 / ((t1 - t0) * buf.N)) if rows is None else dict(scale=1.0 / rows[1], rows=rows)
        if mixed is None:
          pi.backward(cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(out['adv']), cut(out['ret']),
                      cut(out['cadv']) if cost else None, cut(out['cret']) if cost else None, clip=self.clip, vf_coef=self.vf_coef,
                      cost_vf_coef=self.cost_vf_coef, ent_coef=self.ent_coef, adv_affine=(1.0, 0.0), cadv_affine=(self.cost_weight, 0.0),
                      **kw)
        else:   # the cost advantage is inside `mixed`; the cost critic still learns from cret
          pi.backward(cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(mixed), cut(out['ret']), None, cut(out['cret']) if cost else None,
                      clip=self.clip, vf_coef=self.vf_coef, cost_vf_coef=self.cost_vf_coef, ent_coef=self.ent_coef, adv_affine=(1.0, 0.0),
                      cadv_affine=(0.0, 0.0), **kw)
        if self.max_grad_norm is not None:
          c.grad_clip(pi.n_params, pi._gbuf, self._word(_CLIP), self.max_grad_norm)
        self.t += 1
        c.adam(pi.n_params, pi._buf, pi._gbuf, self._m, self._v, self.step_size(self.t), beta1=b1, beta2=b2, eps=self.eps,
               clamp_first=pi.n_params - pi.nu, clamp_lo=self.std_min)
    if self.update_obs_stats and pi.normalize_observations and not pi.obs_norm_frozen:
      pi.update_obs_stats(buf)   # after the last round: collect, evaluate and every epoch of this update saw one table
    pi.refresh()   # joins the stream: the parameters and the statistics below are complete
    s = pi.grad['stats'].numpy()
    rows = s[5] if s[5] > 0 else 1.0
    stats = dict(zip(STATS, (float(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4] / rows))))
    if self._words is not None:
      w = c.dev_download(self._words, (_WORDS,), np.float32)
      if self.max_grad_norm is not None:
        stats['grad_norm'] = float(w[_CLIP])
      if self.normalize_advantage:
        stats['adv_mean'], stats['adv_std'] = float(w[_ADV_MOM + 1]), float(np.sqrt(w[_ADV_MOM + 2]))
      if self.cost_budget is not None:
        self._cost_weight = float(w[_LAG])
        stats['cost_weight'], stats['episode_cost'], stats['episodes'] = float(w[_LAG]), float(w[_LAG + 1]), int(w[_LAG + 2])
    return stats

  def close(self):
    self._own.close()
    self._m = self._v = self._words = self._mixed = self._index = self._ctx = None
