"""PPOLearner: the PPO-Lagrangian update of an MLPPolicy from a RolloutBuffer, on the env's context stream.

  buf.collect(pi); pi.evaluate(buf)
  out = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  stats = learner.update(out)

Every round is two enqueued calls - the gradient of one minibatch read in place from the buffer's views
(sag_policy_backward_device) and one Adam step on the policy's parameters (sag_adam_device); the update joins the stream once,
at its end.  NumPy only; no torch."""
import numpy as np

from safe_adaptation_gym_amd import _native as nat
from safe_adaptation_gym_amd.policy import plane_range

STATS = ('policy_loss', 'value_loss', 'cost_value_loss', 'approx_kl', 'clip_fraction')


class PPOLearner:
  """learner = PPOLearner(pi, buf, lr=3e-4, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0,
                          cost_weight=0.0, betas=(0.9, 0.999), eps=1e-8, std_min=1e-3)

  pi: an MLPPolicy (hidden <= 128), buf: a RolloutBuffer of the same env.  The learner owns the Adam moments and the step count.

  update(out): `out` is what buf.advantages() returned.  epochs x minibatches rounds of backward then Adam; a minibatch is a
  contiguous range of the buffer's T planes (sizes differ by at most one; ValueError if minibatches > T), the old
  log-probabilities are buf.logp, the advantage is adv - cost_weight * cadv (without a cost channel in `out`: adv), and std is
  kept at or above std_min.  Then pi.refresh() - the update's single host join - and the statistics of the last minibatch come
  back as floats: policy_loss, value_loss, cost_value_loss, approx_kl, clip_fraction.

  cost_weight is a plain attribute: the Lagrange multiplier.  Its own update is one line of the user's, from the costs of the
  episodes that ended, e.g.
    costs = [c for i in infos for c in i['episode']['cost']]       # the info dicts of the steps, or buf.episode[t][:, 1]
    learner.cost_weight = max(0.0, learner.cost_weight + 0.05 * (np.mean(costs) - cost_budget))
  Advantages are used as they are; normalising them needs their moments - pass adv_affine / cadv_affine to pi.backward yourself
  if you have them."""

  def __init__(self, pi, buf, lr=3e-4, clip=0.2, epochs=4, minibatches=4, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0,
               cost_weight=0.0, betas=(0.9, 0.999), eps=1e-8, std_min=1e-3):
    if buf.env is not pi.env:
      raise ValueError('PPOLearner: the policy and the buffer belong to different envs')
    if pi.hidden > 128:
      raise ValueError(f'PPOLearner: hidden={pi.hidden}: the backward pass supports hidden <= 128')
    epochs, minibatches = int(epochs), int(minibatches)
    if epochs < 1 or minibatches < 1:
      raise ValueError(f'PPOLearner: epochs={epochs}, minibatches={minibatches}')
    if minibatches > buf.T:
      raise ValueError(f'PPOLearner: minibatches={minibatches} of a buffer of T={buf.T} planes')
    if not (0 < clip < 1) or not lr > 0 or not eps > 0 or not std_min > 0 or not all(0 <= b < 1 for b in betas):
      raise ValueError(f'PPOLearner: lr={lr}, clip={clip}, betas={betas}, eps={eps}, std_min={std_min}')
    self.pi, self.buf = pi, buf
    self.lr, self.clip, self.epochs, self.minibatches = float(lr), float(clip), epochs, minibatches
    self.vf_coef, self.cost_vf_coef, self.ent_coef, self.cost_weight = float(vf_coef), float(cost_vf_coef), float(ent_coef), float(cost_weight)
    self.betas, self.eps, self.std_min = (float(betas[0]), float(betas[1])), float(eps), float(std_min)
    self.t = 0   # Adam steps taken
    self._ctx = c = pi._ctx
    n = pi.n_params
    self._m, self._v = c.dev_alloc(n * 4), c.dev_alloc(n * 4)
    c.dev_upload(self._m, np.zeros(n, np.float32))
    c.dev_upload(self._v, np.zeros(n, np.float32))

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
    for _ in range(self.epochs):
      for t0, t1 in self.ranges():
        cut = lambda v: plane_range(v, t0, t1)   # noqa: E731
        pi.backward(cut(buf.obs), cut(buf.actions), cut(buf.logp), cut(out['adv']), cut(out['ret']),
                    cut(out['cadv']) if cost else None, cut(out['cret']) if cost else None, clip=self.clip, vf_coef=self.vf_coef,
                    cost_vf_coef=self.cost_vf_coef, ent_coef=self.ent_coef, adv_affine=(1.0, 0.0), cadv_affine=(self.cost_weight, 0.0),
                    scale=1.0 / ((t1 - t0) * buf.N))
        self.t += 1
        c.adam(pi.n_params, pi._buf, pi._gbuf, self._m, self._v, self.step_size(self.t), beta1=b1, beta2=b2, eps=self.eps,
               clamp_first=pi.n_params - pi.nu, clamp_lo=self.std_min)
    pi.refresh()   # joins the stream: the parameters and the statistics below are complete
    s = pi.grad['stats'].numpy()
    rows = s[5] if s[5] > 0 else 1.0
    return dict(zip(STATS, (float(s[0]), float(s[1]), float(s[2]), float(s[3]), float(s[4] / rows))))

  def close(self):
    c = getattr(self, '_ctx', None)
    if c is not None and c.h:
      for p in (getattr(self, '_m', None), getattr(self, '_v', None)):
        if p is not None:
          c.dev_free(p)
    self._m = self._v = self._ctx = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass
