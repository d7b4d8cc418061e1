"""NumPy restatement of sag_policy_backward_device and sag_adam_device (include/sag.h), independent of the kernels:
  loss_grad64   loss, gradient and the 8 statistics of the header's function in float64; the ReLU masks may be given (the
                tests pass those of policy_ref.forward_ref32, the forward the device provably computes)
  loss_grad32   the same in plain float32 NumPy with ascending-row sums: the error of an fp32 evaluation, which is what the
                device is granted a multiple of
  adam_ref32    the header's chain, every operation rounded to float32 on its own
  logp64        the float64 log-probability of stored actions
  make_batch    a batch whose probability ratios sit well away from the clip edges, with all four branches present
  flat          gradient dict + statistics -> the device's [n_params + 8] layout
  measure       max |a - b| / max |b| per tensor
NumPy only."""
import numpy as np

import policy_ref as P

F32 = np.float32
KEYS = P.KEYS
RATIOS = (0.6, 0.7, 0.9, 1.0, 1.1, 1.4, 1.5)
COEF = dict(clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.01, adv_mul=1.0, adv_sub=0.0, cadv_mul=0.5, cadv_sub=0.0, scale=1.0)


def relu_masks(params, obs):
  """(h1 > 0, h2 > 0) of the exact fp32 chains: z > 0 <=> relu(z) > 0."""
  *_, h1, h2 = P.forward_ref32(params, obs, 'relu', hidden=True)
  return h1 > 0, h2 > 0


def _rows_outer(a, b, dt):
  """sum over rows i of outer(a[i], b[i])."""
  if dt == np.float64:
    return a.T @ b
  acc = np.zeros((a.shape[1], b.shape[1]), dt)
  for i in range(a.shape[0]):
    acc += np.outer(a[i], b[i]).astype(dt)
  return acc


def _rows_sum(a, dt):
  if dt == np.float64:
    return a.sum(0)
  acc = np.zeros(a.shape[1:], dt)
  for i in range(a.shape[0]):
    acc += a[i]
  return acc


def _loss_grad(params, batch, coef, activation, dt, masks):
  p = {k: np.asarray(params[k], dt) for k in KEYS}
  c = {k: dt(v) for k, v in coef.items()}
  x = np.asarray(batch['obs'], dt)
  a = np.asarray(batch['actions'], dt)
  n, nu = a.shape
  act = (lambda z: np.maximum(z, dt(0))) if activation == 'relu' else np.tanh
  z1 = x @ p['W1'] + p['b1']
  h1 = act(z1).astype(dt)
  z2 = h1 @ p['W2'] + p['b2']
  h2 = act(z2).astype(dt)
  o = (h2 @ p['W3'] + p['b3']).astype(dt)
  if activation == 'relu':
    d1, d2 = ((z1 > 0, z2 > 0) if masks is None else masks)
    d1, d2 = d1.astype(dt), d2.astype(dt)
  else:
    d1, d2 = dt(1) - h1 * h1, dt(1) - h2 * h2
  mean, v, cv = o[:, :nu], o[:, nu], o[:, nu + 1]
  std = p['std']
  zeta = (a - mean) / std
  slog = np.log(std).sum(dtype=dt)
  logp = dt(-0.5) * (zeta * zeta).sum(1, dtype=dt) - slog - dt(nu * 0.5 * np.log(2 * np.pi))
  lpo = np.asarray(batch['logp_old'], dt)
  rho = np.exp(logp - lpo)
  A = c['adv_mul'] * (np.asarray(batch['adv'], dt) - c['adv_sub'])
  if batch.get('cadv') is not None:
    A = A - c['cadv_mul'] * (np.asarray(batch['cadv'], dt) - c['cadv_sub'])
  lo, hi = dt(1) - c['clip'], dt(1) + c['clip']
  live = ((A >= 0) & (rho <= hi)) | ((A < 0) & (rho >= lo))
  surr = np.where(live, rho, np.clip(rho, lo, hi)) * A
  ev = v - np.asarray(batch['ret'], dt)
  L = -surr + c['vf_coef'] * dt(0.5) * ev * ev - c['ent_coef'] * slog
  dlp = np.where(live, -rho * A, dt(0)).astype(dt)
  dO = np.zeros_like(o)
  dO[:, :nu] = dlp[:, None] * zeta / std
  dO[:, nu] = c['vf_coef'] * ev
  stats = np.zeros((n, 8), dt)
  stats[:, 0] = -surr
  stats[:, 1] = dt(0.5) * ev * ev
  if batch.get('cret') is not None:
    ec = cv - np.asarray(batch['cret'], dt)
    L = L + c['cvf_coef'] * dt(0.5) * ec * ec
    dO[:, nu + 1] = c['cvf_coef'] * ec
    stats[:, 2] = dt(0.5) * ec * ec
  stats[:, 3] = lpo - logp
  stats[:, 4] = ~live
  stats[:, 5] = 1
  dstd = dlp[:, None] * (zeta * zeta - dt(1)) / std - c['ent_coef'] / std
  dz2 = ((dO @ p['W3'].T) * d2).astype(dt)
  dz1 = ((dz2 @ p['W2'].T) * d1).astype(dt)
  s = c['scale']
  grad = {'W1': s * _rows_outer(x, dz1, dt), 'b1': s * _rows_sum(dz1, dt), 'W2': s * _rows_outer(h1, dz2, dt), 'b2': s * _rows_sum(dz2, dt),
          'W3': s * _rows_outer(h2, dO, dt), 'b3': s * _rows_sum(dO, dt), 'std': s * _rows_sum(np.broadcast_to(dstd, (n, nu)), dt)}
  return s * _rows_sum(L[:, None], dt)[0], grad, s * _rows_sum(stats, dt)


def loss_grad64(params, batch, coef, masks=None, activation='relu'):
  """-> (loss, {key: gradient}, statistics [8]) in float64.  masks: (d1, d2) boolean ReLU masks, default the float64 z > 0."""
  with np.errstate(over='ignore'):
    return _loss_grad(params, batch, coef, activation, np.float64, masks)


def loss_grad32(params, batch, coef, masks=None, activation='relu'):
  with np.errstate(over='ignore'):
    return _loss_grad(params, batch, coef, activation, np.float32, masks)


def flat(grad, stats):
  return np.concatenate([np.asarray(grad[k]).reshape(-1) for k in KEYS] + [np.asarray(stats).reshape(-1)])


def split(words, shapes):
  """The device's [n_params + 8] words -> ({key: array}, statistics)."""
  out, off = {}, 0
  for k in KEYS:
    n = int(np.prod(shapes[k]))
    out[k] = words[off:off + n].reshape(shapes[k])
    off += n
  return out, words[off:off + 8]


def measure(got, ref):
  """{tensor: max |got - ref| / max |ref|} over the 7 parameter tensors and 'stats' (got, ref: (grad dict, stats)).  A tensor
  whose reference is zero throughout measures 0 if `got` is zero too and inf otherwise."""
  out = {}
  for k, g, r in [(k, got[0][k], ref[0][k]) for k in KEYS] + [('stats', got[1], ref[1])]:
    g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
    top, err = np.abs(r).max(), np.abs(g - r).max()
    out[k] = (0.0 if err == 0 else np.inf) if top == 0 else err / top
    if not np.isfinite(g).all():
      out[k] = np.inf
  return out


def adam_ref32(p, g, m, v, step, beta1=0.9, beta2=0.999, eps=1e-8, clamp_first=None, clamp_lo=0.0):
  """-> (p, m, v) after one step of the header's chain; every line below is one float32 operation per element."""
  p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
  b1, b2, eps, step, lo = F32(beta1), F32(beta2), F32(eps), F32(step), F32(clamp_lo)
  o1, o2 = F32(F32(1) - b1), F32(F32(1) - b2)
  with np.errstate(under='ignore'):
    m0 = (b1 * m).astype(F32)
    m1 = (o1 * g).astype(F32)
    m = (m0 + m1).astype(F32)
    v0 = (b2 * v).astype(F32)
    v1 = (o2 * g).astype(F32)
    v2 = (v1 * g).astype(F32)
    v = (v0 + v2).astype(F32)
    den = (np.sqrt(v).astype(F32) + eps).astype(F32)
    num = (step * m).astype(F32)
    p = (p - (num / den).astype(F32)).astype(F32)
  first = len(p) if clamp_first is None else clamp_first
  p[first:] = np.where(p[first:] > lo, p[first:], lo)
  return p, m, v


def adam_step_size(lr, t, beta1=0.9, beta2=0.999):
  """lr * sqrt(1 - beta2^t) / (1 - beta1^t), rounded once."""
  return float(F32(lr * np.sqrt(1.0 - beta2**t) / (1.0 - beta1**t)))


def logp64(params, obs, actions, activation='relu'):
  """The float64 log-probability of `actions` under the policy, per row."""
  mean, _, _ = P.forward_ref64(params, obs, activation)
  std = np.asarray(params['std'], np.float64)
  zeta = (np.asarray(actions, np.float64) - mean) / std
  return -0.5 * (zeta * zeta).sum(1) - np.log(std).sum() - len(std) * 0.5 * np.log(2 * np.pi)


def make_batch(rng, params, n, activation='relu', clip=0.2, obs_scale=1.5):
  """n rows for `params`: observations, actions sampled from the policy, advantages and returns of both channels, and
  logp_old = (the float64 logp of these actions) - log r with r drawn from RATIOS, so that rho = r up to rounding: with clip =
  0.2 every rho is at least 0.09 from a clip edge.  Asserted for every row (> 0.05); with 33 rows or more all four branches
  (live and clipped, for either sign of A under COEF's affine terms) must occur."""
  od, nu = params['W1'].shape[0], params['std'].shape[0]
  obs = rng.uniform(-obs_scale, obs_scale, (n, od)).astype(F32)
  mean, v, cv = P.forward_ref64(params, obs, activation)
  actions = (mean + np.asarray(params['std'], np.float64) * rng.standard_normal((n, nu))).astype(F32)
  logp = logp64(params, obs, actions, activation)
  r = np.asarray(RATIOS)[rng.randint(0, len(RATIOS), n)]
  batch = dict(obs=obs, actions=actions, logp_old=(logp - np.log(r)).astype(F32), adv=rng.standard_normal(n).astype(F32),
               ret=(v + rng.standard_normal(n)).astype(F32), cadv=rng.standard_normal(n).astype(F32),
               cret=(cv + rng.standard_normal(n)).astype(F32))
  rho = np.exp(logp - batch['logp_old'].astype(np.float64))
  dist = np.minimum(np.abs(rho - (1 - clip)), np.abs(rho - (1 + clip)))
  assert (dist > 0.05).all(), f'a ratio {dist.min():.4f} from a clip edge'
  if n >= 33:
    A = COEF['adv_mul'] * (batch['adv'] - COEF['adv_sub']) - COEF['cadv_mul'] * (batch['cadv'] - COEF['cadv_sub'])
    live = ((A >= 0) & (rho <= 1 + clip)) | ((A < 0) & (rho >= 1 - clip))
    for sign in (A >= 0, A < 0):
      assert (live & sign).any() and (~live & sign).any(), 'a branch of the surrogate is missing from the batch'
  return batch
