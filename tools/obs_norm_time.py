"""What observation normalisation costs: sag_obs_stats_device (csrc/sag_obs_norm.hpp) over a Point rollout of 8 planes, and
sag_policy_forward_norm_device / sag_policy_backward_norm_device against their plain siblings on one plane of it, beside
sag_copy_rows_device on the same rows in the same process.

  python tools/obs_norm_time.py [out.txt] [--rounds 9] [--calls 20] [--rows N]   (--rows: that size alone)
  python tools/obs_norm_time.py [out.txt] --ab LIB [--ab-runs 3] [--rows N]       the plain entry points of LIB (a library of the
                                                                                 commit before) against this tree's, alternated

4096 x 8 and 4 194 304 x 8 rows, hidden 64; every size is a process of its own, one at a time.  As tools/learner_time.py: --calls
calls enqueued back to back and one sag_wait, wall time per call, the median (min ... max) over --rounds rounds after 2 of warm-up.
  stats      sag_obs_stats_device over the 8 x N stored rows under the default cap (1024 blocks) and under max_blocks = 256;
             two passes over the rows: 2 x 8 N x 240 bytes
  forward    one plane of N rows, sampled, every output written: plain, then normalised under the policy's table (clip 10)
  backward   the same plane: plain, then normalised
  copy       the yardstick: sag_copy_rows_device on the N observation rows of 240 bytes, read and written - the least a separate
             normalising pass would cost
  --ab       the plain forward and backward on N random rows, one process per run, LIB and this tree's library in turn: the
             difference between the two must lie inside the spread of LIB's runs against each other
profiles/obs_norm_time.txt is such a table."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4096, 4194304]
T, LIMIT, HIDDEN = 8, 5, 64


def _timed(c, calls, rounds, fn):
  import numpy as np
  ms = []
  for r in range(2 + rounds):
    c.wait()
    t0 = time.perf_counter()
    for _ in range(calls):
      fn()
    c.wait()
    ms.append((time.perf_counter() - t0) * 1e3 / calls)
  return float(np.median(ms[2:])), min(ms[2:]), max(ms[2:])


def child(n, rounds, calls):
  import numpy as np
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import _native as nat
  env = sag.make('point', 'go_to_goal', seed=12345, n_envs=n, device_buffers=True, device_reset=True, time_limit=LIMIT, auto_reset=True,
                 final_observation=True)
  env.reset()
  c = env._ctx[0]
  od, nu = env.robot.obs_dim, env.robot.nu
  pi = sag.MLPPolicy(env, hidden=HIDDEN, activation='tanh', seed=1, normalize_observations=True)
  buf = sag.RolloutBuffer(env, steps=T)
  buf.collect(pi)
  pi.update_obs_stats(buf)   # the table the timed calls read is a rollout's, not the identity
  buf.collect(pi)
  pi.evaluate(buf)
  adv = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  N, P = buf.N, buf.P
  out = {'P': P, 'params': pi.n_params}
  few = calls if n <= 65536 else max(2, calls // 4)
  st, tb = c.dev_alloc((1 + 2 * od) * 8), c.dev_alloc(2 * od * 4)
  c.dev_upload(st, np.zeros(1 + 2 * od, np.float64))
  out['stats'] = _timed(c, few, rounds, lambda: c.obs_stats(st, tb, buf.obs.ptr, N, T, P))
  out['stats256'] = _timed(c, few, rounds, lambda: c.obs_stats(st, tb, buf.obs.ptr, N, T, P, max_blocks=256))
  s = c.dev_download(st, (1 + 2 * od,), np.float64)   # (the tests compare values: here only that the timed calls were the kernels)
  want = pi.get_obs_norm()
  assert s[0] > 0 and s[0] % (T * N) == 0 and np.isfinite(s).all(), s[:3]
  o = {k: c.dev_alloc(sz) for k, sz in (('act', N * nu * 4), ('logp', N * 4), ('value', N * 4), ('cvalue', N * 4), ('copy', N * od * 4), ('mask', N))}
  c.dev_upload(o['mask'], np.ones(N, np.uint8))
  draw = [0]
  fkw = dict(logp_const=pi.logp_const, d_actions=o['act'], d_logp=o['logp'], d_value=o['value'], d_cvalue=o['cvalue'], activation=nat.POLICY_TANH)

  def forward(norm):
    draw[0] += 1
    if norm:
      c.policy_forward_norm(N, HIDDEN, pi._buf, buf.obs.ptr, pi._obs_table, pi.obs_clip, draw=draw[0], **fkw)
    else:
      c.policy_forward(N, HIDDEN, pi._buf, buf.obs.ptr, draw=draw[0], **fkw)
  args = (N, 1, P, HIDDEN, pi._buf, buf.obs.ptr, buf.actions.ptr, buf.logp.ptr, adv['adv'].ptr, adv['ret'].ptr, pi._gbuf, 1.0 / N)
  bkw = dict(d_cadv=adv['cadv'].ptr, d_cret=adv['cret'].ptr, cadv_affine=(0.5, 0.0), ent_coef=0.01, activation=nat.POLICY_TANH)
  # plain and normalised in turn, twice: a drift of the machine shows as a difference between the two passes
  for rep in ('', '_2'):
    out['fwd' + rep] = _timed(c, few, rounds, lambda: forward(False))
    out['fwd_norm' + rep] = _timed(c, few, rounds, lambda: forward(True))
    out['bwd' + rep] = _timed(c, few, rounds, lambda: c.policy_backward(*args, **bkw))
    out['bwd_norm' + rep] = _timed(c, few, rounds, lambda: c.policy_backward_norm(*args, pi._obs_table, pi.obs_clip, **bkw))
  g = pi.grad['stats'].numpy()
  assert np.isfinite(g).all() and abs(g[5] - 1.0) < 1e-3 and want['count'] == T * N, (g, want['count'])
  out['copy'] = _timed(c, calls, rounds, lambda: c.copy_rows(o['mask'], od * 4, buf.obs.ptr, o['copy']))
  print(json.dumps(out), flush=True)
  for p in list(o.values()) + [st, tb]:
    c.dev_free(p)
  pi.close(); buf.close()


def child_plain(n, rounds, calls):
  """The plain forward and backward on N random rows (tools/ppo_time.py's set-up): runs under a library of the commit before."""
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  c = nat.Context('point', n, seed=12345)
  od, nu, H = c.info['obs_dim'], c.info['nu'], HIDDEN
  gen = np.random.default_rng(1)
  b = {k: c.dev_alloc(s) for k, s in (('obs', n * od * 4), ('act', n * nu * 4), ('logp', n * 4), ('value', n * 4), ('cvalue', n * 4), ('adv', n * 4),
                                      ('ret', n * 4), ('cadv', n * 4), ('cret', n * 4))}
  c.dev_upload(b['obs'], gen.uniform(-1, 1, (n, od)).astype(np.float32))
  for k in ('adv', 'ret', 'cadv', 'cret'):
    c.dev_upload(b[k], gen.standard_normal(n).astype(np.float32))
  count = od * H + H + H * H + H + H * (nu + 2) + (nu + 2) + nu
  prm = gen.uniform(-0.1, 0.1, count).astype(np.float32)
  prm[-nu:] = 0.5
  p, g = c.dev_alloc(count * 4), c.dev_alloc((count + 8) * 4)
  c.dev_upload(p, prm)
  draw = [0]
  few = calls if n <= 65536 else max(2, calls // 4)

  def forward():
    draw[0] += 1
    c.policy_forward(n, H, p, b['obs'], float(np.float32(2 * np.log(0.5) + np.log(2 * np.pi))), d_actions=b['act'], d_logp=b['logp'],
                     d_value=b['value'], d_cvalue=b['cvalue'], draw=draw[0])
  out = {'fwd': _timed(c, few, rounds, forward)}
  out['bwd'] = _timed(c, few, rounds, lambda: c.policy_backward(n, 1, n, H, p, b['obs'], b['act'], b['logp'], b['adv'], b['ret'], g, 1.0 / n,
                                                                d_cadv=b['cadv'], d_cret=b['cret'], cadv_affine=(0.5, 0.0), ent_coef=0.01))
  w = c.dev_download(g, (count + 8,), np.float32)
  assert np.isfinite(w).all() and abs(w[count + 5] - 1.0) < 1e-3, w[count:]
  out['grad_crc'] = int(np.bitwise_xor.reduce(w.view(np.uint32)))   # the two libraries compute the same bits
  print(json.dumps(out), flush=True)
  c.close()


def _run(args, env=None):
  r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True, timeout=1100,
                     env=dict(os.environ, **(env or {})))
  if r.returncode != 0:
    sys.exit(f'{args} ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
  return json.loads(r.stdout.strip().splitlines()[-1])


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  rounds, calls, rows, ab = int(opt('--rounds', 9)), int(opt('--calls', 20)), opt('--rows', None), opt('--ab', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = []

  def emit(block):
    lines.extend(block)
    print('\n'.join(block), flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'a' if ab else 'w') as fh:
        fh.write('\n'.join(block if ab else lines) + '\n')
  if ab:
    n, runs = int(rows or SIZES[-1]), int(opt('--ab-runs', 3))
    emit([f'Plain sag_policy_forward_device / sag_policy_backward_device, Point, hidden {HIDDEN}, relu, {n} random rows: {os.path.basename(ab)} '
          f'(the commit before) and this tree\'s library in turn, one process per run; wall ms per call, median (min ... max) of {rounds} rounds after 2'])
    got = {'before': [], 'this': []}
    for i in range(runs):
      for name, env in (('before', {'SAG_LIB': os.path.abspath(ab)}), ('this', {})):
        m = _run(['--child-plain', n, rounds, calls], env)
        got[name].append(m)
        emit([f'  run {i + 1} {name:6s}  forward {m["fwd"][0]:9.4f} ({m["fwd"][1]:.4f} ... {m["fwd"][2]:.4f})   backward {m["bwd"][0]:9.4f} '
              f'({m["bwd"][1]:.4f} ... {m["bwd"][2]:.4f})   gradient checksum {m["grad_crc"]:08x}'])
    for k, what in (('fwd', 'forward'), ('bwd', 'backward')):
      b, t = [m[k][0] for m in got['before']], [m[k][0] for m in got['this']]
      mb, mt = sorted(b)[len(b) // 2], sorted(t)[len(t) // 2]
      emit([f'  {what}: before {mb:.4f} ms (its runs {min(b):.4f} ... {max(b):.4f}: spread {max(b) - min(b):.4f}), this {mt:.4f} ms '
            f'({min(t):.4f} ... {max(t):.4f}); difference {mt - mb:+.4f} ms'])
    return
  emit([f'Point (obs_dim 60), {T} planes of N rows from a collected rollout (time limit {LIMIT}), hidden {HIDDEN}, tanh; one process per size.  '
        f'Wall ms per call, calls back to back and one sag_wait, median (min ... max) of {rounds} rounds after 2',
        'TB/s: stats 2 passes x 240 B per row; copy: sag_copy_rows_device on N rows of 240 B, read + written (the yardstick).  '
        'forward / backward: one plane of N rows, plain and normalised in turn, twice'])
  for n in ([int(rows)] if rows else SIZES):
    m = _run(['--child', n, rounds, calls])
    fmt = lambda k: f'{m[k][0]:9.4f} ms ({m[k][1]:.4f} ... {m[k][2]:.4f})'   # noqa: E731
    rate = lambda k, nbytes: f'{nbytes / (m[k][0] * 1e-3) / 1e12:6.2f} TB/s'   # noqa: E731
    block = [f'{n} x {T} rows (pitch {m["P"]}, {m["params"]} parameters):',
             f'  stats over {T} x {n} rows, cap 1024 {fmt("stats")} {rate("stats", 2 * T * n * 240)}',
             f'  stats, max_blocks 256          {fmt("stats256")} {rate("stats256", 2 * T * n * 240)}',
             f'  copy of {n} rows           {fmt("copy")} {rate("copy", 480 * n)}']
    for rep in ('', '_2'):
      for k, what in (('fwd', 'forward '), ('bwd', 'backward')):
        d = m[k + "_norm" + rep][0] - m[k + rep][0]
        block.append(f'  {what} plain {fmt(k + rep)}  norm {fmt(k + "_norm" + rep)}  norm - plain {d:+.4f} ms = {d / m["copy"][0]:+.2f} copies')
    emit(block)


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] in ('--child', '--child-plain'):
    sys.path.insert(0, ROOT)
    (child if sys.argv[1] == '--child' else child_plain)(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
  else:
    main()
