"""What the rollout buffer costs and saves: sag_gae_device alone, sag_append_rows_device under an empty mask, and a T = 16
rollout through sag.RolloutBuffer against the loop it replaces.

  python tools/rollout_buffer_time.py [out.txt] [--rounds 9] [--calls 20] [--rollouts 6] [--envs N]   (--envs: that size alone)

Point / go_to_goal at 4 194 304 and at 4096 envs; every size is a process of its own, one at a time, and all figures of a size
come from ONE context (box to box and allocation to allocation the step time moves by several per cent: only figures of the
same context are compared).
  gae     sag_gae_device, both channels, slots and final values given, 0.1 % of the step-envs truncated: 4 194 304 envs x T = 16
          and 4096 envs x T = 1000.  --calls calls enqueued back to back and one sag_wait, wall time per call, the median (and
          the minimum) over --rounds rounds after 2 of warm-up.  Bytes moved = envs * (T * (22 read + 16 written) + 8 for value
          row T of both channels) over that time.
  copy    the yardstick, same process: sag_copy_rows_device under a full mask on 240 B rows, 2 * envs * 240 bytes per call - a
          pure stream through the same memory system.  gae / copy is the ratio of the two rates.
  zeros   sag_append_rows_device and sag_copy_rows_device under an all-zero mask: the append also stores the slot plane (4 B
          per env).
  rollout the envs de-phased over time_limit = 1000 steps first (env i starts an episode at warm-up step phase[i]), then windows
          of --rollouts rollouts of 16 steps with one wait at the end, the two forms in turns, --rounds windows of each; wall
          ms per step, median, minimum and maximum per form (the spread between windows of one form is the noise floor):
            buffer    RolloutBuffer.begin(from_env=True), 16 x (actions filled on the device, buf.step(t))
            replaced  env.step(device actions, sync=False) with final_observation=True, then sag_copy_rows_device(NULL mask)
                      of the observation rows into plane t of a [16] array.  Only the observation rows (240 of the 258 bytes
                      per env and step) are copied: reward, cost, done and action rows are narrower than the 16 bytes a row of
                      that call must have, so this loop is a lower bound of what a learner runs today.
profiles/rollout_buffer_time.txt is such a table."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4194304, 4096]
GAE_T = {4194304: 16, 4096: 1000}
LIMIT, T = 1000, 16


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
  return float(np.median(ms[2:])), min(ms[2:])


def child(n, rounds, calls, rollouts):
  import numpy as np
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import _native as nat
  env = sag.make('point', 'go_to_goal', seed=12345, n_envs=n, device_buffers=True, device_reset=True, time_limit=LIMIT, auto_reset=True,
                 final_observation=True)
  env.reset()
  c = env._ctx[0]
  od, nu = env.robot.obs_dim, env.robot.nu
  row = od * 4
  out = {'row_bytes': row}
  rng, gen = np.random.RandomState(1), np.random.default_rng(1)
  normal = lambda *shape: gen.standard_normal(shape, dtype=np.float32)   # noqa: E731
  vp = nat.C.c_void_p

  # -- sag_gae_device alone ------------------------------------------------------------------------------------------
  Tg = GAE_T.get(n, T)
  P = (n + 255) // 256 * 256
  cap = max(1, n * Tg // LIMIT * 2)
  ended = np.zeros((Tg, P), np.uint8)
  ended[rng.rand(Tg, P) < 1.0 / LIMIT] = 2
  slot = np.full((Tg, P), -1, np.int32)
  k = int((ended == 2).sum())
  slot[ended == 2] = rng.permutation(max(k, 1))[:k] % cap
  host = dict(reward=normal(Tg, P, 2), cost=(rng.rand(Tg, P) < 0.1).astype(np.uint8), ended=ended,
              value=normal(Tg + 1, P), cvalue=normal(Tg + 1, P), slot=slot,
              fv=normal(cap), fcv=normal(cap))
  g = {}
  for key, a in host.items():
    g[key] = c.dev_alloc(a.nbytes)
    c.dev_upload(g[key], a)
  for key in ('adv', 'ret', 'cadv', 'cret'):
    g[key] = c.dev_alloc(Tg * P * 4)
  gae = lambda: c.gae(Tg, P, g['reward'], g['cost'], g['ended'], g['value'], g['adv'], g['ret'], 0.99, 0.95, d_cvalue=g['cvalue'],   # noqa: E731
                      d_cadv=g['cadv'], d_cret=g['cret'], d_slot=g['slot'], capacity=cap, d_final_value=g['fv'], d_final_cvalue=g['fcv'])
  out['gae'] = _timed(c, calls if Tg == 16 else max(2, calls // 4), rounds, gae)
  out['gae_T'], out['gae_bytes'] = Tg, n * (Tg * 38 + 8)
  adv = c.dev_download(g['adv'], (Tg, P), np.float32)   # (the tests compare every bit: here only that the timed calls were the kernel)
  assert np.isfinite(adv[:, :n]).all() and adv[:, :n].any()
  for p in g.values():
    c.dev_free(p)

  # -- the yardstick and the empty masks -----------------------------------------------------------------------------
  b = {key: c.dev_alloc(s) for key, s in (('a', n * row), ('b', n * row), ('mask', n), ('count', 256), ('slot', 4 * n))}
  c.dev_upload(b['a'], np.zeros((n, od), np.float32))
  c.dev_upload(b['mask'], np.ones(n, np.uint8))
  out['copy'] = _timed(c, calls, rounds, lambda: c.copy_rows(b['mask'], row, b['a'], b['b']))
  c.dev_upload(b['mask'], np.zeros(n, np.uint8))
  out['copy0'] = _timed(c, calls, rounds, lambda: c.copy_rows(b['mask'], row, b['a'], b['b']))
  out['append0'] = _timed(c, calls, rounds, lambda: c.append_rows(b['mask'], row, b['a'], b['b'], n, b['count'], 1, b['slot']))
  assert (c.dev_download(b['slot'], (min(n, 4096),), np.int32) == -1).all()
  for p in b.values():
    c.dev_free(p)

  # -- the rollout ---------------------------------------------------------------------------------------------------
  act = nat.DeviceArray(c, c.dev_alloc(n * nu * 4).value, (n, nu), np.float32)
  c.dev_fill_actions(vp(act.ptr), 0)
  phase = rng.randint(0, LIMIT, n)
  for s in range(LIMIT):   # de-phase: from here on n / LIMIT envs end per step
    env.step(act, sync=False)
    env.reset(mask=(phase == s), sync=False)
  env.wait()
  buf = sag.RolloutBuffer(env, steps=T)
  keep = c.dev_alloc(T * n * row)   # the [T] observation array of the replaced loop

  def with_buffer():
    buf.begin(from_env=True)
    for t in range(T):
      c.dev_fill_actions(buf._at('actions', t, nu * 4), t)
      buf.step(t)

  def replaced():
    for t in range(T):
      c.dev_fill_actions(vp(act.ptr), t)
      obs = env.step(act, sync=False)[0]
      c.copy_rows(None, row, vp(obs.ptr), vp(keep.value + t * n * row))

  forms = {'buffer': with_buffer, 'replaced': replaced}
  for fn in forms.values():
    fn()
  env.wait()
  r0 = env.reset_counts()[0]
  ms = {key: [] for key in forms}
  for r in range(rounds):
    for key, fn in forms.items():
      env.wait()
      t0 = time.perf_counter()
      for _ in range(rollouts):
        fn()
      env.wait()
      ms[key].append((time.perf_counter() - t0) * 1e3 / (rollouts * T))
  resets = env.reset_counts()
  for key in forms:
    out[key] = (float(np.median(ms[key])), min(ms[key]), max(ms[key]))
  out.update(resets_per_step=(resets[0] - r0) / (2 * rounds * rollouts * T), failed=resets[1], dropped=buf.final_dropped())
  print(json.dumps(out), flush=True)
  buf.close()
  c.dev_free(keep)
  c.dev_free(vp(act.ptr))
  env.close()


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  rounds, calls, rollouts, envs = int(opt('--rounds', 9)), int(opt('--calls', 20)), int(opt('--rollouts', 6)), opt('--envs', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'Point / go_to_goal, one context per size.  gae, copy, zeros: wall ms per call, calls back to back and one sag_wait, median (min) of '
           f'{rounds} rounds after 2',
           'gae: both channels, bytes = envs * (T * 38 + 8); copy: sag_copy_rows_device, full mask, 240 B rows, bytes = 2 * envs * 240; '
           'zeros: all-zero mask, sag_copy_rows_device | sag_append_rows_device (+ 4 B per env of slots)',
           f'rollout: T = {T}, time limit {LIMIT}, de-phased; wall ms per step, windows of {rollouts} rollouts in turns, median (min .. max) of '
           f'{rounds} windows per form; replaced = env.step(final_observation=True) + a copy of the observation rows (a lower bound, see the tool)',
           f'{"envs":>8} | {"gae T":>5} {"gae ms":>9} {"(min)":>9} {"TB/s":>6} | {"copy ms":>9} {"(min)":>9} {"TB/s":>6} {"gae/copy":>8} | '
           f'{"copy 0":>8} {"append 0":>8} {"+ us":>6} | {"buffer":>8} {"(min":>8} {"max)":>8} {"replaced":>8} {"(min":>8} {"max)":>8} '
           f'{"buf/repl":>8} {"resets/step":>11}']
  print('\n'.join(lines), flush=True)
  for n in ([int(envs)] if envs else SIZES):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n), str(rounds), str(calls), str(rollouts)],
                       capture_output=True, text=True, timeout=1100)
    if r.returncode != 0:
      sys.exit(f'{n} envs ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
    m = json.loads(r.stdout.strip().splitlines()[-1])
    assert m['failed'] == 0 and m['dropped'] == 0
    g_rate, c_rate = m['gae_bytes'] / (m['gae'][0] * 1e-3), 2 * n * m['row_bytes'] / (m['copy'][0] * 1e-3)
    bu, re = m['buffer'], m['replaced']
    line = (f'{n:>8} | {m["gae_T"]:>5} {m["gae"][0]:9.4f} {m["gae"][1]:9.4f} {g_rate / 1e12:6.2f} | {m["copy"][0]:9.4f} {m["copy"][1]:9.4f} '
            f'{c_rate / 1e12:6.2f} {g_rate / c_rate:8.2f} | {m["copy0"][0]:8.4f} {m["append0"][0]:8.4f} {(m["append0"][0] - m["copy0"][0]) * 1e3:6.1f} | '
            f'{bu[0]:8.4f} {bu[1]:8.4f} {bu[2]:8.4f} {re[0]:8.4f} {re[1]:8.4f} {re[2]:8.4f} {bu[0] / re[0]:8.3f} {m["resets_per_step"]:11.1f}')
    lines.append(line)
    print(line, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, ROOT)
    child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
  else:
    main()
