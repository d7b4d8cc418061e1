"""What the learner's options cost: sag_moments_device, sag_advantage_mix_device, sag_lagrange_device and sag_grad_clip_device
(csrc/sag_learner.hpp) on a Point rollout of 8 planes, beside sag_copy_rows_device on the observation rows in the same process,
and PPOLearner.update() with the three switches on against all off.

  python tools/learner_time.py [out.txt] [--rounds 9] [--calls 20] [--rows N]   (--rows: that size alone)

4096 x 8 and 4 194 304 x 8 rows; every size is a process of its own, one at a time.  As tools/ppo_time.py: --calls calls enqueued
back to back and one sag_wait, wall time per call, the median (min ... max) over --rounds rounds after 2 of warm-up.
  moments    [8][N] f32 at stride 1, no mask, under the default grid cap (256 blocks) and under max_blocks = 1024; two passes
             over the array: 8 N * 4 bytes each
  episode    the cost column of the buffer's [8][N][4] episode rows under its `done` mask (stride 4): the mask is read twice,
             a 16-byte row wherever its byte is set
  mix        adv and cadv read, the mixed advantage written: 12 bytes per element
  lagrange   one thread;  clip: the n_params of hidden 64 (two launches)
  copy       the yardstick: sag_copy_rows_device on N observation rows of 240 bytes, read and written
  update     sag.PPOLearner(hidden 64, epochs 1, minibatches 8: eight rounds of one plane each) with normalize_advantage,
             max_grad_norm and cost_budget on, and with all off (the calls of the commit before: tools/ppo_time.py's backward +
             Adam on the same rows is what one of its rounds is compared with)
profiles/learner_options_time.txt is such a table.

  python tools/learner_time.py [out.txt] --shuffle [--robot point|doggo] [--envs 4096] [--steps 64] [--rounds 9] [--calls 20]

What shuffled-row minibatches cost (csrc/sag_shuffle.hpp, the ROWS instances of csrc/sag_policy_grad.hpp): one process, a
collected rollout of --steps planes of --envs rows, hidden 64, 8 minibatches.
  backward   one minibatch of steps / 8 contiguous planes: sag_policy_backward_device (the round of shuffle=False)
  sorted     the same rows through sag_policy_backward_rows_device under the list 0, 1, 2, ...: the list's own cost, no gather
  gathered   as many rows through a slice of a permutation: every row a read of 240 to 416 B at a random address
  permute    one sag_permutation_device over all steps x envs entries
  update     PPOLearner.update(), 1 epoch x 8 minibatches, shuffle=False and shuffle=True
Under SAG_LIB=<a library of the commit before> the two entry points are missing and only `backward` and the update with
shuffle=False are measured: the contiguous path of that commit.  profiles/shuffle_time.txt holds such tables."""
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
  env = sag.make('point', 'go_to_goal', seed=12345, n_envs=n, device_buffers=True, device_reset=True, time_limit=LIMIT, auto_reset=True,
                 final_observation=True)
  env.reset()
  c = env._ctx[0]
  od = env.robot.obs_dim
  pi = sag.MLPPolicy(env, hidden=HIDDEN, activation='tanh', seed=1)
  buf = sag.RolloutBuffer(env, steps=T)
  buf.collect(pi)
  pi.evaluate(buf)
  adv = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  N, P = buf.N, buf.P
  out = {'P': P, 'params': pi.n_params, 'ended': int(np.count_nonzero(buf.done.numpy()))}
  words = c.dev_alloc(32 * 4)
  c.dev_upload(words, np.zeros(32, np.float32))
  w = lambda k: words.value + 4 * k   # noqa: E731
  mixed = c.dev_alloc(T * P * 4)
  out['moments'] = _timed(c, calls, rounds, lambda: c.moments(N, T, P, adv['adv'].ptr, w(0), eps=1e-8))
  out['moments1024'] = _timed(c, calls, rounds, lambda: c.moments(N, T, P, adv['adv'].ptr, w(4), eps=1e-8, max_blocks=1024))
  c.moments(N, T, P, adv['cadv'].ptr, w(4), eps=1e-8)
  out['episode'] = _timed(c, calls, rounds, lambda: c.moments(N, T, P, buf.episode.ptr + 4, w(8), d_mask=buf.done.ptr, stride=4, eps=1e-8))
  out['lagrange'] = _timed(c, calls, rounds, lambda: c.lagrange(w(8), w(12), 0.0, 25.0))
  out['mix'] = _timed(c, calls, rounds, lambda: c.advantage_mix(N, T, P, adv['adv'].ptr, mixed, d_cadv=adv['cadv'].ptr, adv_mode=2, cadv_mode=1,
                                                                 d_adv_mom=w(0), d_cadv_mom=w(4), d_lambda=w(12)))
  g = c.dev_alloc((pi.n_params + 8) * 4)
  c.dev_upload(g, np.full(pi.n_params + 8, 0.01, np.float32))
  out['clip'] = _timed(c, calls, rounds, lambda: c.grad_clip(pi.n_params, g, w(16), 1e9))
  m = c.dev_download(words, (20,), np.float32)   # (the tests compare values: here only that the timed calls were the kernels)
  a = adv['adv'].numpy().astype(np.float64)
  assert m[0] == T * N and abs(m[1] - a.mean()) <= 1e-4 * a.std() and abs(m[2] - a.var()) <= 1e-3 * a.var(), m[:4]
  assert m[8] == out['ended'] and m[17] == 1.0 and abs(m[16] - 0.01 * np.sqrt(pi.n_params)) < 1e-5, m
  b = {k: c.dev_alloc(s) for k, s in (('a', N * od * 4), ('b', N * od * 4), ('mask', N))}
  c.dev_upload(b['a'], np.zeros((N, od), np.float32))
  c.dev_upload(b['mask'], np.ones(N, np.uint8))
  out['copy'] = _timed(c, calls, rounds, lambda: c.copy_rows(b['mask'], od * 4, b['a'], b['b']))
  for p in list(b.values()) + [g, mixed, words]:
    c.dev_free(p)
  few = calls if n <= 65536 else 2
  kw = dict(epochs=1, minibatches=T, lr=1e-5, cost_weight=0.1)
  before = pi.get_params()
  for name, opt in (('update_off', {}), ('update_on', dict(normalize_advantage=True, max_grad_norm=0.5, cost_budget=25.0))):
    pi.set_params(before)
    learner = sag.PPOLearner(pi, buf, **kw, **opt)
    out[name] = _timed(c, few, rounds, lambda: learner.update(adv))
    learner.close()
  print(json.dumps(out), flush=True)
  pi.close(); buf.close()


def shuffle_child(robot, n, steps, rounds, calls):
  import numpy as np
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import _native as nat
  from safe_adaptation_gym_amd.policy import plane_range
  env = sag.make(robot, 'go_to_goal', seed=12345, n_envs=n, device_buffers=True, device_reset=True, time_limit=LIMIT, auto_reset=True,
                 final_observation=True)
  env.reset()
  c = env._ctx[0]
  pi = sag.MLPPolicy(env, hidden=HIDDEN, activation='tanh', seed=1)
  buf = sag.RolloutBuffer(env, steps=steps)
  buf.collect(pi)
  pi.evaluate(buf)
  adv = buf.advantages(buf.value, buf.cost_value, buf.final_value, buf.final_cost_value)
  buf.wait()
  N, P, M = buf.N, buf.P, 8
  total, per = steps * N, steps // M
  have = hasattr(c.lib, 'sag_permutation_device')
  out = {'P': P, 'params': pi.n_params, 'have': have}
  kw = dict(clip=0.2, vf_coef=0.5, cost_vf_coef=0.5, ent_coef=0.0, cadv_affine=(0.1, 0.0))
  cut = lambda v, t0, t1: plane_range(v, t0, t1)   # noqa: E731
  views = lambda t0, t1: [cut(v, t0, t1) for v in (buf.obs, buf.actions, buf.logp, adv['adv'], adv['ret'], adv['cadv'], adv['cret'])]   # noqa: E731
  part, whole = views(per, 2 * per), views(0, steps)
  out['backward'] = _timed(c, calls, rounds, lambda: pi.backward(*part, scale=1.0 / (per * N), **kw))
  if have:
    index = c.dev_alloc(total * 4)
    c.dev_upload(index, np.arange(total, dtype=np.int32))
    rows = (index.value + 4 * per * N, per * N)   # the same rows as `backward`
    out['sorted'] = _timed(c, calls, rounds, lambda: pi.backward(*whole, scale=1.0 / (per * N), rows=rows, **kw))
    out['permute'] = _timed(c, calls, rounds, lambda: c.permutation(total, 7, index))
    perm = c.dev_download(index, (total,), np.int32)
    assert np.array_equal(np.sort(perm), np.arange(total))   # (the tests compare values: here only that the timed call was the kernel)
    out['gathered'] = _timed(c, calls, rounds, lambda: pi.backward(*whole, scale=1.0 / (per * N), rows=rows, **kw))
    c.dev_free(index)
  few = calls if total <= 65536 else max(4, calls // 8)
  before = pi.get_params()
  for name, opt in (('update_off', {}), ('update_shuffle', dict(shuffle=True))):
    if opt and not have:
      continue
    pi.set_params(before)
    learner = sag.PPOLearner(pi, buf, epochs=1, minibatches=M, lr=1e-5, cost_weight=0.1, **opt)
    out[name] = _timed(c, few, rounds, lambda: learner.update(adv))
    learner.close()
  print(json.dumps(out), flush=True)
  pi.close(); buf.close()


def shuffle_main(a, path):
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  robot, n, steps = opt('--robot', 'point'), int(opt('--envs', 4096)), int(opt('--steps', 64))
  rounds, calls = int(opt('--rounds', 9)), int(opt('--calls', 20))
  r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shuffle-child', robot, str(n), str(steps), str(rounds), str(calls)],
                     capture_output=True, text=True, timeout=1100)
  if r.returncode != 0:
    sys.exit(f'{robot} ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
  m = json.loads(r.stdout.strip().splitlines()[-1])
  fmt = lambda k: f'{m[k][0]:9.4f} ms ({m[k][1]:.4f} ... {m[k][2]:.4f})'   # noqa: E731
  rows = steps // 8 * n
  lines = [f'{robot}, {steps} planes of {n} rows (pitch {m["P"]}) from a collected rollout, hidden {HIDDEN} ({m["params"]} parameters), library '
           f'{os.path.basename(os.environ.get("SAG_LIB") or "libsag.so")}.  Wall ms per call, {calls} calls back to back and one sag_wait, median (min ... max) of '
           f'{rounds} rounds after 2',
           f'  backward, {steps // 8} contiguous planes = {rows} rows    {fmt("backward")}']
  if m['have']:
    lines += [f'  sorted list of the same {rows} rows          {fmt("sorted")} = {m["sorted"][0] / m["backward"][0]:.3f} x',
              f'  gathered, {rows} entries of a permutation   {fmt("gathered")} = {m["gathered"][0] / m["backward"][0]:.3f} x',
              f'  permutation of {steps * n} entries            {fmt("permute")}']
  lines += [f'  update(), shuffle=False, 8 rounds           {fmt("update_off")} = {m["update_off"][0] / 8:.4f} ms per round']
  if m['have']:
    lines += [f'  update(), shuffle=True,  8 rounds           {fmt("update_shuffle")} = {m["update_shuffle"][0] / 8:.4f} ms per round']
  print('\n'.join(lines), flush=True)
  if path:
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'a') as fh:
      fh.write('\n'.join(lines) + '\n')


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  if '--shuffle' in a:
    return shuffle_main(a, a[0] if a and not a[0].startswith('--') else None)
  rounds, calls, rows = int(opt('--rounds', 9)), int(opt('--calls', 20)), opt('--rows', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'Point (obs_dim 60), {T} planes of N rows from a collected rollout (time limit {LIMIT}), hidden {HIDDEN}; one process per size.  Wall ms per '
           f'call, calls back to back and one sag_wait, median (min ... max) of {rounds} rounds after 2',
           'TB/s: moments 2 passes x 4 B, mix 12 B per element; copy: sag_copy_rows_device on N rows of 240 B, read + written (the yardstick)']
  print('\n'.join(lines), flush=True)
  for n in ([int(rows)] if rows else SIZES):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n), str(rounds), str(calls)], capture_output=True, text=True,
                       timeout=1100)
    if r.returncode != 0:
      sys.exit(f'{n} rows ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
    m = json.loads(r.stdout.strip().splitlines()[-1])
    el = T * n
    fmt = lambda k: f'{m[k][0]:9.4f} ms ({m[k][1]:.4f} ... {m[k][2]:.4f})'   # noqa: E731
    rate = lambda k, nbytes: f'{nbytes / (m[k][0] * 1e-3) / 1e12:6.2f} TB/s'   # noqa: E731
    block = [f'{n} x {T} rows (pitch {m["P"]}, {m["ended"]} episodes ended, {m["params"]} parameters):',
             f'  moments, default 256 blocks {fmt("moments")} {rate("moments", 8 * el)}',
             f'  moments, max_blocks 1024    {fmt("moments1024")} {rate("moments1024", 8 * el)}',
             f'  episode costs (masked)      {fmt("episode")}',
             f'  mix                         {fmt("mix")} {rate("mix", 12 * el)}',
             f'  lagrange                    {fmt("lagrange")}',
             f'  clip ({m["params"]} elements)      {fmt("clip")}',
             f'  copy of {n} rows        {fmt("copy")} {rate("copy", 480 * n)}',
             f'  update(), all off, 8 rounds {fmt("update_off")} = {m["update_off"][0] / T:.4f} ms per round',
             f'  update(), all on,  8 rounds {fmt("update_on")} = {m["update_on"][0] - m["update_off"][0]:+.4f} ms']
    lines += block
    print('\n'.join(block), flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, ROOT)
    child(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
  elif len(sys.argv) > 1 and sys.argv[1] == '--shuffle-child':
    sys.path.insert(0, ROOT)
    shuffle_child(sys.argv[2], *[int(x) for x in sys.argv[3:7]])
  else:
    main()
