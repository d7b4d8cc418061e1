"""Render time of the subset forms and of the image rollout loop (profiles/rgb_rollout.txt is such a table).

  python tools/rgb_rollout_time.py [out.txt] [--parent-tree DIR --parent2 LIB] [--rounds 5] [--steps 100] [--loop-only]

Every measurement is a process of its own, one at a time; the first that fails ends the run.  Wall time over a window of
back-to-back launches after warm-up, one sag_wait at the end of the window.

 1. whole-batch render (sag_render_rgb_device, 64 x 64) of 4096 doggo / haul_box envs (BASELINE config 5) and 4096 point /
    go_to_goal envs: this build against --parent-tree (a checkout of the parent commit with its library built; its own
    package loads it) and --parent2 (the library of a second build of the parent, loaded by the parent's package), the
    three interleaved over --rounds rounds.  |parent2 - parent| per round is the spread of the measurement
    (A/A); this build's difference from the parent is read against it.
 2. sag_render_rows_device at 4096 envs with an all-zero mask, 1 % of the envs and every env, beside the whole-batch render,
    the four interleaved over --rounds rounds; the all-zero mask at 65 536 envs too.
 3. the loop at 4096 envs, 1 % of the envs ending per step (time limit 100, de-phased):
      (c) env.step(device actions, sync=False) of make(..., rgb_observation=True, device_buffers=True, device_reset=True)
          with episode_loop(time_limit=100, auto_reset=True): step, tracker, sag_reset_device_async(ended, no
          observation), whole-batch render, and the env's own host work
      (d) what a pixel learner did before: step, render, wait, mask from the host, sag_reset_device(mask) (synchronous),
          whole-batch render, wait; on --parent-tree when given.
    (c) and (d) alternate, twice each; the smaller figure is reported.  --loop-only runs part 3 alone."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 100


def _context(robot, task, n):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  from safe_adaptation_gym_amd import benchmark
  tid = benchmark.TASKS[task].TASK_ID
  c = nat.Context(robot, n, seed=12345)
  c.set_tasks([nat.task_desc_default(tid)], np.zeros(n, np.int32))
  c.reset_device(True, 1, want_status=False, want_bound=False)
  nu, od = c.info['nu'], c.info['obs_dim']
  b = {k: c.dev_alloc(s) for k, s in (('act', n * nu * 4), ('obs', n * od * 4), ('rew', n * 8), ('cost', n), ('done', n), ('met', n),
                                      ('ended', n), ('episode', n * 16), ('mask', n), ('img', n * 64 * 64 * 3))}
  c.dev_fill_actions(b['act'], 0)
  return c, b


def _window(c, fn, reps, warm=3):
  for _ in range(warm):
    fn()
  c.wait()
  t0 = time.perf_counter()
  for _ in range(reps):
    fn()
  c.wait()
  return (time.perf_counter() - t0) * 1e3 / reps


def child_render(robot, task, n, reps):
  c, b = _context(robot, task, n)
  for _ in range(10):   # (the Doggos land)
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
  print(json.dumps({'ms': _window(c, lambda: c.render_rgb_device(b['img']), reps)}), flush=True)
  c.close()


def child_subset(robot, task, n, reps, rounds):
  import numpy as np
  c, b = _context(robot, task, n)
  for _ in range(10):
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
  masks = {'zero': np.zeros(n, np.uint8), '1 %': (np.arange(n) % 100 == 7).astype(np.uint8), 'all': np.ones(n, np.uint8)}
  d = {k: c.dev_alloc(n) for k in masks}
  for k, m in masks.items():
    c.dev_upload(d[k], m)
  out = {k: [] for k in ['whole', 'zero', '1 %', 'all']}
  for _ in range(rounds):
    out['whole'].append(_window(c, lambda: c.render_rgb_device(b['img']), reps))
    for k in masks:
      out[k].append(_window(c, lambda: c.render_rows_device(d[k], b['img']), reps * (10 if k == 'zero' else 1)))
  print(json.dumps(out), flush=True)
  c.close()


def child_loop(loop, robot, task, n, steps):
  import numpy as np
  c, b = _context(robot, task, n)
  phase = np.random.RandomState(1).randint(0, LIMIT, n)

  def step_d(k):
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
    c.render_rgb_device(b['img'])
    c.wait()
    done = c.dev_download(b['done'], (n,), np.uint8)
    c.dev_upload(b['mask'], ((phase == k % LIMIT) | (done != 0)).astype(np.uint8))
    rc, _, _ = c.reset_device(False, d_mask=b['mask'])
    assert rc == 0
    c.render_rgb_device(b['img'])
    c.wait()

  if loop == 'c':   # the env itself; env i starts an episode at warm-up step phase[i]: from then on 1 % of the envs end per step
    import safe_adaptation_gym_amd as sag
    from safe_adaptation_gym_amd import _native as nat
    c.close()
    env = sag.make(robot, task, seed=12345, n_envs=n, rgb_observation=True, device_buffers=True, device_reset=True)
    env.episode_loop(time_limit=LIMIT, auto_reset=True)
    env.reset()
    c = env._ctx[0]
    nu = c.info['nu']
    d_act = c.dev_alloc(n * nu * 4)
    c.dev_fill_actions(d_act, 0)
    act = nat.DeviceArray(c, d_act.value, (n, nu), np.float32)
    for k in range(LIMIT):
      env.step(act, sync=False)
      env.reset(mask=phase == k, sync=False)
    env.wait()
    r0 = env.reset_counts()[0]
    t0 = time.perf_counter()
    for k in range(steps):
      env.step(act, sync=False)
    env.wait()
    ms, resets = (time.perf_counter() - t0) * 1e3 / steps, (env.reset_counts()[0] - r0) / steps
    print(json.dumps({'ms': ms, 'resets_per_step': resets}), flush=True)
    c.dev_free(d_act)
    env.close()
    return
  else:
    for k in range(3):
      step_d(k)
    t0 = time.perf_counter()
    for k in range(steps):
      step_d(3 + k)
    ms, resets = (time.perf_counter() - t0) * 1e3 / steps, n / LIMIT
  print(json.dumps({'ms': ms, 'resets_per_step': resets}), flush=True)
  c.close()


def run(tree, lib, *args):
  env = dict(os.environ)
  env.pop('SAG_LIB', None)
  if lib:
    env['SAG_LIB'] = os.path.abspath(lib)
  r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', os.path.abspath(tree or ROOT), *map(str, args)],
                     capture_output=True, text=True, timeout=600, env=env)
  if r.returncode != 0:
    sys.exit(f'{args} on {lib or tree or "this build"} ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
  return json.loads(r.stdout.strip().splitlines()[-1])


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  parent, parent2, rounds, steps = opt('--parent-tree', None), opt('--parent2', None), int(opt('--rounds', 5)), int(opt('--steps', 100))
  path = a[0] if a and not a[0].startswith('--') else None
  lines = []

  def say(s):
    lines.append(s)
    print(s, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')

  med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
  cases = [('doggo', 'haul_box', 4096), ('point', 'go_to_goal', 4096)]
  if parent and parent2 and '--loop-only' not in a:
    say(f'1. whole-batch render, 64 x 64, ms per launch (window of 20), {rounds} interleaved rounds: parent, this build, parent2 (second build of the parent)')
    for robot, task, n in cases:
      rows = [[run(tree, lib, 'render', robot, task, n, 20)['ms'] for tree, lib in ((parent, None), (None, None), (parent, parent2))]
              for _ in range(rounds)]
      for k, r in enumerate(rows):
        say(f'   {robot}/{task} {n}  round {k}: parent {r[0]:8.4f}  this {r[1]:8.4f}  parent2 {r[2]:8.4f}')
      aa, ab = [r[2] - r[0] for r in rows], [r[1] - r[0] for r in rows]
      say(f'   {robot}/{task} {n}  medians: parent {med([r[0] for r in rows]):.4f}  this {med([r[1] for r in rows]):.4f}  parent2 {med([r[2] for r in rows]):.4f}'
          f' | A/A parent2 - parent: median {med(aa) * 1e3:+.1f} us, largest |.| {max(map(abs, aa)) * 1e3:.1f} us'
          f' | this - parent: median {med(ab) * 1e3:+.1f} us, largest |.| {max(map(abs, ab)) * 1e3:.1f} us')
  if '--loop-only' not in a:
    part2(say, med, cases, rounds)
  part3(say, parent, steps)


def part2(say, med, cases, rounds):
  say(f'2. sag_render_rows_device, 64 x 64, ms per launch, {rounds} interleaved rounds in one process: median (min)')
  for robot, task, n in cases + [('point', 'go_to_goal', 65536)]:
    r = run(None, None, 'subset', robot, task, n, 20 if n <= 4096 else 3, rounds)
    say(f'   {robot}/{task} {n:>6}: ' + '  '.join(f'{k} {med(v):.4f} ({min(v):.4f})' for k, v in r.items()))


def part3(say, parent, steps):
  say(f'3. image rollout loop at 4096 envs, 1 % ending per step, wall ms per step over {steps} steps: (c) stream-ordered auto-reset, '
      f'(d) step, wait, host mask, synchronous masked reset, second whole-batch render{" (on the parent tree)" if parent else ""}')
  for robot, task, n in [('point', 'go_to_goal', 4096), ('doggo', 'haul_box', 4096)]:
    rc, rd = [], []
    for _ in range(2):
      rc.append(run(None, None, 'loop', 'c', robot, task, n, steps))
      rd.append(run(parent, None, 'loop', 'd', robot, task, n, steps))
    c, d = min(rc, key=lambda r: r['ms']), min(rd, key=lambda r: r['ms'])
    say(f'   {robot}/{task} {n}: (c) {c["ms"]:.4f} ({c["resets_per_step"]:.1f} resets / step)  (d) {d["ms"]:.4f} ({d["resets_per_step"]:.1f} resets / step)  (d)/(c) {d["ms"] / c["ms"]:.2f}')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, sys.argv[2])
    kind, rest = sys.argv[3], sys.argv[4:]
    if kind == 'render':
      child_render(rest[0], rest[1], int(rest[2]), int(rest[3]))
    elif kind == 'subset':
      child_subset(rest[0], rest[1], int(rest[2]), int(rest[3]), int(rest[4]))
    else:
      child_loop(rest[0], rest[1], rest[2], int(rest[3]), int(rest[4]))
  else:
    main()
