"""Rollout loop time: the stream-ordered loop (step -> sag_episode_track_device -> sag_reset_device_async, what
make(..., time_limit=T, auto_reset=True).step(sync=False) enqueues per context) against the plain step and against the
same loop through the synchronous calls.

  python tools/rollout_time.py [out.txt] [--steps 300] [--parent-tree DIR] [--only ROBOT] [--envs N]

Per robot / task set and batch size, wall time per step over a window of --steps steps after warm-up, with one
sag_wait at the end of the window:
  (a) sag_step_device alone
  (b) (a) + tracker + reset chain with a time limit no env reaches: the price of the tracker and of an empty chain
  (c) tracker + reset chain, time limit 100, the envs de-phased over the 100 steps before the window: 1 % end per step
  (d) the loop of (c) through the calls BatchedSafeAdaptationGym.reset(mask=..., sync=True) makes: step, wait,
      sag_reset_device of the 1 % whose turn it is (their mask is on the device already), download of the mask and of the
      whole observation buffer, sag_observe, upload.  Fewer steps at the large sizes (printed): a step takes ~1 s there.
      With --parent-tree (a checkout of another commit with its library built) it runs on that tree's package and library.
(c) and (d) alternate, twice each; the smaller figure is reported.  Every measurement is a process of its own, one at a
time; the first that fails ends the run.  profiles/rollout_loop.txt is such a table."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('point', 'go_to_goal', 4096), ('point', 'go_to_goal', 262144), ('point', 'go_to_goal', 4194304),
         ('car', 'push_box', 4096), ('doggo', 'multitask', 4096)]
TASKS = {'go_to_goal': [3], 'push_box': [10], 'multitask': list(range(14))}
LIMIT, WARM = 100, 20


def child(loop, robot, task, n, steps):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  tasks = TASKS[task]
  c = nat.Context(robot, n, seed=12345)
  c.set_tasks([nat.task_desc_default(t) for t in tasks], (np.arange(n) % len(tasks)).astype(np.int32))
  c.reset_device(True, 1, want_status=False, want_bound=False)
  nu, od = c.info['nu'], c.info['obs_dim']
  b = {k: c.dev_alloc(s) for k, s in (('act', n * nu * 4), ('obs', n * od * 4), ('rew', n * 8), ('cost', n), ('done', n), ('met', n),
                                      ('ended', n), ('episode', n * 16), ('mask', n))}
  c.dev_fill_actions(b['act'], 0)
  limit = 2**30 if loop == 'b' else LIMIT

  def step():
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
    if loop in 'bc':
      c.episode_track(b['rew'], b['cost'], b['done'], b['met'], limit, b['ended'], b['episode'])
      c.reset_device_async(b['ended'], b['obs'])

  phase = np.random.RandomState(1).randint(0, LIMIT, n)
  if loop == 'c':   # env i starts an episode at warm-up step phase[i]: from then on 1 % of the envs end per step
    for k in range(LIMIT):
      step()
      c.dev_upload(b['mask'], (phase == k).astype(np.uint8))
      c.reset_device_async(b['mask'], b['obs'])
  turns = []
  if loop == 'd':
    for k in range(LIMIT):
      turns.append(c.dev_alloc(n))
      c.dev_upload(turns[-1], (phase == k).astype(np.uint8))

  def step_d(k):
    step()
    c.wait()
    rc, _, _ = c.reset_device(False, d_mask=turns[k % LIMIT])
    assert rc == 0
    r = c.dev_download(turns[k % LIMIT], (n,), np.uint8).astype(bool)
    last = c.dev_download(b['obs'], (n, od), np.float32)
    last[r] = c.observe()[r]
    c.dev_upload(b['obs'], last)
    c.wait()

  for k in range(3 if loop == 'd' else WARM):
    step_d(k) if loop == 'd' else step()
  c.wait()
  r0 = c.reset_counts()[0] if loop in 'bc' else 0
  t0 = time.perf_counter()
  for k in range(steps):
    step_d(3 + k) if loop == 'd' else step()
  c.wait()
  ms = (time.perf_counter() - t0) * 1e3 / steps
  resets = c.reset_counts() if loop in 'bc' else (0, 0)
  print(json.dumps({'ms': ms, 'steps': steps, 'resets_per_step': (resets[0] - r0) / steps, 'failed': resets[1]}), flush=True)
  c.close()


def run(tree, loop, robot, task, n, steps):
  r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', tree, loop, robot, task, str(n), str(steps)],
                     capture_output=True, text=True, timeout=900)
  if r.returncode != 0:
    sys.exit(f'loop ({loop}) of {robot}/{task} at {n} envs ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
  return json.loads(r.stdout.strip().splitlines()[-1])


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  steps, parent, only, envs = int(opt('--steps', 300)), opt('--parent-tree', None), opt('--only', None), opt('--envs', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'wall ms per step, window of {steps} steps ((d): see its column) after warm-up, one sag_wait at the end of the window',
           f'(d) runs on {"the tree " + os.path.basename(os.path.abspath(parent)) if parent else "this tree"}',
           f'{"robot/task":<18} {"envs":>8} | {"(a) step":>9} {"(b) +track, empty chain":>24} {"(c) auto-reset 1 %":>19} {"resets/step":>11} | '
           f'{"(d) synchronous":>15} {"steps":>5} | {"(b)-(a) us":>10} {"(c)-(a) ms":>10} {"(d)/(c)":>8}']
  print('\n'.join(lines), flush=True)
  for robot, task, n in CASES:
    if (only and robot != only) or (envs and n != int(envs)):
      continue
    steps_d = steps if n <= 4096 else (30 if n <= 262144 else 5)
    ra, rb = run(ROOT, 'a', robot, task, n, steps), run(ROOT, 'b', robot, task, n, steps)
    rc, rd = [], []
    for _ in range(2):
      rc.append(run(ROOT, 'c', robot, task, n, steps))
      rd.append(run(parent or ROOT, 'd', robot, task, n, steps_d))
    c, d = min(rc, key=lambda r: r['ms']), min(rd, key=lambda r: r['ms'])
    assert rb['resets_per_step'] == 0 and c['failed'] == 0
    line = (f'{robot + "/" + task:<18} {n:>8} | {ra["ms"]:9.4f} {rb["ms"]:24.4f} {c["ms"]:19.4f} {c["resets_per_step"]:11.1f} | '
            f'{d["ms"]:15.3f} {steps_d:>5} | {(rb["ms"] - ra["ms"]) * 1e3:10.1f} {c["ms"] - ra["ms"]:10.4f} {d["ms"] / c["ms"]:8.1f}')
    lines.append(line)
    print(line, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, sys.argv[2])
    child(sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]), int(sys.argv[7]))
  else:
    main()
