"""Time of the renders of this build beside the parent's (profiles/render_aux.txt, profiles/render_unify_time.txt are such
tables).

  python tools/render_aux_time.py [out.txt] --parent-tree DIR --parent2 LIB [--rounds 5]

4096 doggo / haul_box and 4096 point / go_to_goal envs, 64 x 64, the robot's `vision` camera, no overlays.  Every measurement
is a process of its own, one at a time; the first that fails ends the run.  Wall time over a window of 20 back-to-back
launches after warm-up, one sag_wait at the end of the window.  Four figures: rgb (sag_render_rgb_device), depth and
segmentation (sag_render_aux_device), masked (sag_render_rows_device, every second byte of the mask set).  Per round and
figure, interleaved:
  parent   --parent-tree (a checkout of the parent commit with its library built; its own package loads it)
  this     this build
  parent2  --parent2 (the library of a second build of the parent, loaded by the parent's package):
           |parent2 - parent| is the spread of the measurement (A/A)
Two conditions, printed with the figures; the exit status is 1 when one does not hold:
  (1) for each figure, this build's median exceeds the parent's by no more than the largest |parent2 - parent| of the run
      (any round, any figure of the robot config);
  (2) the median of each auxiliary output does not exceed this build's RGB median."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = 20


def child(what, robot, task, n):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  from safe_adaptation_gym_amd import benchmark
  c = nat.Context(robot, n, seed=12345)
  c.set_tasks([nat.task_desc_default(benchmark.TASKS[task].TASK_ID)], np.zeros(n, np.int32))
  c.reset_device(True, 1, want_status=False, want_bound=False)
  nu, od = c.info['nu'], c.info['obs_dim']
  b = {k: c.dev_alloc(s) for k, s in (('act', n * nu * 4), ('obs', n * od * 4), ('rew', n * 8), ('cost', n), ('done', n), ('met', n),
                                      ('img', n * 64 * 64 * 8))}
  c.dev_fill_actions(b['act'], 0)
  for _ in range(10):   # (the Doggos land)
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
  if what == 'masked':
    b['mask'] = c.dev_alloc(n)
    c.dev_upload(b['mask'], (np.arange(n) % 2).astype(np.uint8))
  fn = {'rgb': lambda: c.render_rgb_device(b['img']), 'masked': lambda: c.render_rows_device(b['mask'], b['img'])}.get(
      what, lambda: c.render_aux_device(what, b['img']))
  for _ in range(3):
    fn()
  c.wait()
  t0 = time.perf_counter()
  for _ in range(REPS):
    fn()
  c.wait()
  print(json.dumps({'ms': (time.perf_counter() - t0) * 1e3 / REPS}), flush=True)
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
  return json.loads(r.stdout.strip().splitlines()[-1])['ms']


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  parent, parent2, rounds = opt('--parent-tree', None), opt('--parent2', None), int(opt('--rounds', 5))
  if not parent or not parent2 or rounds < 5:
    sys.exit(__doc__)
  path = a[0] if not a[0].startswith('--') else None
  lines = []

  def say(s):
    lines.append(s)
    print(s, flush=True)
    if path:
      os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')

  med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
  figs, builds = ['rgb', 'depth', 'segmentation', 'masked'], ['parent', 'this', 'parent2']
  ok = True
  say(f'64 x 64 vision renders, ms per launch (window of {REPS}), {rounds} interleaved rounds, a process per figure')
  for robot, task, n in (('doggo', 'haul_box', 4096), ('point', 'go_to_goal', 4096)):
    rows = {f: [] for f in figs}
    for k in range(rounds):
      for f in figs:
        r = [run(parent, None, f, robot, task, n), run(None, None, f, robot, task, n), run(parent, parent2, f, robot, task, n)]
        rows[f].append(r)
        say(f'   {robot}/{task} {n}  round {k} {f:12s}: ' + '  '.join(f'{c} {v:8.4f}' for c, v in zip(builds, r)))
    m = {f: {c: med([r[j] for r in rows[f]]) for j, c in enumerate(builds)} for f in figs}
    aa = max(abs(r[2] - r[0]) for f in figs for r in rows[f])
    for f in figs:
      say(f'   {robot}/{task} {n}  medians {f:12s}: ' + '  '.join(f'{c} {m[f][c]:.4f}' for c in builds))
    for f in figs:
      c1 = m[f]['this'] - m[f]['parent'] <= aa
      say(f'   {robot}/{task} {n}  (1) {f}: this - parent {1e3 * (m[f]["this"] - m[f]["parent"]):+.1f} us against the largest A/A difference '
          f'|parent2 - parent| {1e3 * aa:.1f} us: {"holds" if c1 else "DOES NOT HOLD"}')
      ok = ok and c1
    for f in ('depth', 'segmentation'):
      c2 = m[f]['this'] <= m['rgb']['this']
      say(f'   {robot}/{task} {n}  (2) {f} {m[f]["this"]:.4f} against RGB {m["rgb"]["this"]:.4f} ({m[f]["this"] / m["rgb"]["this"]:.2f} x): '
          f'{"holds" if c2 else "DOES NOT HOLD"}')
      ok = ok and c2
  sys.exit(0 if ok else 1)


if __name__ == '__main__':
  if len(sys.argv) > 1 and sys.argv[1] == '--child':
    sys.path.insert(0, sys.argv[2])
    child(*sys.argv[3:6], int(sys.argv[6]))
  else:
    main()
