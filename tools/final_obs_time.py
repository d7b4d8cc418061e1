"""What final_observation=True costs: sag_copy_rows_device (k_save_rows of csrc/sag_rollout.hpp) alone under a full and under an
empty mask, and the auto_reset loop with the copy between the tracker and the reset against the same loop without it.

  python tools/final_obs_time.py [out.txt] [--rounds 9] [--calls 20] [--steps 200] [--envs N]

Point / go_to_goal (observation rows of 240 B) at 4 194 304 and at 4096 envs; every size is a process of its own, one at a
time, and the three figures of a size come from ONE context (box to box and allocation to allocation the step time moves by
several per cent: only figures of the same context are compared).
  ones    sag_copy_rows_device, all-ones mask: --calls calls enqueued back to back and one sag_wait, wall time per call, the
          median (and the minimum) over --rounds rounds after 2 of warm-up.  Bytes moved = 2 * n * row_bytes (every row read
          and written once; + n mask bytes, not counted) over that time, beside the 6.3 TB/s taken as achievable and the
          4.8 TB/s of the quiet step kernel.
  zeros   the same with an all-zero mask: n mask bytes read, nothing else.
  loop    step -> sag_episode_track_device(time limit 1000) -> [sag_copy_rows_device(ended, obs -> final)] ->
          sag_reset_device_async(ended, obs), the envs de-phased over 1000 steps before the windows (env i starts an episode at
          warm-up step phase[i]: from then on 0.1 % of the envs end per step).  Windows of --steps steps with one sag_wait at
          the end, with and without the copy in turns, --rounds of each; wall ms per step, median and minimum per form.
profiles/final_obs_time.txt is such a table."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4194304, 4096]
LIMIT = 1000
ACHIEVABLE, QUIET = 6.3e12, 4.8e12


def child(n, rounds, calls, steps):
  import numpy as np
  from safe_adaptation_gym_amd import _native as nat
  c = nat.Context('point', n, seed=12345)
  c.set_tasks([nat.task_desc_default(3)], np.zeros(n, np.int32))
  assert c.reset_device(True, 1, want_status=False, want_bound=False)[0] == 0
  nu, od = c.info['nu'], c.info['obs_dim']
  row = od * 4
  b = {k: c.dev_alloc(s) for k, s in (('act', n * nu * 4), ('obs', n * row), ('rew', n * 8), ('cost', n), ('done', n), ('met', n),
                                      ('ended', n), ('episode', n * 16), ('final', n * row), ('mask', n))}
  c.dev_fill_actions(b['act'], 0)
  c.dev_upload(b['final'], np.zeros((n, od), np.float32))

  def step(save):
    c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
    c.episode_track(b['rew'], b['cost'], b['done'], b['met'], LIMIT, b['ended'], b['episode'])
    if save:
      c.copy_rows(b['ended'], row, b['obs'], b['final'])
    c.reset_device_async(b['ended'], b['obs'])

  def copies(mask):
    c.dev_upload(b['mask'], mask)
    ms = []
    for r in range(2 + rounds):
      c.wait()
      t0 = time.perf_counter()
      for _ in range(calls):
        c.copy_rows(b['mask'], row, b['obs'], b['final'])
      c.wait()
      ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return float(np.median(ms[2:])), min(ms[2:])

  step(False)   # (observation rows to copy)
  out = {'row_bytes': row, 'ones': copies(np.ones(n, np.uint8)), 'zeros': copies(np.zeros(n, np.uint8))}
  head = (min(n, 4096), row)   # (the tests compare every byte: here only that the timed calls were the copy)
  assert (c.dev_download(b['final'], head, np.uint8) == c.dev_download(b['obs'], head, np.uint8)).all()
  phase = np.random.RandomState(1).randint(0, LIMIT, n)
  for k in range(LIMIT):   # de-phase: from here on n / LIMIT envs end per step
    step(False)
    c.dev_upload(b['mask'], (phase == k).astype(np.uint8))
    c.reset_device_async(b['mask'], b['obs'])
  for save in (True, False):
    for _ in range(20):
      step(save)
  c.wait()
  r0 = c.reset_counts()[0]
  ms = {True: [], False: []}
  for r in range(rounds):
    for save in (True, False):
      c.wait()
      t0 = time.perf_counter()
      for _ in range(steps):
        step(save)
      c.wait()
      ms[save].append((time.perf_counter() - t0) * 1e3 / steps)
  resets = c.reset_counts()
  out.update(on=(float(np.median(ms[True])), min(ms[True])), off=(float(np.median(ms[False])), min(ms[False])),
             resets_per_step=(resets[0] - r0) / (2 * rounds * steps), failed=resets[1])
  print(json.dumps(out), flush=True)
  c.close()


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  rounds, calls, steps, envs = int(opt('--rounds', 9)), int(opt('--calls', 20)), int(opt('--steps', 200)), opt('--envs', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'Point / go_to_goal.  copy: wall ms per sag_copy_rows_device call, {calls} calls back to back and one sag_wait, median (min) of '
           f'{rounds} rounds after 2; TB/s = 2 * envs * row bytes / median; {ACHIEVABLE / 1e12} TB/s taken as achievable, '
           f'{QUIET / 1e12} TB/s the quiet step kernel',
           f'loop: step + tracker (limit {LIMIT}, de-phased) [+ copy of the ended rows] + async reset, wall ms per step, windows of {steps} '
           f'steps in turns, median (min) of {rounds} windows per form, one context',
           f'{"envs":>8} {"row B":>5} | {"ones ms":>9} {"(min)":>9} {"TB/s":>6} {"of 6.3":>6} {"of 4.8":>6} | {"zeros ms":>9} {"(min)":>9} | '
           f'{"loop off":>9} {"(min)":>9} {"loop on":>9} {"(min)":>9} {"on - off us":>11} {"on / off":>8} {"resets/step":>11}']
  print('\n'.join(lines), flush=True)
  for n in SIZES:
    if envs and n != int(envs):
      continue
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(n), str(rounds), str(calls), str(steps)],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
      sys.exit(f'{n} envs ended with {r.returncode}:\n{r.stdout[-1000:]}{r.stderr[-3000:]}')
    m = json.loads(r.stdout.strip().splitlines()[-1])
    assert m['failed'] == 0
    rate = 2 * n * m['row_bytes'] / (m['ones'][0] * 1e-3)
    line = (f'{n:>8} {m["row_bytes"]:>5} | {m["ones"][0]:9.4f} {m["ones"][1]:9.4f} {rate / 1e12:6.2f} {rate / ACHIEVABLE:6.1%} {rate / QUIET:6.1%} | '
            f'{m["zeros"][0]:9.4f} {m["zeros"][1]:9.4f} | {m["off"][0]:9.4f} {m["off"][1]:9.4f} {m["on"][0]:9.4f} {m["on"][1]:9.4f} '
            f'{(m["on"][0] - m["off"][0]) * 1e3:11.1f} {m["on"][0] / m["off"][0]:8.4f} {m["resets_per_step"]:11.1f}')
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
