"""Reset time: sag_reset_device (throughput mode's device sampler, csrc/sag_reset.hpp) against today's host path.

  python tools/reset_time.py [out.txt]

Per robot / task set and batch size: the wall time of one sag_reset_device call (first_episode 1 and 0; no status / bound
download), the sampling kernel alone (HIP events, sag_enable_timing), and the host path envs.py takes without
device_reset (sag_get_state + sag_sample_layouts on the host threads + sag_set_layout).  Prints the table and, with
out.txt, also writes it there (profiles/reset_on_device.txt is such a table)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_adaptation_gym_amd import _native as nat  # noqa: E402

CASES = [('point', 'go_to_goal', [3]), ('doggo', 'go_to_goal', [3]), ('doggo', 'multitask', list(range(14)))]
SIZES = [4096, 262144, 4194304]
REPS = 3
HOST_MAX = {'point': 4194304, 'doggo': 262144}   # host path of the largest Doggo batch: tens of seconds, not run


def one(robot, tasks, n):
  descs = [nat.task_desc_default(t) for t in tasks]
  doe = (np.arange(n) % len(tasks)).astype(np.int32)
  c = nat.Context(robot, n, seed=12345)
  c.set_tasks(descs, doe)
  c.reset_device(True, 1, want_status=False, want_bound=False)   # warm-up (first launch, allocations)
  c.enable_timing(True)
  out = {}
  for first in (1, 0):
    c.kernel_time_ms(reset=True)
    walls = []
    for _ in range(REPS):
      t0 = time.perf_counter()
      rc, _, _ = c.reset_device(first, 1, want_status=False, want_bound=False)
      walls.append((time.perf_counter() - t0) * 1e3)
      assert rc == 0, f'{rc} envs failed'
    out[first] = (min(walls), float(np.median(walls)), c.kernel_time_ms(reset=True)[0])
  host = None
  threads = min(len(os.sched_getaffinity(0)), 16)
  if n <= HOST_MAX[robot]:
    t0 = time.perf_counter()
    c.get_state()
    rf, ri, st = nat.sample_layouts(robot, np.arange(n) + 7, doe, first_episode=False, descs=descs, nthreads=threads)
    c.set_layout(rf, ri)
    host = (time.perf_counter() - t0) * 1e3
  c.close()
  return out, host, threads


def main():
  path = sys.argv[1] if len(sys.argv) > 1 else None
  hdr = (f'{"robot/task":<18} {"envs":>8} | {"device first=1 wall ms min/med":>30} {"kernel ms":>9} | '
         f'{"first=0 wall ms min/med":>24} {"kernel ms":>9} | {"host path ms (threads)":>22}')
  lines = [hdr]
  print(hdr, flush=True)
  for robot, name, tasks in CASES:
    for n in SIZES:
      out, host, threads = one(robot, tasks, n)
      h = f'{host:10.1f} ({threads})' if host is not None else 'not run'
      line = (f'{robot + "/" + name:<18} {n:>8} | {out[1][0]:14.2f} / {out[1][1]:13.2f} {out[1][2]:9.2f} | '
              f'{out[0][0]:11.2f} / {out[0][1]:10.2f} {out[0][2]:9.2f} | {h:>22}')
      lines.append(line)
      print(line, flush=True)
  if path:
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
