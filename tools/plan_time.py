"""Planning time: ShootingPlanner.plan() (fork, sample, score and refit on the context stream) against the same constrained
CEM planner written with the calls that existed before it - sag_fork_device, H sag_step_device calls with an observation
buffer, a download of reward / cost / done after every step, and sampling, accumulation, ranking and refit in NumPy.

  python tools/plan_time.py [out.txt] [--reps 15] [--only NAME]

Cases (I = 3 iterations, H = 12 steps, K = 64 candidates, E = 8 elites, gamma 0.99, budget 0):
  point-go_to_goal   G = 64 real envs (4096 planner envs)
  doggo-haul_box     G = 8 real envs (512 planner envs)
Both planners live in one process and take turns, call by call (device, composed, device, ...), after 2 warm-up calls each;
each call is timed on the host clock from the call to the end of a wait on the planner's stream, and the env takes the
planned action between the calls so that every call plans from a new state.  Medians over --reps calls.
profiles/plan.txt is such a table."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

CASES = {'point-go_to_goal': ('point', 'go_to_goal', 64), 'doggo-haul_box': ('doggo', 'haul_box', 8)}
K, H, I, E, GAMMA, BUDGET, SIGMA0, SIGMA_MIN = 64, 12, 3, 8, 0.99, 0.0, 0.5, 0.05


class ComposedPlanner:
  """The same planner through fork_device, step_device with an observation buffer, per-step downloads and NumPy."""

  def __init__(self, env, nat):
    self.e, G = env._ctx[0], env.n_envs
    self.G, self.n, self.nu, od = G, G * K, env.robot.nu, env.robot.obs_dim
    n, nu = self.n, self.nu
    rf, ri = env.get_state()
    rf, ri = np.repeat(rf, K, axis=0), np.repeat(ri, K, axis=0)
    ri[:, nat.I_ENV_ID] = np.arange(n)
    self.c = c = nat.Context(env.robot.name, n, device=self.e.device, seed=env._base_seed)
    c.set_layout(rf, ri)
    self.b = {k: c.dev_alloc(s) for k, s in (('src', 4 * n), ('act', 4 * n * nu), ('obs', 4 * n * od), ('rew', 8 * n), ('cost', n),
                                             ('done', n), ('met', n))}
    c.dev_upload(self.b['src'], (np.arange(n) // K).astype(np.int32))
    self.mean, self.sigma = np.zeros((H, G, nu), np.float32), np.full((H, G, nu), SIGMA0, np.float32)
    self.rng, self.planned = np.random.RandomState(1), False

  def plan(self):
    c, b, G, n, nu = self.c, self.b, self.G, self.n, self.nu
    if self.planned:
      self.mean = np.concatenate([self.mean[1:], np.zeros((1, G, nu), np.float32)])
      self.sigma[:] = SIGMA0
    for _ in range(I):
      c.fork_device(b['src'], self.e)
      z = self.rng.standard_normal((H, G, K, nu)).astype(np.float32)
      z[:, :, 0] = 0
      plans = np.clip(self.mean[:, :, None] + self.sigma[:, :, None] * z, -1, 1).reshape(H, n, nu)
      score, alive, w = np.zeros((n, 2), np.float32), np.ones(n, bool), np.float32(1)
      for t in range(H):
        c.dev_upload(b['act'], plans[t])
        c.step_device(b['act'], None, -1, b['obs'], b['rew'], b['cost'], b['done'], b['met'])
        rew = c.dev_download(b['rew'], (n, 2), np.float32)
        cost = c.dev_download(b['cost'], (n,), np.uint8)
        done = c.dev_download(b['done'], (n,), np.uint8)
        score[alive, 0] += w * rew[alive, 0]
        score[alive, 1] += w * (cost[alive] != 0)
        alive &= done == 0
        w = np.float32(w * np.float32(GAMMA))
      ret, cst = score[:, 0].reshape(G, K), score[:, 1].reshape(G, K)
      infeasible = cst > BUDGET
      for g in range(G):   # feasible by higher return, then infeasible by lower cost, then higher return, then k
        order = np.lexsort((np.arange(K), -ret[g], np.where(infeasible[g], cst[g], 0), infeasible[g]))
        x = plans[:, g * K + np.sort(order[:E]), :]
        self.mean[:, g] = x.mean(axis=1)
        self.sigma[:, g] = np.maximum(SIGMA_MIN, x.std(axis=1))
    self.planned = True
    return self.mean[0]

  def close(self):
    for p in self.b.values():
      self.c.dev_free(p)
    self.c.close()


def run(name, reps):
  import safe_adaptation_gym_amd as sag
  from safe_adaptation_gym_amd import _native as nat
  robot, task, G = CASES[name]
  envs = [sag.make(robot, task, n_envs=G, seed=11, device_buffers=True, device_reset=True) for _ in range(2)]
  for e in envs:
    e.reset()
  dev = sag.ShootingPlanner(envs[0], candidates=K, horizon=H, iterations=I, elites=E, gamma=GAMMA, cost_budget=BUDGET,
                            init_sigma=SIGMA0, min_sigma=SIGMA_MIN)
  host = ComposedPlanner(envs[1], nat)
  t_dev, t_host = [], []
  for r in range(2 + reps):
    for e in envs:
      e.wait()
    dev.wait(); host.c.wait()
    t0 = time.perf_counter()
    act = dev.plan()
    dev.wait()
    t1 = time.perf_counter()
    act_h = host.plan()
    host.c.wait()
    t2 = time.perf_counter()
    envs[0].step(act)
    envs[1].step(act_h)
    if r >= 2:
      t_dev.append((t1 - t0) * 1e3)
      t_host.append((t2 - t1) * 1e3)
  dev.close(); host.close()
  for e in envs:
    e.close()
  return G, float(np.median(t_dev)), min(t_dev), float(np.median(t_host)), min(t_host)


def main():
  a = sys.argv[1:]
  opt = lambda k, d: a[a.index(k) + 1] if k in a else d   # noqa: E731
  reps, only = int(opt('--reps', 15)), opt('--only', None)
  path = a[0] if a and not a[0].startswith('--') else None
  lines = [f'plan(): K = {K} candidates, H = {H} steps, I = {I} iterations, E = {E} elites; wall ms per call from the call to the end of a '
           f'wait on the planner\'s stream, median (min) of {reps} calls after 2, the two planners taking turns in one process',
           f'{"case":<18} {"G":>4} {"envs":>6} | {"device ms":>10} {"(min)":>9} | {"composed ms":>12} {"(min)":>9} | {"composed / device":>17} '
           f'| {"env-steps / s, device":>21}']
  print('\n'.join(lines), flush=True)
  for name in CASES:
    if only and name != only:
      continue
    G, d, dmin, h, hmin = run(name, reps)
    line = (f'{name:<18} {G:>4} {G * K:>6} | {d:10.3f} {dmin:9.3f} | {h:12.2f} {hmin:9.2f} | {h / d:17.1f} | '
            f'{G * K * H * I / (d * 1e-3):21.3e}')
    lines.append(line)
    print(line, flush=True)
    if path:
      os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
      with open(path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
