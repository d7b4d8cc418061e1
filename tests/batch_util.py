"""Builds batches of layouts with the package's host sampler (reference semantics,
seed base 666) for the parity tests and the bench."""
import numpy as np

from safe_adaptation_gym_amd import _native as nat
from safe_adaptation_gym_amd import benchmark
from safe_adaptation_gym_amd.robot import Robot
from world import World


def sample_records_native(robot_name, task_names, n, seed=666, config=None):
  """Same through the native sampler; task_names may be one name or a per-env list."""
  if isinstance(task_names, str):
    tids = benchmark.TASKS[task_names].TASK_ID
  else:
    tids = np.array([benchmark.TASKS[t].TASK_ID for t in task_names], np.int32)
  rf, ri, st = nat.sample_layouts(robot_name, seed + np.arange(n), tids, config=config)
  assert not st.any()
  return rf, ri


def sample_records(robot_name, task_name, n, seed=666, config=None):
  """n records: env i sampled with RandomState(seed + i) exactly as make() would."""
  robot = Robot(f'xmls/{robot_name}.xml')
  rf = np.zeros((n, nat.REC_FLOATS), np.float32)
  ri = np.zeros((n, nat.REC_INTS), np.int32)
  for i in range(n):
    rs = np.random.RandomState(seed + i)
    task = benchmark.TASKS[task_name]() if isinstance(task_name, str) else benchmark.TASKS[task_name[i]]()
    w = World(rs, task, robot, config)
    w.sample_layout()
    w.reset()
    rf[i], ri[i] = w.record(env_id=i)
  return rf, ri


def pursuit_actions(rf, ri, rng, p_random=0.2, robot='point'):
  """A policy that drives Point robots towards their current target with noise, so
  goals are met and obstacles are hit: u0 = forward, u1 = turn rate command."""
  n = len(rf)
  x, y, yaw = rf[:, nat.F_ROBOT], rf[:, nat.F_ROBOT + 1], rf[:, nat.F_ROBOT + 2]
  tx, ty = rf[:, nat.F_GOAL].copy(), rf[:, nat.F_GOAL + 1].copy()
  nb = ri[:, nat.I_NB]
  for i in np.flatnonzero(nb > 0):
    task = ri[i, nat.I_TASK]
    if task == 1:  # collect: lowest active button
      m = int(ri[i, nat.I_ACTIVE_MASK])
      b = (m & -m).bit_length() - 1 if m else 0
    else:
      b = ri[i, nat.I_GOAL_BUTTON]
    tx[i], ty[i] = rf[i, nat.F_BUTTONS + 2 * b], rf[i, nat.F_BUTTONS + 2 * b + 1]
  # box tasks: drive at the box (tests place the goal just beyond it, see goal_beyond_box)
  for i in np.flatnonzero(ri[:, nat.I_BOX_KIND] > 0):
    tx[i], ty[i] = rf[i, nat.F_BOX], rf[i, nat.F_BOX + 1]
    if ri[i, nat.I_TASK] == 7:  # haul_box: the box follows on its tether; head for the goal
      tx[i], ty[i] = rf[i, nat.F_GOAL], rf[i, nat.F_GOAL + 1]
  heading = yaw if robot == 'point' else yaw - np.pi / 2   # the car drives along its -y axis
  ang = np.arctan2(ty - y, tx - x) - heading
  ang = (ang + np.pi) % (2 * np.pi) - np.pi
  if robot == 'point':
    a = np.stack([np.where(np.abs(ang) < 1.0, 1.0, 0.2), np.clip(2.0 * ang, -1, 1)], -1)
  else:
    # wheel torques saturate at |u| = .02 (car.xml:7): steer by easing one wheel; left faster = CCW
    turn = np.clip(1.5 * ang, -1, 1)
    a = 0.02 * np.stack([1 + 2 * np.minimum(turn, 0), 1 - 2 * np.maximum(turn, 0)], -1)
  rnd = rng.uniform(-1, 1, (n, 2))
  pick = rng.uniform(size=n) < p_random
  a[pick] = rnd[pick]
  return a.astype(np.float32)


STATE_TOL = 1e-4     # one-step qpos/qvel: HIP fp32 vs oracle fp64 from the same fp32 state
STATE_TOL32 = 2e-5   # ... vs the fp32 build of the oracle
MIXED = 'multitask'


def lockstep_state_tol(robot, task, ncol):
  """The lockstep's per-column state tolerances (abs; the same value again relative) against the fp64 and the fp32
  build of the oracle, for the Point and the Car."""
  tol64 = np.full(ncol, STATE_TOL)
  tol32 = np.full(ncol, STATE_TOL32)
  # rest capture (REST_W = 1e-4 rad/s) and contacts at zero depth between resting bodies are
  # decided at float rounding: free-body spin rates may differ by that scale
  for wf in [46] + [81 + 6 * k + 5 for k in range(10)]:
    tol32[wf] = 2e-4
    tol64[wf] = 2e-4
  if robot == 'car':
    # the rear ball (2.6 g, I = 2.6e-6 kg m^2, joint damping 1e-3: time constant I / d = 2.6 ms < h) and the wheels
    # are stiff spinning parts: the fp32 oracle (world-frame friction, divisions) and the device (body-frame
    # constants, reciprocals) round differently by an ulp per operation, amplified here ~100x; values are O(10) rad/s
    for wf in range(144, 149):
      tol32[wf] = 2e-4
  if task in ('dribble_ball', MIXED):
    # the ball's spin (unobservable; I = 4.5e-8 kg m^2) is set by friction torques of a stiff,
    # underdamped contact (solref .018 .2): fp32 rounding is amplified ~1000x there
    tol64[46] = tol32[46] = 5e-3
  return tol64, tol32


def doggo_state_tol(ncol):
  """The Doggo lockstep's per-column state tolerance (abs; the same value again relative) after one step from identical
  fp32 state: robot qpos within 2e-5, qvel within 2e-3, free bodies within the planar STATE_TOL (spin 2e-4; the task
  object's 5e-3)."""
  E = 144
  pos_f = [0, 1, 2, E] + list(range(E + 1, E + 5)) + list(range(E + 9, E + 22))
  tol = np.full(ncol, 2e-3)
  tol[pos_f] = 2e-5
  for k in range(10):
    tol[81 + 6 * k:81 + 6 * k + 6] = STATE_TOL
    tol[81 + 6 * k + 5] = 2e-4
  tol[41:47] = STATE_TOL; tol[46] = 5e-3
  return tol


def rows_outside(d_rf, o_rf, tol):
  """Rows of d_rf with a column outside tol (abs + rel) of o_rf."""
  return (np.abs(d_rf - o_rf) > tol + tol * np.abs(o_rf)).any(1)


def goal_beyond_box(rf, ri, dist=0.55):
  """Test set-up for the PushBox family: move every goal to `dist` beyond the box on the
  robot -> box line, so a straight push meets it (and the on-goal resample, RNG draws and
  PushBox.reset run many times in a short rollout)."""
  rf = rf.copy()
  for i in np.flatnonzero(ri[:, nat.I_BOX_KIND] > 0):
    r = rf[i, nat.F_ROBOT:nat.F_ROBOT + 2]
    b = rf[i, nat.F_BOX:nat.F_BOX + 2]
    d = (b - r) / (np.linalg.norm(b - r) + 1e-9)
    rf[i, nat.F_GOAL:nat.F_GOAL + 2] = b + dist * d
  return rf
