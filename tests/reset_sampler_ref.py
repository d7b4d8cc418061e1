"""NumPy restatement of the device reset sampler (csrc/sag_reset.hpp): the SPECIFICATION of its draws.

sample_one / try_layout of csrc/sag_sampler.cpp step for step, with the words of Philox4x32-10 under the context key on
stream 3 instead of the reference's MT19937.  Every draw is addressed by what it is for:
  candidate t of placement k in layout attempt a:  counter (env id, a << 8 | k, t, nonce << 2 | 3)
  draws after the layout:                          counter (env id, 0x80000000 | purpose, block, nonce << 2 | 3)
      purpose 0x000 robot rotation | 0x100 + item: yaw of a vase / the task object | 0x200 goal resample (block = candidate)
              0x300 button choice (masked rejection over words 0..3 of blocks 0, 1, ...)
              0x400 + actuator: Cauchy ctrl scale = x1 / x2 of a point of the unit disc (rejection over blocks)
              0x500 U(0, max_bound)
A block gives x from words 0-1 and y from words 2-3 (numpy's 53-bit random_sample).  fp64 throughout, in the host's
operation order, so records match the device bit for bit.  Vectorised over envs: each pass tests a chunk of CHUNK
consecutive candidates per env and takes the first accepted one - the same result as one candidate at a time."""
import numpy as np

MASK32 = np.uint64(0xffffffff)
REC_FLOATS, REC_INTS, MAX_NU = 184, 16, 12
(F_ROBOT, F_ROBOT0, F_GEAR, F_DAMP, F_ACTION_NOISE, F_CTRL_SCALE, F_HAZARD_SIZE, F_VASE_SIZE, F_PILLAR_SIZE, F_KEEPOUT, F_GOAL,
 F_CATCH, F_BOX, F_HAZARDS, F_PILLARS, F_BUTTONS, F_VASES, F_BOUND, F_ROBOT_EXT) = (
    0, 6, 9, 10, 11, 12, 24, 25, 26, 27, 32, 34, 41, 47, 65, 69, 81, 141, 144)
(I_TASK, I_NH, I_NV, I_NP, I_NB, I_BOX_KIND, I_GOAL_BUTTON, I_BTN_STATE, I_BTN_TIMER, I_CATCH_TIMER, I_ACTIVE_MASK, I_STEP,
 I_ENV_ID, I_FLAGS, I_EPISODE, I_AWAKE) = range(16)
ROBOTS = {'point': 0, 'car': 1, 'doggo': 2}
TASK_CATCH_GOAL = 0
STREAM = 3
POST = 0x80000000
P_ROT, P_YAW, P_GOAL, P_BUTTON, P_CTRL, P_BOUND = 0x000, 0x100, 0x200, 0x300, 0x400, 0x500
PLACE_TRIES, LAYOUT_TRIES, GOAL_TRIES, REJECT_BLOCKS = 1000, 10000, 10000, 64
CHUNK = 16
TWO_PI = 2 * 3.14159265358979323846


def philox(c0, c1, c2, c3, k0, k1):
  """Philox4x32-10 of counters (broadcast arrays of uint32 words) under the key (k0, k1) -> four uint32 arrays."""
  c0, c1, c2, c3 = (np.asarray(x, np.uint64) & MASK32 for x in np.broadcast_arrays(c0, c1, c2, c3))
  k0, k1 = np.uint64(int(k0) & 0xffffffff), np.uint64(int(k1) & 0xffffffff)
  for _ in range(10):
    p0 = np.uint64(0xD2511F53) * c0
    p1 = np.uint64(0xCD9E8D57) * c2
    c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK32
    k0 = (k0 + np.uint64(0x9E3779B9)) & MASK32
    k1 = (k1 + np.uint64(0xBB67AE85)) & MASK32
  return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def u53(a, b):
  return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0


def uniform(lo, hi, u):
  return lo + (hi - lo) * u


class Items:
  """The placements of a descriptor in the reference's dict order: robot, hazards, vases, pillars, goal, box, buttons."""

  def __init__(self, d, cfg, robot):
    nH, nV, nP, nB = d['n_hazards'], d['n_vases'], d['n_pillars'], d['n_buttons']
    k_haz = max(cfg['hazards_keepout'], cfg['hazards_size'])
    k_vase = max(cfg['vases_keepout'], cfg['vases_size'])
    k_pil = max(cfg['pillars_keepout'], cfg['pillars_size'])
    ext = list(d['extents'])
    own = lambda r: ext if all(v == 0 for v in r) else list(r)   # noqa: E731
    kinds, ko, rect = [0], [cfg['robot_keepout']], [ext]
    for kind, cnt, k in ((1, nH, k_haz), (2, nV, k_vase), (3, nP, k_pil)):
      kinds += [kind] * cnt; ko += [k] * cnt; rect += [ext] * cnt
    self.i_goal = self.i_box = -1
    if d['has_goal']:
      self.i_goal = len(kinds); kinds.append(4); ko.append(d['goal_keepout']); rect.append([-1.5, -1.5, 1.5, 1.5])
    if d['box_kind']:
      self.i_box = len(kinds); kinds.append(5); ko.append(d['box_keepout']); rect.append(own(d['box_rect']))
    for _ in range(nB):
      kinds.append(6); ko.append(d['button_keepout']); rect.append(own(d['button_rect']))
    self.kinds, self.ko, self.rect, self.n = np.array(kinds), np.array(ko, np.float64), np.array(rect, np.float64), len(kinds)
    self.k_haz, self.k_vase, self.k_pil = k_haz, k_vase, k_pil
    self.margin = cfg['placements_margin'] + (0.165 if robot == ROBOTS['doggo'] else 0.0)


def _closer(dx, dy, k):
  return np.sqrt(dx * dx + dy * dy) < k


def sample(robot, desc, cfg, gids, nonces, key, first_episode, prev=None, chunk=CHUNK):
  """Records of the envs with global ids `gids` (uint32) and episode nonces `nonces`, all of one descriptor `desc` (a
  Task.descriptor() dict); cfg: the full world config dict; key: the 64-bit context key.  prev (later episodes): dict of the
  current state's ctrl_scale [B, 12], bound, btn_state, catch_timer, catch_cur, catch_next.
  chunk: candidates tested per env and pass (any value gives the same records).
  -> rec_f [B, 184] f32, rec_i [B, 16] i32, status [B] (0, -1 layout attempts exhausted, -2 goal resample exhausted)."""
  robot = ROBOTS[robot] if isinstance(robot, str) else robot
  gids = np.asarray(gids, np.uint32)
  B = len(gids)
  nonces = np.broadcast_to(np.asarray(nonces, np.uint32), (B,))
  n4 = (nonces << np.uint32(2)) | np.uint32(STREAM)
  k0, k1 = int(key) & 0xffffffff, (int(key) >> 32) & 0xffffffff
  it = Items(desc, cfg, robot)
  n = it.n
  pos = np.zeros((B, n, 2))
  a = np.zeros(B, np.int64); k = np.zeros(B, np.int64); t = np.zeros(B, np.int64); g = np.full(B, 1.5)
  phase = np.zeros(B, np.int64)   # 0 place, 1 goal, 2 done, 3 failed
  status = np.zeros(B, np.int32)
  ar = np.arange(chunk)
  while True:
    e = np.flatnonzero(phase == 0)
    if e.size:
      kk, tt = k[e], t[e][:, None] + ar
      w1 = ((a[e] << 8) | kk).astype(np.uint32)[:, None]
      c = philox(gids[e][:, None], w1, tt.astype(np.uint32), n4[e][:, None], k0, k1)
      ko = it.ko[kk][:, None]
      r = it.rect[kk]
      lo_x, hi_x, lo_y, hi_y = r[:, 0:1] + ko, r[:, 2:3] - ko, r[:, 1:2] + ko, r[:, 3:4] - ko
      x, y = uniform(lo_x, hi_x, u53(c[0], c[1])), uniform(lo_y, hi_y, u53(c[2], c[3]))
      ok = tt < PLACE_TRIES
      for q in range(n - 1):
        thr = it.ko[q] + it.margin + ko
        hit = _closer(x - pos[e, q, 0][:, None], y - pos[e, q, 1][:, None], thr) & (q < kk)[:, None]
        ok &= ~hit
      got = ok.any(1)
      first = ok.argmax(1)
      eg = e[got]
      pos[eg, k[eg], 0] = x[got, first[got]]
      pos[eg, k[eg], 1] = y[got, first[got]]
      k[eg] += 1; t[eg] = 0
      full = eg[k[eg] == n]
      if it.i_box >= 0 and desc['box_at_robot']:
        pos[full, it.i_box, 0] = pos[full, 0, 0] + desc['box_offset']
        pos[full, it.i_box, 1] = pos[full, 0, 1]
      phase[full] = 1 if it.i_goal >= 0 else 2
      en = e[~got]
      t[en] += chunk
      over = en[t[en] >= PLACE_TRIES]
      t[over] = 0; k[over] = 0; a[over] += 1
      dead = over[a[over] >= LAYOUT_TRIES]
      phase[dead] = 3; status[dead] = -1
      continue
    e = np.flatnonzero(phase == 1)
    if not e.size:
      break
    tt = t[e][:, None] + ar
    c = philox(gids[e][:, None], np.uint32(POST | P_GOAL), tt.astype(np.uint32), n4[e][:, None], k0, k1)
    gs = np.empty((e.size, chunk))
    gs[:, 0] = g[e]
    for q in range(1, chunk):
      gs[:, q] = gs[:, q - 1] * 1.01
    gk = desc['goal_keepout']
    x, y = uniform(-gs + gk, gs - gk, u53(c[0], c[1])), uniform(-gs + gk, gs - gk, u53(c[2], c[3]))
    ok = tt < GOAL_TRIES
    for q in range(n):
      if q != it.i_goal:
        ok &= ~_closer(x - pos[e, q, 0][:, None], y - pos[e, q, 1][:, None], it.ko[q] + gk)
    got = ok.any(1)
    first = ok.argmax(1)
    eg = e[got]
    pos[eg, it.i_goal, 0] = x[got, first[got]]
    pos[eg, it.i_goal, 1] = y[got, first[got]]
    phase[eg] = 2
    en = e[~got]
    g[en] = gs[~got, -1] * 1.01
    t[en] += chunk
    dead = en[t[en] >= GOAL_TRIES]
    phase[dead] = 3; status[dead] = -2
  rf, ri = _records(robot, desc, cfg, it, gids, nonces, n4, k0, k1, pos, first_episode, prev)
  rf[status != 0] = 0
  ri[status != 0] = 0
  return rf, ri, status


def _post(gids, purpose, block, n4, k0, k1):
  return philox(gids, np.uint32(POST | purpose), np.uint32(block), n4, k0, k1)


def _records(robot, desc, cfg, it, gids, nonces, n4, k0, k1, pos, first_episode, prev):
  B = len(gids)
  rf = np.zeros((B, REC_FLOATS), np.float32)
  ri = np.zeros((B, REC_INTS), np.int32)
  c = _post(gids, P_ROT, 0, n4, k0, k1)
  robot_rot = uniform(0.0, TWO_PI, u53(c[0], c[1]))
  nu = 12 if robot == ROBOTS['doggo'] else 2
  if first_episode:
    ctrl = np.ones((B, MAX_NU))
    for q in range(nu):
      todo = np.ones(B, bool)
      for b in range(REJECT_BLOCKS):
        if not todo.any():
          break
        c = philox(gids, np.uint32(POST | P_CTRL | q), np.uint32(b), n4, k0, k1)
        x1, x2 = 2.0 * u53(c[0], c[1]) - 1.0, 2.0 * u53(c[2], c[3]) - 1.0
        r2 = x1 * x1 + x2 * x2
        acc = todo & ~((r2 >= 1.0) | (r2 == 0.0))
        with np.errstate(divide='ignore', invalid='ignore'):
          v = x1 / x2 * cfg['robot_ctrl_range_scale'] + 1.0
        ctrl[acc, q] = v[acc]
        todo &= ~acc
    rf[:, F_CTRL_SCALE:F_CTRL_SCALE + MAX_NU] = ctrl.astype(np.float32)
    bound = np.full(B, cfg['max_bound'], np.float32)
    if cfg['random_bound']:
      c = _post(gids, P_BOUND, 0, n4, k0, k1)
      bound = uniform(0.0, cfg['max_bound'], u53(c[0], c[1])).astype(np.float32)
    btn_state, catch_timer = np.ones(B, np.int32), np.zeros(B, np.int32)
    catch_cur, catch_next = np.full(B, 1.0, np.float32), np.full(B, 0.2, np.float32)
  else:
    rf[:, F_CTRL_SCALE:F_CTRL_SCALE + MAX_NU] = prev['ctrl_scale']
    bound = np.asarray(prev['bound'], np.float32)
    btn_state, catch_timer = prev['btn_state'], prev['catch_timer']
    catch_cur, catch_next = prev['catch_cur'], prev['catch_next']
  goal_button = np.zeros(B, np.int32)
  btn_timer = 0
  active = 0
  nB = desc['n_buttons']
  if desc['button_reset'] == 1:
    mx = nB - 1
    mask = mx
    for s in (1, 2, 4, 8, 16):
      mask |= mask >> s
    todo = np.full(B, mx != 0)
    for b in range(REJECT_BLOCKS):
      if not todo.any():
        break
      c = _post(gids, P_BUTTON, b, n4, k0, k1)
      for w in c:
        v = (w & np.uint32(mask)).astype(np.int64)
        acc = todo & (v <= mx)
        goal_button[acc] = v[acc]
        todo &= ~acc
    btn_timer = desc['button_timer']
  if desc['button_reset'] == 2:
    active = (1 << nB) - 1
  ri[:, I_TASK], ri[:, I_NH], ri[:, I_NV], ri[:, I_NP] = desc['task_id'], desc['n_hazards'], desc['n_vases'], desc['n_pillars']
  ri[:, I_NB], ri[:, I_BOX_KIND], ri[:, I_ENV_ID] = nB, desc['box_kind'], gids.astype(np.int32)
  ri[:, I_GOAL_BUTTON], ri[:, I_BTN_STATE], ri[:, I_BTN_TIMER] = goal_button, btn_state, btn_timer
  ri[:, I_CATCH_TIMER], ri[:, I_ACTIVE_MASK], ri[:, I_EPISODE] = catch_timer, active, nonces.astype(np.int32)
  rf[:, F_ROBOT], rf[:, F_ROBOT + 1], rf[:, F_ROBOT + 2] = pos[:, 0, 0], pos[:, 0, 1], robot_rot
  rf[:, F_ROBOT0:F_ROBOT0 + 3] = rf[:, F_ROBOT:F_ROBOT + 3]
  if robot == ROBOTS['car']:
    rf[:, F_ROBOT_EXT + 5] = 1.0
  rf[:, F_GEAR], rf[:, F_DAMP], rf[:, F_ACTION_NOISE] = desc['gear'], desc['damping'], cfg['action_noise']
  rf[:, F_HAZARD_SIZE], rf[:, F_VASE_SIZE], rf[:, F_PILLAR_SIZE] = cfg['hazards_size'], cfg['vases_size'], cfg['pillars_size']
  rf[:, F_KEEPOUT:F_KEEPOUT + 5] = np.array([cfg['robot_keepout'], it.k_haz, it.k_vase, it.k_pil, desc['box_keepout']], np.float32)
  rf[:, F_CATCH + 2], rf[:, F_CATCH + 3], rf[:, F_BOUND] = catch_cur, catch_next, bound
  h = v = p = b = 0
  for q in range(1, it.n):
    x, y = pos[:, q, 0].astype(np.float32), pos[:, q, 1].astype(np.float32)
    kind = it.kinds[q]
    if kind == 1:
      rf[:, F_HAZARDS + 2 * h], rf[:, F_HAZARDS + 2 * h + 1] = x, y; h += 1
    elif kind == 2:
      c = _post(gids, P_YAW | q, 0, n4, k0, k1)
      rf[:, F_VASES + 6 * v], rf[:, F_VASES + 6 * v + 1] = x, y
      rf[:, F_VASES + 6 * v + 2] = uniform(0.0, TWO_PI, u53(c[0], c[1])); v += 1
    elif kind == 3:
      rf[:, F_PILLARS + 2 * p], rf[:, F_PILLARS + 2 * p + 1] = x, y; p += 1
    elif kind == 4:
      rf[:, F_GOAL], rf[:, F_GOAL + 1] = x, y
      if desc['task_id'] == TASK_CATCH_GOAL:
        rf[:, F_CATCH], rf[:, F_CATCH + 1] = x, y
    elif kind == 5:
      rf[:, F_BOX], rf[:, F_BOX + 1] = x, y
      if desc['box_yaw']:
        c = _post(gids, P_YAW | q, 0, n4, k0, k1)
        rf[:, F_BOX + 2] = uniform(0.0, TWO_PI, u53(c[0], c[1]))
    else:
      rf[:, F_BUTTONS + 2 * b], rf[:, F_BUTTONS + 2 * b + 1] = x, y; b += 1
  return rf, ri



# ---------------------------------------------------------------------------------------------------------------------
# What the install of a NEW world (k_install with init_task, csrc/sag_device.hpp) derives from a sampled record
# ---------------------------------------------------------------------------------------------------------------------
F_LAST, MAX_VASES, BUTTON_R = 38, 10, np.float32(0.1)
TASK_COLLECT, TASK_PRESS_BUTTONS, TASK_PRESS_BUTTONS_SCARCE = 1, 8, 9
BOX_BOUND = {1: np.float32(0.42426406871192851), 2: np.float32(0.31048349392520047), 3: np.float32(0.14)}   # box, rod, ball


def install_last(rf, ri):
  """task.reset's `last` distances (record floats 38-40) of installed records: fp64 from the fp32 positions, stored fp32."""
  rf = np.asarray(rf, np.float32)
  d = lambda a, b: np.sqrt((rf[:, a].astype(np.float64) - rf[:, b]) ** 2 + (rf[:, a + 1].astype(np.float64) - rf[:, b + 1]) ** 2)  # noqa: E731
  out = rf[:, F_LAST:F_LAST + 3].copy()
  task = ri[:, I_TASK]
  buttons = (task == TASK_PRESS_BUTTONS) | (task == TASK_PRESS_BUTTONS_SCARCE)
  gb = F_BUTTONS + 2 * ri[:, I_GOAL_BUTTON]
  rows = np.arange(len(rf))
  to_button = np.sqrt((rf[:, F_ROBOT].astype(np.float64) - rf[rows, gb]) ** 2 + (rf[:, F_ROBOT + 1].astype(np.float64) - rf[rows, gb + 1]) ** 2)
  out[:, 0] = np.where(buttons, to_button, np.where(task != TASK_COLLECT, d(F_ROBOT, F_GOAL), out[:, 0]))
  box = ri[:, I_BOX_KIND] != 0
  out[box, 2] = d(F_GOAL, F_BOX)[box]
  out[box, 1] = d(F_ROBOT, F_BOX)[box]
  return out


def install_awake(rf, ri):
  """SAG_I_AWAKE of installed records: bit a (vases 0-9, the task object 10) is set when body a moves or its bounding circle
  overlaps another free body's, a pillar's or a button's - in the install's fp32 arithmetic."""
  rf = np.asarray(rf, np.float32)
  n = len(rf)
  vsz, psz = rf[:, F_VASE_SIZE], rf[:, F_PILLAR_SIZE]
  col = lambda a: F_VASES + 6 * a if a < MAX_VASES else F_BOX   # noqa: E731
  exists = lambda a: ri[:, I_NV] > a if a < MAX_VASES else ri[:, I_BOX_KIND] != 0   # noqa: E731

  def bound(a):
    if a < MAX_VASES:
      return vsz * np.float32(1.41421356237309504880)
    return np.select([ri[:, I_BOX_KIND] == k for k in (1, 2, 3)], [np.full(n, BOX_BOUND[k], np.float32) for k in (1, 2, 3)], np.float32(0))

  def closer(a, x, y, r):
    dx, dy, rs = x - rf[:, col(a)], y - rf[:, col(a) + 1], bound(a) + r
    return dx * dx + dy * dy < rs * rs

  awake = np.zeros(n, np.int32)
  for a in range(MAX_VASES + 1):
    over = (rf[:, col(a) + 3:col(a) + 6] != 0).any(1)
    for b in range(MAX_VASES + 1):
      if b != a:
        over |= exists(b) & closer(a, rf[:, col(b)], rf[:, col(b) + 1], bound(b))
    for q in range(2):
      over |= (ri[:, I_NP] > q) & closer(a, rf[:, F_PILLARS + 2 * q], rf[:, F_PILLARS + 2 * q + 1], psz)
    for q in range(6):
      over |= (ri[:, I_NB] > q) & closer(a, rf[:, F_BUTTONS + 2 * q], rf[:, F_BUTTONS + 2 * q + 1], BUTTON_R)
    awake |= (over & exists(a)).astype(np.int32) << a
  return awake
