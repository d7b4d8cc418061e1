"""ctypes binding of libsag.so (include/sag.h).  NumPy only - no torch on the path.

There is no CPU fallback: if the HIP library is missing or no MI355X is visible,
every entry point raises."""
import collections
import ctypes as C
import functools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAG_LIB overrides the library file (A/B builds of the same ABI during kernel tuning)
LIB_PATH = os.environ.get('SAG_LIB') or os.path.join(_HERE, 'libsag.so')

ABI_VERSION = 5
MAX_HAZARDS, MAX_VASES, MAX_PILLARS, MAX_BUTTONS, MAX_NU = 9, 10, 2, 6, 12
REC_FLOATS, REC_INTS = 184, 16

# record field offsets (enum sag_rec_float / sag_rec_int)
F_ROBOT, F_ROBOT0, F_GEAR, F_DAMP, F_ACTION_NOISE, F_CTRL_SCALE = 0, 6, 9, 10, 11, 12
F_HAZARD_SIZE, F_VASE_SIZE, F_PILLAR_SIZE, F_KEEPOUT = 24, 25, 26, 27
F_GOAL, F_CATCH, F_LAST, F_BOX = 32, 34, 38, 41
F_HAZARDS, F_PILLARS, F_BUTTONS, F_VASES = 47, 65, 69, 81
F_ROBOT_EXT = 144
F_BOUND = 141
(I_TASK, I_NH, I_NV, I_NP, I_NB, I_BOX_KIND, I_GOAL_BUTTON, I_BTN_STATE, I_BTN_TIMER,
 I_CATCH_TIMER, I_ACTIVE_MASK, I_STEP, I_ENV_ID, I_FLAGS, I_EPISODE, I_AWAKE) = range(16)

ROBOT_IDS = {'point': 0, 'car': 1, 'doggo': 2}
FORK_SAME_STREAM = 1   # enum sag_fork_flags

class SagError(RuntimeError):
  pass


class _Config(C.Structure):
  _fields_ = [('abi_version', C.c_int32), ('robot', C.c_int32), ('n_envs', C.c_int32),
              ('device', C.c_int32), ('max_hazards', C.c_int32), ('max_vases', C.c_int32),
              ('max_pillars', C.c_int32), ('max_buttons', C.c_int32), ('has_box', C.c_int32),
              ('reserved0', C.c_int32), ('seed', C.c_uint64)]


class WorldConfig(C.Structure):
  _fields_ = [(k, C.c_double) for k in ('placements_margin', 'robot_keepout', 'hazards_size',
                                         'vases_size', 'pillars_size', 'hazards_keepout',
                                         'vases_keepout', 'pillars_keepout',
                                         'robot_ctrl_range_scale', 'action_noise', 'max_bound')] + [
                                             ('random_bound', C.c_int32), ('reserved', C.c_int32)]


class GaeDesc(C.Structure):
  """sag_gae_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('T', 'pitch', 'capacity', 'reserved')] + [
      (k, C.c_float) for k in ('gamma', 'lam', 'cost_gamma', 'cost_lam')] + [
          (k, C.c_void_p) for k in ('d_reward', 'd_cost', 'd_ended', 'd_value', 'd_cvalue', 'd_slot', 'd_final_value',
                                    'd_final_cvalue', 'd_adv', 'd_ret', 'd_cadv', 'd_cret')]


class PolicyDesc(C.Structure):
  """sag_policy_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('n_rows', 'hidden', 'activation', 'flags', 'obs_pitch', 'reserved')] + [
      ('draw', C.c_uint32), ('row0', C.c_uint32), ('logp_const', C.c_float)] + [
          (k, C.c_void_p) for k in ('d_params', 'd_obs', 'd_actions', 'd_logp', 'd_value', 'd_cvalue')]


class PolicyGradDesc(C.Structure):
  """sag_policy_grad_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('n_rows', 'n_planes', 'pitch', 'obs_pitch', 'hidden', 'activation', 'flags', 'max_blocks')] + [
      (k, C.c_float) for k in ('clip', 'vf_coef', 'cvf_coef', 'ent_coef', 'adv_mul', 'adv_sub', 'cadv_mul', 'cadv_sub', 'scale', 'reserved')] + [
          (k, C.c_void_p) for k in ('d_params', 'd_obs', 'd_actions', 'd_logp_old', 'd_adv', 'd_ret', 'd_cadv', 'd_cret', 'd_grad')]


class AdamDesc(C.Structure):
  """sag_adam_desc (include/sag.h)."""
  _fields_ = [('n', C.c_int32), ('clamp_first', C.c_int32)] + [
      (k, C.c_float) for k in ('beta1', 'beta2', 'eps', 'step', 'clamp_lo', 'reserved')] + [
          (k, C.c_void_p) for k in ('d_param', 'd_grad', 'd_m', 'd_v')]


class MomentsDesc(C.Structure):
  """sag_moments_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('n_rows', 'n_planes', 'pitch', 'stride', 'max_blocks', 'reserved')] + [
      ('eps', C.c_float), ('reserved_f', C.c_float)] + [(k, C.c_void_p) for k in ('d_x', 'd_mask', 'd_out')]


class AdvantageMixDesc(C.Structure):
  """sag_advantage_mix_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('n_rows', 'n_planes', 'pitch', 'reserved', 'adv_mode', 'cadv_mode')] + [
      ('cost_weight', C.c_float), ('reserved_f', C.c_float)] + [
          (k, C.c_void_p) for k in ('d_adv', 'd_cadv', 'd_adv_mom', 'd_cadv_mom', 'd_lambda', 'd_out')]


class LagrangeDesc(C.Structure):
  """sag_lagrange_desc (include/sag.h)."""
  _fields_ = [(k, C.c_float) for k in ('lr', 'budget', 'lambda_max', 'reserved')] + [(k, C.c_void_p) for k in ('d_mom', 'd_state')]


class GradClipDesc(C.Structure):
  """sag_grad_clip_desc (include/sag.h)."""
  _fields_ = [('n', C.c_int32), ('max_blocks', C.c_int32), ('max_norm', C.c_float), ('reserved', C.c_float)] + [
      (k, C.c_void_p) for k in ('d_grad', 'd_out')]


class ObsStatsDesc(C.Structure):
  """sag_obs_stats_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('n_rows', 'n_planes', 'pitch', 'obs_pitch', 'max_blocks', 'flags')] + [
      ('eps', C.c_float), ('reserved', C.c_float)] + [(k, C.c_void_p) for k in ('d_obs', 'd_state', 'd_table')]


OBS_STATS_TABLE_ONLY = 1          # enum sag_obs_stats_flags
POLICY_RELU, POLICY_TANH = 0, 1   # enum sag_policy_activation
ADV_RAW, ADV_CENTER, ADV_STANDARDIZE = 0, 1, 2   # enum sag_advantage_mode
POLICY_MEAN = 1                   # enum sag_policy_flags
POLICY_GRAD_ACCUMULATE = 1        # enum sag_policy_grad_flags
POLICY_GRAD_STATS = 8             # words behind the gradient


class TaskDesc(C.Structure):
  """sag_task_desc (include/sag.h)."""
  _fields_ = [(k, C.c_int32) for k in ('task_id', 'n_hazards', 'n_vases', 'n_pillars', 'has_goal', 'box_kind', 'box_yaw',
                                        'box_at_robot', 'n_buttons', 'button_reset', 'button_timer', 'reserved')] + [
      ('extents', C.c_double * 4), ('goal_keepout', C.c_double), ('box_keepout', C.c_double), ('button_keepout', C.c_double),
      ('box_offset', C.c_double), ('box_rect', C.c_double * 4), ('button_rect', C.c_double * 4), ('gear', C.c_double),
      ('damping', C.c_double)]

  @classmethod
  def from_dict(cls, d):
    t = cls()
    for k, v in d.items():
      if isinstance(v, (list, tuple)):
        setattr(t, k, (C.c_double * 4)(*v))
      else:
        setattr(t, k, v)
    return t

  def to_dict(self):
    return {k: (list(getattr(self, k)) if k in ('extents', 'box_rect', 'button_rect') else getattr(self, k))
            for k, _ in self._fields_ if k != 'reserved'}


def _signatures():
  """Every function include/sag.h declares -> (argtypes, restype): the one table load() applies and EXPORTS lists."""
  i32, u32, u64, f32, vp = C.c_int32, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p
  fp, ip, up, bp, dp, u64p = (C.POINTER(t) for t in (C.c_float, C.c_int32, C.c_uint32, C.c_uint8, C.c_double, C.c_uint64))
  cfg, task = C.POINTER(WorldConfig), C.POINTER(TaskDesc)
  sample_tail = [cfg, i32, i32, fp, ip, up, ip, ip, dp, ip, i32]
  sigs = {
      'sag_last_error': ([vp], C.c_char_p),
      'sag_robot_info': [i32, ip, dp],
      'sag_create': [C.POINTER(_Config), C.POINTER(vp)],
      'sag_destroy': [vp],
      'sag_set_layout': [vp, ip, i32, fp, ip],
      'sag_set_state': [vp, ip, i32, fp, ip],
      'sag_get_state': [vp, ip, i32, fp, ip],
      'sag_reset': [vp, ip, i32],
      'sag_step': [vp, fp, fp, up, i32, i32, fp, fp, bp, bp, bp, ip],
      'sag_step_device': [vp, vp, vp, i32, vp, vp, vp, vp, vp],
      'sag_wait': [vp],
      'sag_observe': [vp, fp],
      'sag_set_ext_contacts': [vp, ip, up],
      'sag_lidar_cost': [vp, i32, i32, fp, fp, bp, f32, fp, ip, bp],
      'sag_lidar_cost_device': [vp, i32, i32, vp, vp, vp, f32, vp, vp, vp],
      'sag_set_seed': [vp, u64],
      'sag_dev_alloc': [vp, u64, C.POINTER(vp)],
      'sag_dev_free': [vp, vp],
      'sag_dev_upload': [vp, vp, vp, u64],
      'sag_dev_download': [vp, vp, vp, u64],
      'sag_dev_fill_actions': [vp, vp, u32],
      'sag_kernel_time_ms': [vp, i32, dp, C.POINTER(C.c_int64)],
      'sag_enable_timing': [vp, i32],
      'sag_busy_count': [vp, ip],
      'sag_debug_cycles': [vp, i32, u64p, i32],
      'sag_debug_doggo_coop': [vp, dp],
      'sag_render_rgb': [vp, bp],
      'sag_render_rgb_device': [vp, vp],
      'sag_render': [vp, i32, i32, i32, i32, bp],
      'sag_render_device': [vp, i32, i32, i32, i32, vp, vp, vp],
      'sag_render_rows_device': [vp, i32, i32, i32, i32, vp, vp, vp, vp],
      'sag_render_envs': [vp, i32, i32, i32, i32, ip, i32, bp],
      'sag_render_aux': [vp, i32, i32, i32, i32, i32, ip, i32, vp],
      'sag_render_aux_device': [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp],
      'sag_device_count': [],
      'sag_world_config_default': ([cfg], None),
      'sag_task_desc_default': [i32, task],
      'sag_task_desc_check': ([task], C.c_char_p),
      'sag_sample_layouts': [i32, i32, up, ip] + sample_tail,
      'sag_sample_layouts_desc': [i32, i32, up, task, i32, ip] + sample_tail,
      'sag_set_tasks': [vp, vp, i32, ip, cfg, i32],
      'sag_reset_device': [vp, i32, i32, vp, ip, fp],
      'sag_reset_device_async': [vp, vp, vp],
      'sag_reset_device_counts': [vp, i32, u64p, u64p],
      'sag_episode_track_device': [vp, vp, vp, vp, vp, i32, vp, vp],
      'sag_episode_clear': [vp, vp],
      'sag_copy_rows_device': [vp, vp, i32, vp, vp],
      'sag_append_rows_device': [vp, vp, i32, vp, vp, i32, vp, i32, vp],
      'sag_fork_device': [vp, vp, vp, i32],
      'sag_fork_counts': [vp, i32, u64p, u64p],
      'sag_wait_for': [vp, vp],
      'sag_plan_sample_device': [vp, i32, i32, vp, vp, u32, vp],
      'sag_plan_score_device': [vp, vp, i32, f32, vp],
      'sag_plan_refit_device': [vp, i32, i32, i32, vp, vp, vp, f32, vp, vp, vp, vp],
      'sag_plan_shift_device': [vp, i32, i32, vp, vp, f32],
      'sag_plan_clear_device': [vp, i32, i32, vp, vp, vp, f32],
      'sag_gae_device': [vp, C.POINTER(GaeDesc)],
      'sag_policy_forward_device': [vp, C.POINTER(PolicyDesc)],
      'sag_policy_backward_device': [vp, C.POINTER(PolicyGradDesc)],
      'sag_adam_device': [vp, C.POINTER(AdamDesc)],
      'sag_moments_device': [vp, C.POINTER(MomentsDesc)],
      'sag_advantage_mix_device': [vp, C.POINTER(AdvantageMixDesc)],
      'sag_lagrange_device': [vp, C.POINTER(LagrangeDesc)],
      'sag_grad_clip_device': [vp, C.POINTER(GradClipDesc)],
      'sag_obs_stats_device': [vp, C.POINTER(ObsStatsDesc)],
      'sag_policy_forward_norm_device': [vp, C.POINTER(PolicyDesc), vp, f32],
      'sag_policy_backward_norm_device': [vp, C.POINTER(PolicyGradDesc), vp, f32],
      'sag_permutation_device': [vp, i32, u32, vp],
      'sag_policy_backward_rows_device': [vp, C.POINTER(PolicyGradDesc), vp, i32, vp, f32],
  }
  return {k: v if isinstance(v, tuple) else (v, C.c_int) for k, v in sigs.items()}   # (a bare list returns the status int)


SIGNATURES = _signatures()
EXPORTS = list(SIGNATURES)
_lib = None


def load():
  """Load libsag.so; raises SagError (never falls back) if it is not there."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise SagError(
        f'{LIB_PATH} not found: build it with `python -m safe_adaptation_gym_amd.build` '
        '(hipcc, --offload-arch=gfx950). There is no CPU fallback.')
  lib = C.CDLL(LIB_PATH)
  # (a SAG_LIB library of an earlier commit lacks some symbols: it still loads for an A/B run of the paths it has, and a call of
  # a missing one raises AttributeError)
  for name, (argtypes, restype) in SIGNATURES.items():
    if hasattr(lib, name):
      fn = getattr(lib, name)
      fn.argtypes, fn.restype = argtypes, restype
  _lib = lib
  return lib


def robot_info(robot):
  lib = load()
  out = (C.c_int32 * 5)()
  dt = C.c_double()
  rc = lib.sag_robot_info(ROBOT_IDS[robot] if isinstance(robot, str) else robot, out, C.byref(dt))
  if rc:
    raise SagError(f'sag_robot_info failed ({rc})')
  return dict(nu=out[0], obs_dim=out[1], nstep=out[2], nq=out[3], nv=out[4], dt=dt.value)


def task_desc_default(task_id):
  """The descriptor the library holds for one of the reference's 14 tasks (what the Python Task classes are tested against)."""
  t = TaskDesc()
  if load().sag_task_desc_default(int(task_id), C.byref(t)) != 0:
    raise SagError(f'no task {task_id}')
  return t.to_dict()


def task_desc_check(desc):
  """None, or what the library objects to in a descriptor dict (the field's name and the rule: include/sag.h)."""
  msg = load().sag_task_desc_check(C.byref(TaskDesc.from_dict(desc)))
  return None if msg is None else msg.decode()


def sample_layouts(robot, seeds, task_ids, config=None, first_episode=True, env_id0=0,
                   want_rng=False, nthreads=None, descs=None):
  """Native reset path: records for len(seeds) envs, env j drawn with
  np.random.RandomState(seeds[j]) semantics.  config: dict over World.DEFAULT keys.
  task_ids: one of the 14 reference tasks per env - or, with `descs` (a list of Task.descriptor() dicts), the index of
  env j's descriptor in that list.
  Returns (rec_f, rec_i, status[, rng states as numpy RandomState set_state tuples])."""
  lib = load()
  seeds = np.ascontiguousarray(np.asarray(seeds, np.int64) % 2**32, np.uint32)
  n = len(seeds)
  tids = np.ascontiguousarray(np.broadcast_to(np.asarray(task_ids, np.int32), (n,)))
  cfg = world_config(config)
  rf = np.zeros((n, REC_FLOATS), np.float32)
  ri = np.zeros((n, REC_INTS), np.int32)
  status = np.zeros(n, np.int32)
  key = np.zeros((n, 624), np.uint32) if want_rng else None
  pos = np.zeros(n, np.int32) if want_rng else None
  hg = np.zeros(n, np.int32) if want_rng else None
  g = np.zeros(n, np.float64) if want_rng else None
  if nthreads is None:
    nthreads = min(len(os.sched_getaffinity(0)), 16)
  rid = ROBOT_IDS[robot] if isinstance(robot, str) else robot
  tail = (C.byref(cfg), int(first_episode), env_id0, _ptr(rf, C.c_float), _ptr(ri, C.c_int32), _ptr(key, C.c_uint32),
          _ptr(pos, C.c_int32), _ptr(hg, C.c_int32), _ptr(g, C.c_double), _ptr(status, C.c_int32), nthreads)
  if descs is None:
    rc = lib.sag_sample_layouts(rid, n, _ptr(seeds, C.c_uint32), _ptr(tids, C.c_int32), *tail)
  else:
    for k, d in enumerate(descs):
      msg = task_desc_check(d)
      if msg:
        raise SagError(f'task descriptor {k}: {msg}')
    arr = (TaskDesc * len(descs))(*[TaskDesc.from_dict(d) for d in descs])
    rc = lib.sag_sample_layouts_desc(rid, n, _ptr(seeds, C.c_uint32), arr, len(descs), _ptr(tids, C.c_int32), *tail)
  if rc < 0:
    raise SagError(f'sag_sample_layouts failed ({rc}): a task descriptor exceeds the record capacity or is inconsistent')
  if want_rng:
    states = [('MT19937', key[j], int(pos[j]), int(hg[j]), float(g[j])) for j in range(n)]
    return rf, ri, status, states
  return rf, ri, status


def world_config(config=None):
  """sag_world_config from World.DEFAULT with the keys of `config` (a dict) applied."""
  lib = load()
  cfg = WorldConfig()
  lib.sag_world_config_default(C.byref(cfg))
  for k, v in (config or {}).items():
    if k in ('gremlins_size', 'gremlins_keepout', 'gremlins_travel', 'obstacles_size_noise_scale'):
      continue  # accepted by the reference, without effect (no task spawns gremlins)
    if not hasattr(cfg, k):
      raise KeyError(f'unknown world config key {k!r}')
    setattr(cfg, k, int(v) if k == 'random_bound' else float(v))
  return cfg


def device_count():
  return load().sag_device_count()


def _ptr(a, ctype):
  return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _addr(p):
  """What a descriptor's pointer field takes: the address in a c_void_p; an int or None as it is."""
  return p.value if isinstance(p, C.c_void_p) else p


class DeviceArray:
  """A view of device memory owned by a Context (the outputs of a device-resident env.step, BatchedSafeAdaptationGym
  with device_buffers=True): pointer, shape, dtype, strides.  It exports the CUDA array interface (version 2; HIP pointers are
  what PyTorch-ROCm and CuPy-ROCm expect there), so a learner wraps it without a copy - torch.as_tensor(a, device='cuda')
  -; `numpy()` downloads.  The memory is written on the context's stream: read it after env.wait() (or step(sync=True))."""

  def __init__(self, ctx, ptr, shape, dtype, strides=None, base=None):
    self.ctx, self.ptr, self.shape, self.dtype, self.strides = ctx, int(ptr), tuple(shape), np.dtype(dtype), strides
    self._base = base   # (ptr, shape) of the contiguous buffer a strided view lives in

  @property
  def __cuda_array_interface__(self):
    return {'shape': self.shape, 'typestr': self.dtype.str, 'data': (self.ptr, False), 'version': 2,
            'strides': self.strides}

  def numpy(self):
    if self.strides is None:
      return self.ctx.dev_download(C.c_void_p(self.ptr), self.shape, self.dtype)
    bptr, bshape = self._base
    full = self.ctx.dev_download(C.c_void_p(bptr), bshape, self.dtype)
    off = (self.ptr - bptr) // self.dtype.itemsize
    return np.lib.stride_tricks.as_strided(full.reshape(-1)[off:], self.shape, self.strides).copy()


def is_device_array(x):
  """Whether device_view() reads x: a DeviceArray, or a torch / cupy array on the GPU."""
  return isinstance(x, DeviceArray) or hasattr(x, '__cuda_array_interface__')


@functools.lru_cache(maxsize=1024)
def _dense_strides(shape, itemsize):
  strides = []
  for n in reversed(shape):
    strides.append(itemsize)
    itemsize *= max(n, 1)
  return tuple(reversed(strides))


def dense_strides(shape, dtype):
  """The strides in bytes of a C-contiguous array of that shape, as NumPy forms them; an axis of length 0 counts as 1, so an
  empty array keeps the strides of its rows.  (Cached: the learner's enqueue path asks for the same few shapes on every call.)"""
  return _dense_strides(tuple(shape), (dtype if isinstance(dtype, np.dtype) else np.dtype(dtype)).itemsize)


class DeviceView(collections.namedtuple('DeviceView', 'ptr shape strides dtype device')):
  """What device_view() makes of a device array: ptr (int), shape (tuple), strides (bytes, always concrete: the dense ones
  where the array names none), dtype (np.dtype), device (the index of the GPU the array says it lives on, or None)."""
  __slots__ = ()

  @property
  def contiguous(self):
    return self.strides == dense_strides(self.shape, self.dtype)


def device_view(x, what='device array', device=None):
  """The one reader of device arrays: a DeviceArray, or anything that exports __cuda_array_interface__ (a torch / cupy
  array on the GPU), as a DeviceView; TypeError for anything else.  `what` starts the messages.  With `device`, the index of
  the GPU the caller's context runs on, an array that names another one - torch's .device.index, cupy's .device.id, a
  DeviceArray's context - raises ValueError before a kernel can be handed its pointer.  Every entry point puts its own
  conditions (dtype, shape, pitch, alignment) on the record."""
  if isinstance(x, DeviceArray):
    ptr, shape, strides, dtype, where = x.ptr, x.shape, x.strides, x.dtype, getattr(x.ctx, 'device', None)
  else:
    cai = getattr(x, '__cuda_array_interface__', None)
    if cai is None:
      raise TypeError(f'{what}: {type(x).__name__} is not a device array')
    ptr, shape, strides, dtype = int(cai['data'][0]), tuple(cai['shape']), cai.get('strides'), np.dtype(cai['typestr'])
    dev = getattr(x, 'device', None)   # torch.device (.index) / cupy Device (.id); the interface itself names none
    where = getattr(dev, 'index', getattr(dev, 'id', None))
  if not isinstance(where, int):
    where = None
  elif device is not None and where != device:
    raise ValueError(f'{what} on device {where}: this shard runs on device {device}')
  # (tuple.__new__: the record is built on every enqueue, and a namedtuple's own constructor costs three times as much)
  return tuple.__new__(DeviceView, (ptr, shape, dense_strides(shape, dtype) if strides is None else tuple(strides), dtype, where))


def device_pointer(x, shape=None, device=None, dtype='<f4'):
  """Device pointer of anything device_view() reads.
  With `shape`, the array is what a step reads as its actions: float32 ('<f4'), exactly that shape, contiguous and - where
  the array says which device it lives on - on `device`.  Anything else raises ValueError before a kernel can read it
  (a float64 tensor would be read as float32 pairs, a short one past its end).  `dtype`: the element type required
  instead of float32 (uint8 for a reset mask)."""
  v = device_view(x, 'device_pointer')
  if not v.contiguous:
    raise ValueError('device actions must be contiguous')
  if shape is not None:
    want = np.dtype(dtype)
    if v.dtype != want:
      raise ValueError(f'device actions must be float32 (<f4), not {v.dtype.str}' if want == np.dtype('<f4') else
                       f'device array must be {want.str}, not {v.dtype.str}')
    if v.shape != tuple(shape):
      raise ValueError(f'device actions of shape {v.shape}: this shard steps {tuple(shape)}')
    if device is not None and v.device is not None and v.device != device:
      raise ValueError(f'device actions on device {v.device}: this shard runs on device {device}')
  return v.ptr


class DeviceBuffers:
  """The device allocations of one object on one Context, by name: bufs.alloc('mean', nbytes) -> the c_void_p, bufs['mean'],
  bufs.get('budget'), 'adv' in bufs.  close() frees each exactly once - or not at all once the context is destroyed: there is no
  handle left to free through - and the object closes itself when it is collected, so an owner's close() is a call of this one and a
  constructor that fails halfway leaks nothing."""

  def __init__(self, ctx):
    self.ctx, self._ptrs = ctx, {}

  def alloc(self, name, nbytes, zero=False):
    """A new allocation under a new name; zero=True fills it with zero bytes."""
    if name in self._ptrs:
      raise KeyError(f'device buffer {name!r} exists')
    p = self._ptrs[name] = self.ctx.dev_alloc(int(nbytes))
    if zero:
      self.ctx.dev_upload(p, np.zeros(int(nbytes), np.uint8))
    return p

  def __getitem__(self, name):
    return self._ptrs[name]

  def __contains__(self, name):
    return name in self._ptrs

  def get(self, name, default=None):
    return self._ptrs.get(name, default)

  def close(self):
    ptrs, self._ptrs = self._ptrs, {}
    if getattr(self.ctx, 'h', None):
      for p in ptrs.values():
        self.ctx.dev_free(p)

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass


class Context:
  """One GPU shard: owns the SoA world of n_envs environments on `device`."""

  def __init__(self, robot, n_envs, device=0, seed=0, max_hazards=MAX_HAZARDS,
               max_vases=MAX_VASES, max_pillars=MAX_PILLARS, max_buttons=MAX_BUTTONS,
               has_box=True):
    self.lib = load()
    self.robot = robot
    self.device = int(device)
    self.info = robot_info(robot)
    self.n_envs = int(n_envs)
    cfg = _Config(ABI_VERSION, ROBOT_IDS[robot], self.n_envs, device, max_hazards, max_vases,
                  max_pillars, max_buttons, int(has_box), 0, seed & (2**64 - 1))
    h = C.c_void_p()
    rc = self.lib.sag_create(C.byref(cfg), C.byref(h))
    if rc:
      raise SagError(f'sag_create failed ({rc}): {self.lib.sag_last_error(None).decode()}')
    self.h = h
    nu, od, n = self.info['nu'], self.info['obs_dim'], self.n_envs
    self._obs = np.zeros((n, od), np.float32)
    self._rew = np.zeros((n, 2), np.float32)
    self._cost = np.zeros(n, np.uint8)
    self._done = np.zeros(n, np.uint8)
    self._met = np.zeros(n, np.uint8)
    self._used = np.zeros(n, np.int32)

  def _check(self, rc, what):
    if rc:
      raise SagError(f'{what} failed ({rc}): {self.lib.sag_last_error(self.h).decode()}')

  def close(self):
    if getattr(self, 'h', None):
      self.lib.sag_destroy(self.h)
      self.h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # interpreter shutdown
      pass

  # -- records ---------------------------------------------------------------
  def _recs(self, env_ids, rec_f, rec_i):
    rec_f = np.ascontiguousarray(rec_f, np.float32).reshape(-1, REC_FLOATS)
    rec_i = np.ascontiguousarray(rec_i, np.int32).reshape(-1, REC_INTS)
    n = len(rec_f)
    assert len(rec_i) == n
    ids = None
    if env_ids is not None:
      ids = np.ascontiguousarray(env_ids, np.int32)
      assert len(ids) == n
    return ids, n, rec_f, rec_i

  def set_layout(self, rec_f, rec_i, env_ids=None):
    ids, n, rf, ri = self._recs(env_ids, rec_f, rec_i)
    self._check(self.lib.sag_set_layout(self.h, _ptr(ids, C.c_int32), n, _ptr(rf, C.c_float),
                                        _ptr(ri, C.c_int32)), 'sag_set_layout')

  def set_state(self, rec_f, rec_i, env_ids=None):
    ids, n, rf, ri = self._recs(env_ids, rec_f, rec_i)
    self._check(self.lib.sag_set_state(self.h, _ptr(ids, C.c_int32), n, _ptr(rf, C.c_float),
                                       _ptr(ri, C.c_int32)), 'sag_set_state')

  def get_state(self, env_ids=None):
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    n = self.n_envs if ids is None else len(ids)
    rf = np.zeros((n, REC_FLOATS), np.float32)
    ri = np.zeros((n, REC_INTS), np.int32)
    self._check(self.lib.sag_get_state(self.h, _ptr(ids, C.c_int32), n, _ptr(rf, C.c_float),
                                       _ptr(ri, C.c_int32)), 'sag_get_state')
    return rf, ri

  def reset(self, env_ids=None):
    ids = None if env_ids is None else np.ascontiguousarray(env_ids, np.int32)
    n = self.n_envs if ids is None else len(ids)
    self._check(self.lib.sag_reset(self.h, _ptr(ids, C.c_int32), n), 'sag_reset')

  # -- stepping --------------------------------------------------------------
  def step(self, actions, noise=None, tape=None, nstep=-1, want_tape_used=False):
    n, nu = self.n_envs, self.info['nu']
    a = np.ascontiguousarray(actions, np.float32).reshape(n, nu)
    nz = None if noise is None else np.ascontiguousarray(noise, np.float32).reshape(n, nu)
    tp, tl = None, 0
    if tape is not None:
      tp = np.ascontiguousarray(tape, np.uint32).reshape(n, -1)
      tl = tp.shape[1]
    self._check(
        self.lib.sag_step(self.h, _ptr(a, C.c_float), _ptr(nz, C.c_float), _ptr(tp, C.c_uint32), tl,
                          nstep, _ptr(self._obs, C.c_float), _ptr(self._rew, C.c_float),
                          _ptr(self._cost, C.c_uint8), _ptr(self._done, C.c_uint8),
                          _ptr(self._met, C.c_uint8),
                          _ptr(self._used, C.c_int32) if want_tape_used or tp is not None else None),
        'sag_step')
    return (self._obs.copy(), self._rew.copy(), self._cost.copy(), self._done.copy(),
            self._met.copy(), self._used.copy())

  def observe(self):
    self._check(self.lib.sag_observe(self.h, _ptr(self._obs, C.c_float)), 'sag_observe')
    return self._obs.copy()

  def set_ext_contacts(self, cost_contacts, btn_mask):
    """Contact results of the final state for the next step(nstep=0) (replayed episodes): per env the number of
    robot <-> obstacle contacts (-1: keep the device's own) and the mask of touched buttons
    (mujoco_bridge.py:177-191).  None, None clears a pending set."""
    if cost_contacts is None and btn_mask is None:
      self._check(self.lib.sag_set_ext_contacts(self.h, None, None), 'sag_set_ext_contacts')
      return
    cc = np.ascontiguousarray(cost_contacts, np.int32).reshape(self.n_envs)
    bm = np.ascontiguousarray(btn_mask, np.uint32).reshape(self.n_envs)
    self._check(self.lib.sag_set_ext_contacts(self.h, _ptr(cc, C.c_int32), _ptr(bm, C.c_uint32)), 'sag_set_ext_contacts')

  def lidar_cost(self, robot, points, group, hazard_size=0.2, want_bins=True):
    robot = np.ascontiguousarray(robot, np.float32).reshape(-1, 3)
    n = len(robot)
    group = np.ascontiguousarray(group, np.uint8).reshape(n, -1)
    K = group.shape[1]
    points = np.ascontiguousarray(points, np.float32).reshape(n, K, 2)
    lidar = np.zeros((n, 48), np.float32)
    bins = np.full((n, K), -1, np.int32) if want_bins else None
    cost = np.zeros(n, np.uint8)
    self._check(
        self.lib.sag_lidar_cost(self.h, n, K, _ptr(robot, C.c_float), _ptr(points, C.c_float),
                                _ptr(group, C.c_uint8), hazard_size, _ptr(lidar, C.c_float),
                                _ptr(bins, C.c_int32), _ptr(cost, C.c_uint8)), 'sag_lidar_cost')
    return lidar, bins, cost

  def lidar_cost_device(self, n, K, d_robot, d_points, d_group, d_lidar, d_bins, d_cost, hazard_size=0.2):
    """The same kernel on device buffers, asynchronous on the context stream (bench: kernel-only time)."""
    self._check(self.lib.sag_lidar_cost_device(self.h, n, K, d_robot, d_points, d_group, hazard_size, d_lidar, d_bins,
                                               d_cost), 'sag_lidar_cost_device')

  def set_tasks(self, descs, desc_of_env, config=None, env_id0=0):
    """Task descriptors (Task.descriptor() dicts), env i's descriptor index and the world config for sag_reset_device;
    env_id0 = the global id of this context's env 0."""
    for k, d in enumerate(descs):
      msg = task_desc_check(d)
      if msg:
        raise SagError(f'task descriptor {k}: {msg}')
    arr = (TaskDesc * len(descs))(*[TaskDesc.from_dict(d) for d in descs])
    doe = np.ascontiguousarray(np.broadcast_to(np.asarray(desc_of_env, np.int32), (self.n_envs,)))
    cfg = world_config(config)
    self._check(self.lib.sag_set_tasks(self.h, arr, len(descs), _ptr(doe, C.c_int32), C.byref(cfg), int(env_id0)),
                'sag_set_tasks')

  def reset_device(self, first_episode=False, episode0=0, d_mask=None, want_status=True, want_bound=True):
    """New layouts sampled and installed on the device (sag_reset_device).  d_mask: device pointer of [n_envs] bytes, or
    None for every env.  -> (number of envs that failed, status [n_envs] i32 or None, bound [n_envs] f32 or None)."""
    status = np.zeros(self.n_envs, np.int32) if want_status else None
    bound = np.zeros(self.n_envs, np.float32) if want_bound else None
    rc = self.lib.sag_reset_device(self.h, int(bool(first_episode)), int(episode0), d_mask, _ptr(status, C.c_int32),
                                   _ptr(bound, C.c_float))
    if rc < 0:
      self._check(rc, 'sag_reset_device')
    return rc, status, bound

  def reset_device_async(self, d_mask, d_obs=None):
    """sag_reset_device_async: a later-episode masked device reset enqueued on the context stream - no wait, no host copy.
    d_mask: device pointer of [n_envs] bytes or None (every env); d_obs: device pointer of [n_envs][obs_dim] f32 whose rows
    of the reset envs receive their first observation, or None.  Failures are data: reset_counts()."""
    self._check(self.lib.sag_reset_device_async(self.h, d_mask, d_obs), 'sag_reset_device_async')

  def reset_counts(self, clear=False):
    """(envs reset, envs whose sampling failed) by reset_device_async since the last clear; joins the stream."""
    a, b = C.c_uint64(), C.c_uint64()
    self._check(self.lib.sag_reset_device_counts(self.h, int(bool(clear)), C.byref(a), C.byref(b)), 'sag_reset_device_counts')
    return a.value, b.value

  def episode_track(self, d_reward, d_cost, d_done, d_met, max_steps, d_ended, d_episode):
    """sag_episode_track_device: the episode bookkeeping of one step on device buffers, enqueued on the context stream."""
    self._check(self.lib.sag_episode_track_device(self.h, d_reward, d_cost, d_done, d_met, int(max_steps), d_ended, d_episode),
                'sag_episode_track_device')

  def episode_clear(self, d_mask=None):
    self._check(self.lib.sag_episode_clear(self.h, d_mask), 'sag_episode_clear')

  def copy_rows(self, d_mask, row_bytes, d_src, d_dst):
    """sag_copy_rows_device: row i (row_bytes bytes, a multiple of 16) of d_src -> row i of d_dst for the envs with a non-zero
    byte of d_mask (device pointer of [n_envs] bytes; None: every env), enqueued on the context stream - no wait, no host
    copy.  The other rows of d_dst are not written."""
    self._check(self.lib.sag_copy_rows_device(self.h, d_mask, int(row_bytes), d_src, d_dst), 'sag_copy_rows_device')

  def append_rows(self, d_mask, row_bytes, d_src, d_store, capacity, d_count, restart, d_slot):
    """sag_append_rows_device: row i of d_src -> the next free slot of d_store ([capacity] rows) for the envs with a non-zero
    byte of d_mask, d_slot[i] = that slot (-1: not set, or the store was full), d_count = slots claimed so far (one device
    int32, zeroed first when restart), enqueued on the context stream - no wait, no host copy."""
    self._check(self.lib.sag_append_rows_device(self.h, d_mask, int(row_bytes), d_src, d_store, int(capacity), d_count,
                                                int(bool(restart)), d_slot), 'sag_append_rows_device')

  def gae(self, T, pitch, d_reward, d_cost, d_ended, d_value, d_adv, d_ret, gamma, lam, d_cvalue=None, d_cadv=None, d_cret=None,
          cost_gamma=None, cost_lam=None, d_slot=None, capacity=0, d_final_value=None, d_final_cvalue=None):
    """sag_gae_device: advantages and returns over T stored steps of [T][pitch] arrays, for the reward channel and (d_cvalue
    given) the cost channel, enqueued on the context stream.  Pointers are c_void_p, ints or None; cost_gamma / cost_lam
    default to gamma / lam."""
    d = GaeDesc(int(T), int(pitch), int(capacity), 0, float(gamma), float(lam), float(gamma if cost_gamma is None else cost_gamma),
                float(lam if cost_lam is None else cost_lam), *[_addr(x) for x in (d_reward, d_cost, d_ended, d_value, d_cvalue, d_slot,
                                                                                 d_final_value, d_final_cvalue, d_adv, d_ret, d_cadv, d_cret)])
    self._check(self.lib.sag_gae_device(self.h, C.byref(d)), 'sag_gae_device')

  def _policy_desc(self, n_rows, hidden, d_params, d_obs, logp_const, d_actions, d_logp, d_value, d_cvalue, activation, flags, draw, row0,
                   obs_pitch):
    return PolicyDesc(int(n_rows), int(hidden), int(activation), int(flags), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), 0,
                      int(draw) & 0xffffffff, int(row0) & 0xffffffff, float(logp_const),
                      *[_addr(x) for x in (d_params, d_obs, d_actions, d_logp, d_value, d_cvalue)])

  def _policy_grad_desc(self, n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale, d_cadv,
                        d_cret, clip, vf_coef, cvf_coef, ent_coef, adv_affine, cadv_affine, activation, flags, max_blocks, obs_pitch):
    return PolicyGradDesc(int(n_rows), int(n_planes), int(pitch), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), int(hidden),
                          int(activation), int(flags), int(max_blocks), float(clip), float(vf_coef), float(cvf_coef), float(ent_coef),
                          float(adv_affine[0]), float(adv_affine[1]), float(cadv_affine[0]), float(cadv_affine[1]), float(scale), 0.0,
                          *[_addr(x) for x in (d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_cadv, d_cret, d_grad)])

  def policy_forward(self, n_rows, hidden, d_params, d_obs, logp_const=0.0, d_actions=None, d_logp=None, d_value=None, d_cvalue=None,
                     activation=POLICY_RELU, flags=0, draw=0, row0=0, obs_pitch=None):
    """sag_policy_forward_device: the fused actor-critic forward of n_rows observation rows (obs_pitch floats apart; default
    obs_dim) under the parameters at d_params (the header has their layout and the arithmetic), enqueued on the context stream
    - no wait, no host copy.  Pointers are c_void_p, ints or None; an output that is None is not written."""
    d = self._policy_desc(n_rows, hidden, d_params, d_obs, logp_const, d_actions, d_logp, d_value, d_cvalue, activation, flags, draw, row0,
                          obs_pitch)
    self._check(self.lib.sag_policy_forward_device(self.h, C.byref(d)), 'sag_policy_forward_device')

  def policy_forward_norm(self, n_rows, hidden, d_params, d_obs, d_table, clip=10.0, logp_const=0.0, d_actions=None, d_logp=None,
                          d_value=None, d_cvalue=None, activation=POLICY_RELU, flags=0, draw=0, row0=0, obs_pitch=None):
    """sag_policy_forward_norm_device: policy_forward with every observation element replaced, where its row is staged, by
    clamp((x - mean) * rstd, -clip, clip) under d_table = mean [obs_dim] then rstd [obs_dim] (what obs_stats writes)."""
    d = self._policy_desc(n_rows, hidden, d_params, d_obs, logp_const, d_actions, d_logp, d_value, d_cvalue, activation, flags, draw, row0,
                          obs_pitch)
    self._check(self.lib.sag_policy_forward_norm_device(self.h, C.byref(d), _addr(d_table), float(clip)), 'sag_policy_forward_norm_device')

  def policy_backward(self, n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale,
                      d_cadv=None, d_cret=None, clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.0, adv_affine=(1.0, 0.0),
                      cadv_affine=(0.0, 0.0), activation=POLICY_RELU, flags=0, max_blocks=0, obs_pitch=None, rows=None):
    """sag_policy_backward_device: the PPO-Lagrangian gradient and 8 statistics of n_planes x n_rows stored rows (planes `pitch`
    rows apart) into d_grad [n_params + 8], enqueued on the context stream - no wait, no host copy.  The header defines the
    function; adv_affine = (adv_mul, adv_sub), cadv_affine likewise.  Pointers are c_void_p, ints or None.
    rows=(d_rows, n_index): sag_policy_backward_rows_device - the batch is the n_index logical elements that the device int32
    list at d_rows names, gathered in place."""
    d = self._policy_grad_desc(n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale, d_cadv,
                               d_cret, clip, vf_coef, cvf_coef, ent_coef, adv_affine, cadv_affine, activation, flags, max_blocks, obs_pitch)
    if rows is not None:
      self._check(self.lib.sag_policy_backward_rows_device(self.h, C.byref(d), _addr(rows[0]), int(rows[1]), None, 0.0),
                  'sag_policy_backward_rows_device')
      return
    self._check(self.lib.sag_policy_backward_device(self.h, C.byref(d)), 'sag_policy_backward_device')

  def policy_backward_norm(self, n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale,
                           d_table, obs_clip=10.0, d_cadv=None, d_cret=None, clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.0,
                           adv_affine=(1.0, 0.0), cadv_affine=(0.0, 0.0), activation=POLICY_RELU, flags=0, max_blocks=0, obs_pitch=None,
                           rows=None):
    """sag_policy_backward_norm_device: policy_backward over observations normalised under d_table and clamped to
    +-obs_clip where they are staged, as policy_forward_norm does.  rows=(d_rows, n_index): sag_policy_backward_rows_device
    with the table."""
    d = self._policy_grad_desc(n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale, d_cadv,
                               d_cret, clip, vf_coef, cvf_coef, ent_coef, adv_affine, cadv_affine, activation, flags, max_blocks, obs_pitch)
    if rows is not None:
      self._check(self.lib.sag_policy_backward_rows_device(self.h, C.byref(d), _addr(rows[0]), int(rows[1]), _addr(d_table), float(obs_clip)),
                  'sag_policy_backward_rows_device')
      return
    self._check(self.lib.sag_policy_backward_norm_device(self.h, C.byref(d), _addr(d_table), float(obs_clip)), 'sag_policy_backward_norm_device')

  def permutation(self, n, draw, d_index):
    """sag_permutation_device: d_index[0 ... n) (device int32) = a keyed pseudo-random permutation of 0 ... n - 1 under the
    context key and `draw` (the header defines it bit for bit); enqueued on the context stream - no wait, no host copy."""
    self._check(self.lib.sag_permutation_device(self.h, int(n), int(draw) & 0xffffffff, _addr(d_index)), 'sag_permutation_device')

  def obs_stats(self, d_state, d_table, d_obs=None, n_rows=0, n_planes=0, pitch=0, obs_pitch=None, eps=1e-8, max_blocks=0, table_only=False):
    """sag_obs_stats_device: the per-column moments of n_planes x n_rows observation rows (planes `pitch` rows, rows obs_pitch
    floats apart) merged into d_state = {count, mean [obs_dim], M2 [obs_dim]} float64, and d_table = mean, rstd float32 made from
    it; table_only=True rewrites the table from the state and reads no observations.  Enqueued on the context stream."""
    d = ObsStatsDesc(int(n_rows), int(n_planes), int(pitch), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), int(max_blocks),
                     OBS_STATS_TABLE_ONLY if table_only else 0, float(eps), 0.0, _addr(d_obs), _addr(d_state), _addr(d_table))
    self._check(self.lib.sag_obs_stats_device(self.h, C.byref(d)), 'sag_obs_stats_device')

  def adam(self, n, d_param, d_grad, d_m, d_v, step, beta1=0.9, beta2=0.999, eps=1e-8, clamp_first=None, clamp_lo=0.0):
    """sag_adam_device: one Adam step on n float32 elements (the header has the chain; `step` is the bias-corrected learning
    rate), elements from clamp_first on kept at or above clamp_lo; enqueued on the context stream."""
    d = AdamDesc(int(n), int(n if clamp_first is None else clamp_first), float(beta1), float(beta2), float(eps), float(step),
                 float(clamp_lo), 0.0, *[_addr(x) for x in (d_param, d_grad, d_m, d_v)])
    self._check(self.lib.sag_adam_device(self.h, C.byref(d)), 'sag_adam_device')

  def moments(self, n_rows, n_planes, pitch, d_x, d_out, d_mask=None, stride=1, eps=1e-8, max_blocks=0):
    """sag_moments_device: d_out[4] = {count, mean, var, 1 / (sqrt(var) + eps)} of the n_planes x n_rows elements of d_x (planes
    `pitch` rows apart, elements `stride` floats apart) whose byte of d_mask [n_planes][pitch] is non-zero (None: all); enqueued
    on the context stream, the result stays on the device."""
    d = MomentsDesc(int(n_rows), int(n_planes), int(pitch), int(stride), int(max_blocks), 0, float(eps), 0.0, _addr(d_x), _addr(d_mask), _addr(d_out))
    self._check(self.lib.sag_moments_device(self.h, C.byref(d)), 'sag_moments_device')

  def advantage_mix(self, n_rows, n_planes, pitch, d_adv, d_out, d_cadv=None, adv_mode=ADV_RAW, cadv_mode=ADV_RAW, d_adv_mom=None,
                    d_cadv_mom=None, d_lambda=None, cost_weight=0.0):
    """sag_advantage_mix_device: d_out = norm(adv) - lambda * norm(cadv) elementwise (the header has the chain), the moments
    arrays as moments() writes them, lambda = d_lambda[0] or cost_weight; enqueued on the context stream."""
    d = AdvantageMixDesc(int(n_rows), int(n_planes), int(pitch), 0, int(adv_mode), int(cadv_mode), float(cost_weight), 0.0,
                         *[_addr(x) for x in (d_adv, d_cadv, d_adv_mom, d_cadv_mom, d_lambda, d_out)])
    self._check(self.lib.sag_advantage_mix_device(self.h, C.byref(d)), 'sag_advantage_mix_device')

  def lagrange(self, d_mom, d_state, lr, budget, lambda_max=float('inf')):
    """sag_lagrange_device: d_state[4] = {lambda, mean cost, episodes, updates} takes one step lambda += lr * (mean - budget),
    kept in [0, lambda_max], from the moments at d_mom (no step where their count is 0); enqueued on the context stream."""
    d = LagrangeDesc(float(lr), float(budget), float(lambda_max), 0.0, _addr(d_mom), _addr(d_state))
    self._check(self.lib.sag_lagrange_device(self.h, C.byref(d)), 'sag_lagrange_device')

  def grad_clip(self, n, d_grad, d_out, max_norm, max_blocks=0):
    """sag_grad_clip_device: d_grad[0 ... n) scaled in place by min(1, max_norm / (norm + 1e-6)), d_out[2] = {norm, factor};
    enqueued on the context stream."""
    d = GradClipDesc(int(n), int(max_blocks), float(max_norm), 0.0, _addr(d_grad), _addr(d_out))
    self._check(self.lib.sag_grad_clip_device(self.h, C.byref(d)), 'sag_grad_clip_device')

  def fork_device(self, d_src, source=None, same_stream=False, flags=None):
    """sag_fork_device: env i takes the complete state of env d_src[i] of `source` (a Context on the same device; default:
    this one), enqueued on this context's stream - no wait, no host copy.  d_src: device pointer of [n_envs] int32,
    negative = keep.  Rejections (an index past the source's envs, a source that the call overwrites) are data:
    fork_counts().  same_stream: the env id is copied too (SAG_FORK_SAME_STREAM); `flags` overrides the flag word."""
    if flags is None:
      flags = FORK_SAME_STREAM if same_stream else 0
    self._check(self.lib.sag_fork_device(self.h, (self if source is None else source).h, d_src, int(flags)), 'sag_fork_device')

  def fork_counts(self, clear=False):
    """(envs copied, envs rejected) by fork_device into this context since the last clear; joins the stream."""
    a, b = C.c_uint64(), C.c_uint64()
    self._check(self.lib.sag_fork_counts(self.h, int(bool(clear)), C.byref(a), C.byref(b)), 'sag_fork_counts')
    return a.value, b.value

  def wait_for(self, producer):
    """sag_wait_for: this context's stream waits for what is enqueued on `producer`'s (a Context on the same device); no
    host wait."""
    self._check(self.lib.sag_wait_for(self.h, producer.h), 'sag_wait_for')

  # -- shooting planner (include/sag.h; planner.ShootingPlanner drives these) -------
  def plan_sample(self, K, H, d_mean, d_sigma, draw, d_plans):
    """sag_plan_sample_device: plans [H][n_envs][nu] = clamp(mean + sigma * z), candidate 0 of each group of K the mean."""
    self._check(self.lib.sag_plan_sample_device(self.h, int(K), int(H), d_mean, d_sigma, int(draw) & 0xffffffff, d_plans),
                'sag_plan_sample_device')

  def plan_score(self, d_plans, H, gamma, d_score):
    """sag_plan_score_device: H steps of this context on the plans, without observations; score [n_envs][4] = discounted
    return, discounted cost, steps alive, goals met.  The context's state advances by H steps."""
    self._check(self.lib.sag_plan_score_device(self.h, d_plans, int(H), float(gamma), d_score), 'sag_plan_score_device')

  def plan_refit(self, K, H, E, d_plans, d_score, d_budget, sigma_min, d_mean, d_sigma, d_best, d_best_score=None):
    """sag_plan_refit_device: rank each group's K candidates under d_budget ([G] floats or None), refit mean / sigma to the
    E elites, d_best [G] int32 = the first candidate."""
    self._check(self.lib.sag_plan_refit_device(self.h, int(K), int(H), int(E), d_plans, d_score, d_budget, float(sigma_min), d_mean,
                                               d_sigma, d_best, d_best_score), 'sag_plan_refit_device')

  def plan_shift(self, G, H, d_mean, d_sigma, sigma_init):
    """sag_plan_shift_device: mean[h] = mean[h + 1], last row 0, sigma = sigma_init."""
    self._check(self.lib.sag_plan_shift_device(self.h, int(G), int(H), d_mean, d_sigma, float(sigma_init)), 'sag_plan_shift_device')

  def plan_clear(self, G, H, d_mask, d_mean, d_sigma, sigma_init):
    """sag_plan_clear_device: mean = 0, sigma = sigma_init for the groups of d_mask ([G] bytes; None: all)."""
    self._check(self.lib.sag_plan_clear_device(self.h, int(G), int(H), d_mask, d_mean, d_sigma, float(sigma_init)),
                'sag_plan_clear_device')

  def set_seed(self, seed):
    """Key of the device-side generator of throughput mode (env.seed())."""
    self._check(self.lib.sag_set_seed(self.h, int(seed) & (2**64 - 1)), 'sag_set_seed')

  # -- device-resident stepping (bench harness / GPU learners) -----------------
  def dev_alloc(self, nbytes):
    p = C.c_void_p()
    self._check(self.lib.sag_dev_alloc(self.h, nbytes, C.byref(p)), 'sag_dev_alloc')
    return p

  def dev_free(self, p):
    self._check(self.lib.sag_dev_free(self.h, p), 'sag_dev_free')

  def dev_upload(self, dst, arr):
    arr = np.ascontiguousarray(arr)
    self._check(self.lib.sag_dev_upload(self.h, dst, arr.ctypes.data_as(C.c_void_p), arr.nbytes),
                'sag_dev_upload')

  def dev_download(self, src, shape, dtype):
    out = np.zeros(shape, dtype)
    self._check(self.lib.sag_dev_download(self.h, out.ctypes.data_as(C.c_void_p), src, out.nbytes),
                'sag_dev_download')
    return out

  def dev_fill_actions(self, d_actions, step_index):
    self._check(self.lib.sag_dev_fill_actions(self.h, d_actions, step_index), 'sag_dev_fill_actions')

  def step_device(self, d_actions, d_noise=None, nstep=-1, d_obs=None, d_reward=None, d_cost=None,
                  d_done=None, d_goal_met=None):
    self._check(
        self.lib.sag_step_device(self.h, d_actions, d_noise, nstep, d_obs, d_reward, d_cost, d_done,
                                 d_goal_met), 'sag_step_device')

  def wait(self):
    self._check(self.lib.sag_wait(self.h), 'sag_wait')

  def enable_timing(self, on=True):
    self._check(self.lib.sag_enable_timing(self.h, int(on)), 'sag_enable_timing')

  def debug_cycles(self, reset=False, worst=False):
    """[3 kernel forms, 15 sections + wavefront count] clock ticks summed over wavefronts (library built with -DSAG_CYCLES);
    worst=True: the sections of the slowest wavefront since the last reset (last column: its total) and its block index per form."""
    out = (C.c_uint64 * 291)()
    self._check(self.lib.sag_debug_cycles(self.h, int(reset), out, 291), 'sag_debug_cycles')
    a = np.array(out[:], np.uint64)
    self.cycles_hist = a[99:291].reshape(3, 64)   # wavefronts by total ticks: bucket b = [2^((b + 40) / 4), 2^((b + 41) / 4))
    return (a[48:96].reshape(3, 16), a[96:99]) if worst else a[:48].reshape(3, 16)

  def render_rgb(self):
    """[n_envs, 64, 64, 3] uint8: the robots' first-person camera images (rgb_observation)."""
    img = np.zeros((self.n_envs, 64, 64, 3), np.uint8)
    self._check(self.lib.sag_render_rgb(self.h, img.ctypes.data_as(C.POINTER(C.c_uint8))), 'sag_render_rgb')
    return img

  CAMERAS = {'vision': 0, 'fixednear': 1, 'fixedfar': 2, 'track': 3}
  OUTPUTS = {'depth': 1, 'segmentation': 2}   # enum sag_render_output
  DEPTH_SKY = 50.0                            # SAG_DEPTH_SKY: what a sky pixel of the depth image holds

  def _env_ids(self, envs, who):
    """envs of render(): None, or the indices as a contiguous int32 array (the library checks them against n_envs)."""
    if envs is None:
      return None
    ids = np.asarray(envs)
    if ids.ndim != 1 or (ids.size and ids.dtype.kind not in 'iu'):
      raise ValueError(f'envs: a 1-D sequence of integer indices, not {ids.dtype} {ids.shape}')
    if ids.size and (int(ids.min()) < -2**31 or int(ids.max()) >= 2**31):   # (must not wrap into range; the library checks the rest)
      raise SagError(f'{who}: an env index outside int32 ({self.n_envs} envs)')
    return np.ascontiguousarray(ids, np.int32)

  def render(self, camera='fixedfar', width=256, height=256, overlays=True, envs=None, output='rgb'):
    """[n_envs, height, width, 3] uint8 from one of the scene's cameras (name or id), optionally with the lidar
    rings and the cost indicator of the last step.  envs: int32 indices of the envs to render, any order, duplicates
    allowed (sag_render_envs) -> [len(envs), height, width, 3], row j = env envs[j]; device work and staging are for
    len(envs) images only.
    output: 'rgb'; 'depth' -> [rows, height, width] float32, the distance of the nearest surface from the camera plane in
    metres (sky: DEPTH_SKY); 'segmentation' -> [rows, height, width, 2] int32, (instance, class) of that surface (enum
    sag_seg_class; sky (-1, -1)) (sag_render_aux)."""
    cam = self.CAMERAS[camera] if isinstance(camera, str) else int(camera)
    if output != 'rgb' and output not in self.OUTPUTS:
      raise ValueError(f'output: one of {["rgb"] + sorted(self.OUTPUTS)}, not {output!r}')
    out = self.OUTPUTS.get(output, 0)
    who = 'sag_render_aux' if out else ('sag_render' if envs is None else 'sag_render_envs')
    ids = self._env_ids(envs, who)
    rows = self.n_envs if ids is None else len(ids)
    pixel, dtype = (((3,), np.uint8), ((), np.float32), ((2,), np.int32))[out]
    img = np.zeros((rows, int(height), int(width)) + pixel, dtype)
    args = (cam, int(width), int(height), 1 if overlays else 0)
    p, idp = _ptr(img, C.c_uint8), _ptr(ids, C.c_int32)
    if out:
      rc = self.lib.sag_render_aux(self.h, out, *args, idp, rows, p) if rows else 0   # (an empty list is not NULL, which would mean every env)
    else:
      rc = self.lib.sag_render(self.h, *args, p) if ids is None else self.lib.sag_render_envs(self.h, *args, idp, rows, p)
    self._check(rc, who)
    return img

  def render_aux_device(self, output, d_out, d_mask=None, camera='vision', width=64, height=64, overlays=False, d_obs=None, d_cost=None):
    """sag_render_aux_device: the 'depth' ([n_envs][height][width] float32, d_out aligned to 4 bytes) or 'segmentation'
    ([n_envs][height][width][2] int32, aligned to 8) images of the envs with a non-zero byte of d_mask (device pointer of
    [n_envs] bytes; None: every env) into their own rows of d_out, enqueued on the context stream; the other rows are not
    written.  d_obs / d_cost: what the overlays show (device pointers or None)."""
    cam = self.CAMERAS[camera] if isinstance(camera, str) else int(camera)
    out = self.OUTPUTS[output] if isinstance(output, str) else int(output)
    self._check(self.lib.sag_render_aux_device(self.h, out, cam, int(width), int(height), 1 if overlays else 0, d_obs, d_cost,
                                               d_mask, d_out), 'sag_render_aux_device')

  def render_rows_device(self, d_mask, d_out, camera='vision', width=64, height=64, overlays=False, d_obs=None, d_cost=None):
    """sag_render_rows_device: the images of the envs with a non-zero byte of d_mask (device pointer of [n_envs] bytes; None:
    every env) into their own rows of d_out (device pointer of [n_envs][height][width][3] bytes), enqueued on the context
    stream; the other rows are not written.  d_obs / d_cost: what the overlays show (device pointers or None)."""
    cam = self.CAMERAS[camera] if isinstance(camera, str) else int(camera)
    self._check(self.lib.sag_render_rows_device(self.h, cam, int(width), int(height), 1 if overlays else 0, d_obs, d_cost,
                                                d_mask, d_out), 'sag_render_rows_device')

  def debug_doggo_coop(self):
    out = np.zeros((self.n_envs, 760), np.float64)
    self._check(self.lib.sag_debug_doggo_coop(self.h, out.ctypes.data_as(C.POINTER(C.c_double))), 'sag_debug_doggo_coop')
    return out[:, :361].reshape(-1, 19, 19), out[:, 361:380], out[:, 380:399], out[:, 399:].reshape(-1, 19, 19)

  def render_rgb_device(self, d_out):
    self._check(self.lib.sag_render_rgb_device(self.h, d_out), 'sag_render_rgb_device')

  def busy_count(self):
    n = C.c_int32()
    self._check(self.lib.sag_busy_count(self.h, C.byref(n)), 'sag_busy_count')
    return n.value

  def kernel_time_ms(self, reset=False):
    ms, n = C.c_double(), C.c_int64()
    self._check(self.lib.sag_kernel_time_ms(self.h, int(reset), C.byref(ms), C.byref(n)),
                'sag_kernel_time_ms')
    return ms.value, n.value
