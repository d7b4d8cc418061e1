"""ctypes binding of libsag.so (include/sag.h).  NumPy only - no torch on the path.

There is no CPU fallback: if the HIP library is missing or no MI355X is visible,
every entry point raises."""
import ctypes as C
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

EXPORTS = [
    'sag_robot_info', 'sag_create', 'sag_destroy', 'sag_last_error', 'sag_set_layout',
    'sag_reset', 'sag_get_state', 'sag_set_state', 'sag_step', 'sag_step_device', 'sag_wait',
    'sag_observe', 'sag_set_ext_contacts', 'sag_lidar_cost', 'sag_lidar_cost_device', 'sag_set_seed', 'sag_dev_alloc', 'sag_dev_free', 'sag_dev_upload',
    'sag_dev_download', 'sag_dev_fill_actions', 'sag_kernel_time_ms', 'sag_enable_timing', 'sag_busy_count', 'sag_debug_cycles', 'sag_render_rgb', 'sag_render_rgb_device', 'sag_render', 'sag_render_device', 'sag_render_rows_device', 'sag_render_envs', 'sag_render_aux', 'sag_render_aux_device', 'sag_debug_doggo_coop',
    'sag_device_count', 'sag_world_config_default', 'sag_sample_layouts', 'sag_sample_layouts_desc', 'sag_task_desc_default', 'sag_task_desc_check',
    'sag_set_tasks', 'sag_reset_device', 'sag_reset_device_async', 'sag_reset_device_counts', 'sag_episode_track_device',
    'sag_episode_clear', 'sag_copy_rows_device', 'sag_fork_device', 'sag_fork_counts', 'sag_wait_for', 'sag_plan_sample_device', 'sag_plan_score_device',
    'sag_plan_refit_device', 'sag_plan_shift_device', 'sag_plan_clear_device', 'sag_append_rows_device', 'sag_gae_device',
    'sag_policy_forward_device', 'sag_policy_backward_device', 'sag_adam_device',
    'sag_moments_device', 'sag_advantage_mix_device', 'sag_lagrange_device', 'sag_grad_clip_device',
    'sag_obs_stats_device', 'sag_policy_forward_norm_device', 'sag_policy_backward_norm_device',
    'sag_permutation_device', 'sag_policy_backward_rows_device'
]


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
  vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
  up, bp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
  lib.sag_last_error.restype = C.c_char_p
  lib.sag_last_error.argtypes = [vp]
  lib.sag_robot_info.argtypes = [C.c_int32, ip, C.POINTER(C.c_double)]
  lib.sag_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
  lib.sag_destroy.argtypes = [vp]
  lib.sag_set_layout.argtypes = [vp, ip, C.c_int32, fp, ip]
  lib.sag_set_state.argtypes = [vp, ip, C.c_int32, fp, ip]
  lib.sag_get_state.argtypes = [vp, ip, C.c_int32, fp, ip]
  lib.sag_reset.argtypes = [vp, ip, C.c_int32]
  lib.sag_step.argtypes = [vp, fp, fp, up, C.c_int32, C.c_int32, fp, fp, bp, bp, bp, ip]
  lib.sag_step_device.argtypes = [vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
  lib.sag_wait.argtypes = [vp]
  lib.sag_observe.argtypes = [vp, fp]
  lib.sag_set_ext_contacts.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]
  lib.sag_lidar_cost.argtypes = [vp, C.c_int32, C.c_int32, fp, fp, bp, C.c_float, fp, ip, bp]
  lib.sag_lidar_cost_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_float, vp, vp, vp]
  lib.sag_set_seed.argtypes = [vp, C.c_uint64]
  lib.sag_dev_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
  lib.sag_dev_free.argtypes = [vp, vp]
  lib.sag_dev_upload.argtypes = [vp, vp, vp, C.c_uint64]
  lib.sag_dev_download.argtypes = [vp, vp, vp, C.c_uint64]
  lib.sag_dev_fill_actions.argtypes = [vp, vp, C.c_uint32]
  lib.sag_kernel_time_ms.argtypes = [vp, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
  lib.sag_enable_timing.argtypes = [vp, C.c_int32]
  lib.sag_busy_count.argtypes = [vp, C.POINTER(C.c_int32)]
  lib.sag_render_rgb.argtypes = [vp, C.POINTER(C.c_uint8)]
  lib.sag_render_rgb_device.argtypes = [vp, vp]
  lib.sag_render.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]
  lib.sag_render_device.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
  lib.sag_render_rows_device.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
  lib.sag_render_envs.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, C.c_int32, C.POINTER(C.c_uint8)]
  lib.sag_render_aux_device.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
  lib.sag_render_aux.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, ip, C.c_int32, vp]
  lib.sag_debug_doggo_coop.argtypes = [vp, C.POINTER(C.c_double)]
  lib.sag_debug_cycles.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), C.c_int32]
  lib.sag_world_config_default.argtypes = [C.POINTER(WorldConfig)]
  lib.sag_world_config_default.restype = None
  lib.sag_sample_layouts.argtypes = [C.c_int32, C.c_int32, up, ip, C.POINTER(WorldConfig), C.c_int32,
                                     C.c_int32, fp, ip, up, ip, ip, C.POINTER(C.c_double), ip, C.c_int32]
  lib.sag_set_tasks.argtypes = [vp, vp, C.c_int32, ip, C.POINTER(WorldConfig), C.c_int32]
  lib.sag_reset_device.argtypes = [vp, C.c_int32, C.c_int32, vp, ip, fp]
  lib.sag_reset_device_async.argtypes = [vp, vp, vp]
  lib.sag_reset_device_counts.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
  lib.sag_episode_track_device.argtypes = [vp, vp, vp, vp, vp, C.c_int32, vp, vp]
  lib.sag_episode_clear.argtypes = [vp, vp]
  lib.sag_copy_rows_device.argtypes = [vp, vp, C.c_int32, vp, vp]
  lib.sag_fork_device.argtypes = [vp, vp, vp, C.c_int32]
  lib.sag_fork_counts.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
  lib.sag_wait_for.argtypes = [vp, vp]
  lib.sag_plan_sample_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_uint32, vp]
  lib.sag_plan_score_device.argtypes = [vp, vp, C.c_int32, C.c_float, vp]
  lib.sag_plan_refit_device.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, C.c_float, vp, vp, vp, vp]
  lib.sag_plan_shift_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_float]
  lib.sag_plan_clear_device.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, C.c_float]
  lib.sag_append_rows_device.argtypes = [vp, vp, C.c_int32, vp, vp, C.c_int32, vp, C.c_int32, vp]
  lib.sag_gae_device.argtypes = [vp, C.POINTER(GaeDesc)]
  lib.sag_policy_forward_device.argtypes = [vp, C.POINTER(PolicyDesc)]
  lib.sag_policy_backward_device.argtypes = [vp, C.POINTER(PolicyGradDesc)]
  lib.sag_adam_device.argtypes = [vp, C.POINTER(AdamDesc)]
  lib.sag_moments_device.argtypes = [vp, C.POINTER(MomentsDesc)]
  lib.sag_advantage_mix_device.argtypes = [vp, C.POINTER(AdvantageMixDesc)]
  lib.sag_lagrange_device.argtypes = [vp, C.POINTER(LagrangeDesc)]
  lib.sag_grad_clip_device.argtypes = [vp, C.POINTER(GradClipDesc)]
  # (a SAG_LIB library of an earlier commit lacks some of these: it still loads for an A/B run of the plain paths, and a call
  # of one of them raises AttributeError)
  for name, sig in (('sag_obs_stats_device', [vp, C.POINTER(ObsStatsDesc)]),
                    ('sag_policy_forward_norm_device', [vp, C.POINTER(PolicyDesc), vp, C.c_float]),
                    ('sag_policy_backward_norm_device', [vp, C.POINTER(PolicyGradDesc), vp, C.c_float]),
                    ('sag_permutation_device', [vp, C.c_int32, C.c_uint32, vp]),
                    ('sag_policy_backward_rows_device', [vp, C.POINTER(PolicyGradDesc), vp, C.c_int32, vp, C.c_float])):
    if hasattr(lib, name):
      getattr(lib, name).argtypes = sig
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


def task_desc_default(task_id):
  """The descriptor the library holds for one of the reference's 14 tasks (what the Python Task classes are tested against)."""
  lib = load()
  lib.sag_task_desc_default.argtypes = [C.c_int32, C.POINTER(TaskDesc)]
  t = TaskDesc()
  if lib.sag_task_desc_default(int(task_id), C.byref(t)) != 0:
    raise SagError(f'no task {task_id}')
  return t.to_dict()


def task_desc_check(desc):
  """None, or what the library objects to in a descriptor dict (the field's name and the rule: include/sag.h)."""
  lib = load()
  lib.sag_task_desc_check.argtypes = [C.POINTER(TaskDesc)]
  lib.sag_task_desc_check.restype = C.c_char_p
  msg = lib.sag_task_desc_check(C.byref(TaskDesc.from_dict(desc)))
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


class DeviceArray:
  """A view of device memory owned by a Context (the outputs of a device-resident env.step, BatchedSafeAdaptationGym
  with device_buffers=True): pointer, shape, dtype, strides.  `__cuda_array_interface__` (version 2; HIP pointers are
  what PyTorch-ROCm and CuPy-ROCm expect there) lets a learner wrap it without a copy - torch.as_tensor(a, device='cuda')
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


def device_pointer(x, shape=None, device=None, dtype='<f4'):
  """Device pointer of a DeviceArray or of anything that exports __cuda_array_interface__ (a torch / cupy array on the GPU).
  With `shape`, the array is what a step reads as its actions: float32 ('<f4'), exactly that shape, contiguous and - where
  the array says which device it lives on - on `device`.  Anything else raises ValueError before a kernel can read it
  (a float64 tensor would be read as float32 pairs, a short one past its end).  `dtype`: the element type required
  instead of float32 (uint8 for a reset mask)."""
  if isinstance(x, DeviceArray):
    typestr, xshape, strides, ptr = x.dtype.str, x.shape, x.strides, x.ptr
    where = getattr(x.ctx, 'device', None)
  else:
    cai = getattr(x, '__cuda_array_interface__', None)
    if cai is None:
      raise TypeError(f'{type(x).__name__}: not a device array')
    typestr, xshape, strides, ptr = cai['typestr'], tuple(cai['shape']), cai.get('strides'), int(cai['data'][0])
    dev = getattr(x, 'device', None)   # torch.device (.index) / cupy Device (.id); the interface itself names none
    where = getattr(dev, 'index', getattr(dev, 'id', None))
  if strides is not None and tuple(strides) != tuple(np.zeros(xshape, np.dtype(typestr)).strides):
    raise ValueError('device actions must be contiguous')
  if shape is not None:
    if np.dtype(typestr) != np.dtype(dtype):
      raise ValueError(f'device actions must be float32 (<f4), not {typestr}' if np.dtype(dtype) == np.dtype('<f4') else
                       f'device array must be {np.dtype(dtype).str}, not {typestr}')
    if tuple(xshape) != tuple(shape):
      raise ValueError(f'device actions of shape {tuple(xshape)}: this shard steps {tuple(shape)}')
    if device is not None and isinstance(where, int) and where != device:
      raise ValueError(f'device actions on device {where}: this shard runs on device {device}')
  return ptr


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
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = GaeDesc(int(T), int(pitch), int(capacity), 0, float(gamma), float(lam), float(gamma if cost_gamma is None else cost_gamma),
                float(lam if cost_lam is None else cost_lam), *[ptr(x) for x in (d_reward, d_cost, d_ended, d_value, d_cvalue, d_slot,
                                                                                 d_final_value, d_final_cvalue, d_adv, d_ret, d_cadv, d_cret)])
    self._check(self.lib.sag_gae_device(self.h, C.byref(d)), 'sag_gae_device')

  def policy_forward(self, n_rows, hidden, d_params, d_obs, logp_const=0.0, d_actions=None, d_logp=None, d_value=None, d_cvalue=None,
                     activation=POLICY_RELU, flags=0, draw=0, row0=0, obs_pitch=None):
    """sag_policy_forward_device: the fused actor-critic forward of n_rows observation rows (obs_pitch floats apart; default
    obs_dim) under the parameters at d_params (the header has their layout and the arithmetic), enqueued on the context stream
    - no wait, no host copy.  Pointers are c_void_p, ints or None; an output that is None is not written."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = PolicyDesc(int(n_rows), int(hidden), int(activation), int(flags), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), 0,
                   int(draw) & 0xffffffff, int(row0) & 0xffffffff, float(logp_const),
                   *[ptr(x) for x in (d_params, d_obs, d_actions, d_logp, d_value, d_cvalue)])
    self._check(self.lib.sag_policy_forward_device(self.h, C.byref(d)), 'sag_policy_forward_device')

  def policy_forward_norm(self, n_rows, hidden, d_params, d_obs, d_table, clip=10.0, logp_const=0.0, d_actions=None, d_logp=None,
                          d_value=None, d_cvalue=None, activation=POLICY_RELU, flags=0, draw=0, row0=0, obs_pitch=None):
    """sag_policy_forward_norm_device: policy_forward with every observation element replaced, where its row is staged, by
    clamp((x - mean) * rstd, -clip, clip) under d_table = mean [obs_dim] then rstd [obs_dim] (what obs_stats writes)."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = PolicyDesc(int(n_rows), int(hidden), int(activation), int(flags), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), 0,
                   int(draw) & 0xffffffff, int(row0) & 0xffffffff, float(logp_const),
                   *[ptr(x) for x in (d_params, d_obs, d_actions, d_logp, d_value, d_cvalue)])
    self._check(self.lib.sag_policy_forward_norm_device(self.h, C.byref(d), ptr(d_table), float(clip)), 'sag_policy_forward_norm_device')

  def policy_backward(self, n_rows, n_planes, pitch, hidden, d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_grad, scale,
                      d_cadv=None, d_cret=None, clip=0.2, vf_coef=0.5, cvf_coef=0.5, ent_coef=0.0, adv_affine=(1.0, 0.0),
                      cadv_affine=(0.0, 0.0), activation=POLICY_RELU, flags=0, max_blocks=0, obs_pitch=None, rows=None):
    """sag_policy_backward_device: the PPO-Lagrangian gradient and 8 statistics of n_planes x n_rows stored rows (planes `pitch`
    rows apart) into d_grad [n_params + 8], enqueued on the context stream - no wait, no host copy.  The header defines the
    function; adv_affine = (adv_mul, adv_sub), cadv_affine likewise.  Pointers are c_void_p, ints or None.
    rows=(d_rows, n_index): sag_policy_backward_rows_device - the batch is the n_index logical elements that the device int32
    list at d_rows names, gathered in place."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = PolicyGradDesc(int(n_rows), int(n_planes), int(pitch), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), int(hidden),
                       int(activation), int(flags), int(max_blocks), float(clip), float(vf_coef), float(cvf_coef), float(ent_coef),
                       float(adv_affine[0]), float(adv_affine[1]), float(cadv_affine[0]), float(cadv_affine[1]), float(scale), 0.0,
                       *[ptr(x) for x in (d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_cadv, d_cret, d_grad)])
    if rows is not None:
      self._check(self.lib.sag_policy_backward_rows_device(self.h, C.byref(d), ptr(rows[0]), int(rows[1]), None, 0.0),
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
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = PolicyGradDesc(int(n_rows), int(n_planes), int(pitch), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), int(hidden),
                       int(activation), int(flags), int(max_blocks), float(clip), float(vf_coef), float(cvf_coef), float(ent_coef),
                       float(adv_affine[0]), float(adv_affine[1]), float(cadv_affine[0]), float(cadv_affine[1]), float(scale), 0.0,
                       *[ptr(x) for x in (d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret, d_cadv, d_cret, d_grad)])
    if rows is not None:
      self._check(self.lib.sag_policy_backward_rows_device(self.h, C.byref(d), ptr(rows[0]), int(rows[1]), ptr(d_table), float(obs_clip)),
                  'sag_policy_backward_rows_device')
      return
    self._check(self.lib.sag_policy_backward_norm_device(self.h, C.byref(d), ptr(d_table), float(obs_clip)), 'sag_policy_backward_norm_device')

  def permutation(self, n, draw, d_index):
    """sag_permutation_device: d_index[0 ... n) (device int32) = a keyed pseudo-random permutation of 0 ... n - 1 under the
    context key and `draw` (the header defines it bit for bit); enqueued on the context stream - no wait, no host copy."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    self._check(self.lib.sag_permutation_device(self.h, int(n), int(draw) & 0xffffffff, ptr(d_index)), 'sag_permutation_device')

  def obs_stats(self, d_state, d_table, d_obs=None, n_rows=0, n_planes=0, pitch=0, obs_pitch=None, eps=1e-8, max_blocks=0, table_only=False):
    """sag_obs_stats_device: the per-column moments of n_planes x n_rows observation rows (planes `pitch` rows, rows obs_pitch
    floats apart) merged into d_state = {count, mean [obs_dim], M2 [obs_dim]} float64, and d_table = mean, rstd float32 made from
    it; table_only=True rewrites the table from the state and reads no observations.  Enqueued on the context stream."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = ObsStatsDesc(int(n_rows), int(n_planes), int(pitch), int(self.info['obs_dim'] if obs_pitch is None else obs_pitch), int(max_blocks),
                     OBS_STATS_TABLE_ONLY if table_only else 0, float(eps), 0.0, ptr(d_obs), ptr(d_state), ptr(d_table))
    self._check(self.lib.sag_obs_stats_device(self.h, C.byref(d)), 'sag_obs_stats_device')

  def adam(self, n, d_param, d_grad, d_m, d_v, step, beta1=0.9, beta2=0.999, eps=1e-8, clamp_first=None, clamp_lo=0.0):
    """sag_adam_device: one Adam step on n float32 elements (the header has the chain; `step` is the bias-corrected learning
    rate), elements from clamp_first on kept at or above clamp_lo; enqueued on the context stream."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = AdamDesc(int(n), int(n if clamp_first is None else clamp_first), float(beta1), float(beta2), float(eps), float(step),
                 float(clamp_lo), 0.0, *[ptr(x) for x in (d_param, d_grad, d_m, d_v)])
    self._check(self.lib.sag_adam_device(self.h, C.byref(d)), 'sag_adam_device')

  def moments(self, n_rows, n_planes, pitch, d_x, d_out, d_mask=None, stride=1, eps=1e-8, max_blocks=0):
    """sag_moments_device: d_out[4] = {count, mean, var, 1 / (sqrt(var) + eps)} of the n_planes x n_rows elements of d_x (planes
    `pitch` rows apart, elements `stride` floats apart) whose byte of d_mask [n_planes][pitch] is non-zero (None: all); enqueued
    on the context stream, the result stays on the device."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = MomentsDesc(int(n_rows), int(n_planes), int(pitch), int(stride), int(max_blocks), 0, float(eps), 0.0, ptr(d_x), ptr(d_mask), ptr(d_out))
    self._check(self.lib.sag_moments_device(self.h, C.byref(d)), 'sag_moments_device')

  def advantage_mix(self, n_rows, n_planes, pitch, d_adv, d_out, d_cadv=None, adv_mode=ADV_RAW, cadv_mode=ADV_RAW, d_adv_mom=None,
                    d_cadv_mom=None, d_lambda=None, cost_weight=0.0):
    """sag_advantage_mix_device: d_out = norm(adv) - lambda * norm(cadv) elementwise (the header has the chain), the moments
    arrays as moments() writes them, lambda = d_lambda[0] or cost_weight; enqueued on the context stream."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = AdvantageMixDesc(int(n_rows), int(n_planes), int(pitch), 0, int(adv_mode), int(cadv_mode), float(cost_weight), 0.0,
                         *[ptr(x) for x in (d_adv, d_cadv, d_adv_mom, d_cadv_mom, d_lambda, d_out)])
    self._check(self.lib.sag_advantage_mix_device(self.h, C.byref(d)), 'sag_advantage_mix_device')

  def lagrange(self, d_mom, d_state, lr, budget, lambda_max=float('inf')):
    """sag_lagrange_device: d_state[4] = {lambda, mean cost, episodes, updates} takes one step lambda += lr * (mean - budget),
    kept in [0, lambda_max], from the moments at d_mom (no step where their count is 0); enqueued on the context stream."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = LagrangeDesc(float(lr), float(budget), float(lambda_max), 0.0, ptr(d_mom), ptr(d_state))
    self._check(self.lib.sag_lagrange_device(self.h, C.byref(d)), 'sag_lagrange_device')

  def grad_clip(self, n, d_grad, d_out, max_norm, max_blocks=0):
    """sag_grad_clip_device: d_grad[0 ... n) scaled in place by min(1, max_norm / (norm + 1e-6)), d_out[2] = {norm, factor};
    enqueued on the context stream."""
    ptr = lambda x: x.value if isinstance(x, C.c_void_p) else x   # noqa: E731
    d = GradClipDesc(int(n), int(max_blocks), float(max_norm), 0.0, ptr(d_grad), ptr(d_out))
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
