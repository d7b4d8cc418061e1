// sag_api.hip - host side of the C ABI declared in include/sag.h.
//
// One context = one GPU = one HIP stream.  Device memory: the SoA world
// (S: [DEV_GROUPS][N] float4, I: tstate [N] + int4 [N]; sag_device.hpp didx / iaddr), AoS staging for records,
// pinned host + device staging for the host-pointer step.  No allocation, no
// synchronisation and no host<->device copy happens inside sag_step_device()
// (every buffer it needs exists after sag_create; timing events, off by default,
// are the exception), so callers may capture it into a hipGraph.  Every entry point
// selects the context's device first: contexts on different GPUs may share a host thread.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "sag_device.hpp"
#include "sag_reset.hpp"
#include "sag_rollout.hpp"
#include "sag_fork.hpp"
#include "sag_plan.hpp"
#include "sag_buffer.hpp"
#include "sag_policy.hpp"
#include "sag_policy_grad.hpp"
#include "sag_learner.hpp"
#include "sag_obs_norm.hpp"
#include "sag_shuffle.hpp"

#ifndef SAG_SPLIT_MIN_ENVS
#define SAG_EARLY_FORK_MIN_ENVS 2097152  // tools/ab.sh run sweep: crossover between 1.5 M and 2 M envs
#define SAG_SPLIT_MIN_ENVS 262144  // measured crossover (tools/split_sweep.py, overlapped launches): Point ~260k, Car ~390k
#define SAG_SPLIT_MIN_ENVS_CAR 393216
#endif

using namespace sag;

namespace {

struct RobotInfo { int nu, obs_dim, nstep, nq, nv; double dt; };
const RobotInfo ROBOTS[3] = {
    {2, 60, 5, 3, 3, 0.004},      // point.xml:3, safe_adaptation_gym.py:15-19
    {2, 72, 10, 13, 11, 0.008},   // car.xml:3
    {12, 104, 12, 20, 19, 0.012}  // doggo.xml:2
};

thread_local std::string g_create_error;

}  // namespace

struct sag_ctx {
  sag_config cfg;
  RobotInfo rb;
  int N;
  hipStream_t stream = nullptr;
  // split form: the busy kernel (few, long, VALU-bound wavefronts) runs on a second stream beside
  // the quiet kernel (many short memory-bound ones); fork/join events order them against the main stream
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int early_fork = -1;  // quiet stream forks before the compaction: 1 / 0, -1 = by batch size (SAG_EARLY_FORK)
  float* S = nullptr;
  int32_t* I = nullptr;
  float* G = nullptr;  // [3][NBODY][N] spill of body accelerations beyond the LDS pool
  // busy lists (split launches), rebuilt by k_compact from the busy bits before every busy launch:
  // rows [BUSY_CLASSES][N]; d_count holds two sets of BUSY_CLASSES counters, used alternately (a
  // compaction fills one and zeroes the other for the next step), then the env count of the last busy launch
  int32_t* d_rows = nullptr; int32_t* d_count = nullptr;
  uint8_t* d_kind = nullptr;   // [N] kind of every busy env (BUSY_CLASSES)
  int count_flip = 0;          // which counter set of d_count this step's compaction fills
  int32_t* last_count = nullptr;
  float* d_hot = nullptr;     // [N][HOT_FLOATS] hot records (split form), see sag_device.hpp
  bool hot_valid = false;
  // last installed layout (sag_reset)
  float* L_f = nullptr;   // [N][SAG_REC_FLOATS] AoS, device
  int32_t* L_i = nullptr; // [N][SAG_REC_INTS]
  // staging
  float* st_f = nullptr; int32_t* st_i = nullptr; int32_t* st_ids = nullptr;  // device, N records
  void* pin = nullptr; size_t pin_bytes = 0;  // pinned host
  // step staging (device)
  float* d_act = nullptr; float* d_noise = nullptr; uint32_t* d_tape = nullptr; size_t tape_cap = 0;
  float* d_obs = nullptr; float* d_rew = nullptr; uint8_t* d_cost = nullptr; uint8_t* d_done = nullptr;
  uint8_t* d_met = nullptr; int32_t* d_used = nullptr;
  int32_t* d_ext_cc = nullptr; uint32_t* d_ext_btn = nullptr; bool ext_pending = false;   // sag_set_ext_contacts
  // generic buffers for sag_lidar_cost
  void* scratch = nullptr; size_t scratch_bytes = 0;
  bool have_layout = false;
  // kernel timing
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  double ev_ms = 0; int64_t ev_n = 0;
  bool timing = false;
  int phase = 0;       // busy-bit copy read by the next step launch
  int phase_used = 0;  // (the phase of the launch being built)
  int n_cu = 256;      // compute units of the device
  uint8_t* d_rgb = nullptr; size_t rgb_bytes = 0;  // [N][H][W][3] staging of sag_render, grown on demand
  double* d_dr = nullptr;    // Doggo: per-env result block of the physics kernel (k_doggo_physics: 2 envs per wavefront)
  int32_t* d_dg_sched = nullptr; int dg_phase = 0;   // Doggo: longest-first launch order (sag_doggo_coop.hpp); SAG_DOGGO_SCHED=0 turns it off
  bool dg_sched_on = true;
  int busy_kinds = -1;   // SAG_BUSY_KINDS: 1 = the busy list by kind of contact, 0 = one list; default: the Car (the Point's step is its quiet kernel: no gain)
  int kinds_min = -1;    // SAG_BUSY_KINDS_MIN: busy envs of the step before above which the kinds are used (default: 64 per resident slot; tests: 0)
  bool split = true;   // QUIET + BUSY launches; SAG_SPLIT=0/1 in the environment forces the form
  // device reset (sag_set_tasks / sag_reset_device): descriptor table, descriptor of every env, world config
  sag_task_desc* d_descs = nullptr; int n_descs = 0;
  int32_t* d_desc_of_env = nullptr;
  sag_world_config rcfg{};
  int32_t env_id0 = 0;
  bool have_tasks = false;
  int32_t* d_rstat = nullptr;   // [N] status by env, then 2 counters (listed envs, failures)
  float* d_rbound = nullptr;    // [N]
  unsigned long long* d_rtot = nullptr;   // sag_reset_device_async: envs reset, envs whose sampling failed (sag_reset_device_counts)
  float* d_acc = nullptr;       // [N] float4 episode accumulators (sag_episode_track_device), allocated on first use
  // sag_fork_device: the descriptor table as given to sag_set_tasks (two contexts fork only under the same table), the
  // counters (envs copied, envs rejected) and the events that order a fork between two contexts' streams
  std::vector<sag_task_desc> h_descs;
  unsigned long long* d_ftot = nullptr;
  hipEvent_t ev_xsrc = nullptr, ev_xdone = nullptr;
  // sag_plan_*: alive flags of a scoring rollout and the ranks of a refit ([N] each), the second buffer of sag_plan_shift_device
  uint8_t* d_palive = nullptr; int32_t* d_prank = nullptr;
  float* d_pshift = nullptr; size_t pshift_floats = 0;
  // sag_policy_backward_device: one partial gradient per block
  float* d_pgrad = nullptr; size_t pgrad_floats = 0;
  // sag_moments_device, sag_grad_clip_device: one (sum, count) partial per block
  float* d_lpart = nullptr; size_t lpart_blocks = 0;
  // sag_obs_stats_device: the batch means (f64, f32), then one [obs_dim] partial per block; allocated on first use for the largest grid
  void* d_obsn = nullptr;
  std::string err;
};

namespace {

int fail(sag_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf; else g_create_error = buf;
  return code;
}

#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, SAG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                 \
  } while (0)

int ensure_pin(sag_ctx* c, size_t bytes) {
  if (c->pin_bytes >= bytes) return 0;
  if (c->pin) (void)hipHostFree(c->pin);
  c->pin = nullptr; c->pin_bytes = 0;
  HIPCHK(c, hipHostMalloc(&c->pin, bytes, hipHostMallocDefault));
  c->pin_bytes = bytes;
  return 0;
}

int ensure_scratch(sag_ctx* c, size_t bytes) {
  if (c->scratch_bytes >= bytes) return 0;
  if (c->scratch) (void)hipFree(c->scratch);
  c->scratch = nullptr; c->scratch_bytes = 0;
  HIPCHK(c, hipMalloc(&c->scratch, bytes));
  c->scratch_bytes = bytes;
  return 0;
}

// ---- Doggo model tables (doggo.xml), built in fp64 and copied to constant memory ----
// Geometry numbers are the XML's: body offsets (:18-79), joint axes / ranges / springref (:21-71),
// geoms as (from, to, radius, density) with capsules unless noted (:5-6,15,48), touch sites (:27-28 ...).
void dg_build_model(DgModel& M) {
  static const int parent[DG_NB] = {-1, 0, 1, 0, 3, 0, 5, 6, 5, 8};
  static const double bpos[DG_NB][3] = {{0, 0, 0}, {.2, .1, 0}, {.098, .0566, -.05}, {.2, -.1, 0}, {.098, -.0566, -.05},
                                        {0, 0, 0}, {-.2, .1, 0}, {.098, .0566, -.05}, {-.2, -.1, 0}, {.098, -.0566, -.05}};
  static const int dof_body[DG_NV] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 3, 3, 4, 5, 6, 6, 7, 8, 8, 9};
  static const double axis[DG_NJ][3] = {{0, 0, 1}, {0, 1, 0}, {-.5, .866, 0}, {0, 0, -1}, {0, 1, 0}, {.5, .866, 0}, {1, 0, 0},
                                        {0, 0, 1}, {0, 1, 0}, {-.5, .866, 0}, {0, 0, -1}, {0, 1, 0}, {.5, .866, 0}};
  static const double range_deg[DG_NJ][2] = {{-10, 30}, {-75, 15}, {-75, 0}, {-10, 30}, {-75, 15}, {-75, 0}, {-30, 30},
                                             {-10, 30}, {0, 135}, {-75, 0}, {-10, 30}, {0, 135}, {-75, 0}};
  static const double springref_deg[DG_NJ] = {0, -10, -20, 0, -10, -20, 0, 0, 0, -20, 0, 0, -20};
  static const int act_joint[12] = {0, 7, 10, 3, 1, 8, 11, 4, 2, 9, 12, 5};
  struct G { int body; double a[3], b[3], r, dens; bool capsule; };
  static const G geoms[14] = {
      {0, {0, 0, 0}, {.2, 0, 0}, .075, .5, false}, {0, {.1, 0, 0}, {.2, .1, 0}, .032, 5, true},
      {0, {.1, 0, 0}, {.2, -.1, 0}, .032, 5, true}, {1, {0, 0, 0}, {.098, .0566, -.05}, .032, 5, true},
      {2, {0, 0, 0}, {-.1176, -.0679, -.1}, .032, 5, true}, {3, {0, 0, 0}, {.098, -.0566, -.05}, .032, 5, true},
      {4, {0, 0, 0}, {-.1176, .0679, -.1}, .032, 5, true}, {5, {-.2, 0, 0}, {0, 0, 0}, .075, .5, false},
      {5, {-.1, 0, 0}, {-.2, .1, 0}, .032, 5, true}, {5, {-.1, 0, 0}, {-.2, -.1, 0}, .032, 5, true},
      {6, {0, 0, 0}, {.098, .0566, -.05}, .032, 5, true}, {7, {0, 0, 0}, {-.1176, -.0679, -.1}, .032, 5, true},
      {8, {0, 0, 0}, {.098, -.0566, -.05}, .032, 5, true}, {9, {0, 0, 0}, {-.1176, .0679, -.1}, .032, 5, true}};
  // floor contact points (oracle DG_FLOORPTS): geom, end, rim, merged, touch slot, half share
  struct Fp { int geom, end, rim, dbl, touch, half; };
  static const Fp floorpts[DG_NFP] = {
      {0, 1, 1, 0, -1, 0}, {0, 0, 1, 0, -1, 0},
      {3, 0, 0, 1, -1, 0}, {4, 0, 0, 1, 0, 1}, {4, 1, 0, 0, 4, 0},
      {5, 0, 0, 1, -1, 0}, {6, 0, 0, 1, 3, 1}, {6, 1, 0, 0, 7, 0},
      {7, 1, 1, 0, -1, 0}, {7, 0, 1, 0, -1, 0},
      {10, 0, 0, 1, -1, 0}, {11, 0, 0, 1, 1, 1}, {11, 1, 0, 0, 5, 0},
      {12, 0, 0, 1, -1, 0}, {13, 0, 0, 1, 2, 1}, {13, 1, 0, 0, 6, 0}};
  static const int geom_touch[14] = {-1, -1, -1, -1, 0, -1, 3, -1, -1, -1, -1, 1, -1, 2};
  const double pi = 3.14159265358979323846;
  memset(&M, 0, sizeof(M));
  for (int b = 0; b < DG_NB; b++) {
    M.parent[b] = parent[b];
    for (int k = 0; k < 3; k++) M.bpos[b][k] = bpos[b][k];
    unsigned anc = 0;
    for (int a = b; a >= 0; a = parent[a]) anc |= 1u << a;
    M.anc[b] = anc;
  }
  for (int i = 0; i < DG_NV; i++) M.dof_body[i] = dof_body[i];
  for (int j = 0; j < DG_NJ; j++) {
    const double n = std::sqrt(axis[j][0] * axis[j][0] + axis[j][1] * axis[j][1] + axis[j][2] * axis[j][2]);
    for (int k = 0; k < 3; k++) M.axis[j][k] = axis[j][k] / n;
    M.lo[j] = range_deg[j][0] * pi / 180; M.hi[j] = range_deg[j][1] * pi / 180;
    M.springref[j] = springref_deg[j] * pi / 180;
  }
  for (int k = 0; k < 12; k++) M.act_joint[k] = act_joint[k];
  double gm[14], gc[14][3], gI[14][9];
  for (int g = 0; g < 14; g++) {
    const G& q = geoms[g];
    const double d[3] = {q.b[0] - q.a[0], q.b[1] - q.a[1], q.b[2] - q.a[2]};
    const double L = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), r = q.r;
    const double u[3] = {d[0] / L, d[1] / L, d[2] / L};
    const double mc = q.dens * pi * r * r * L, ms = q.capsule ? q.dens * 4.0 / 3.0 * pi * r * r * r : 0.0;
    const double Ia = mc * r * r / 2 + ms * 2 * r * r / 5;
    const double It = mc * (r * r / 4 + L * L / 12) + ms * (2 * r * r / 5 + L * L / 4 + 3 * L * r / 8);
    gm[g] = mc + ms;
    for (int k = 0; k < 3; k++) gc[g][k] = 0.5 * (q.a[k] + q.b[k]);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) gI[g][3 * a + b] = It * ((a == b ? 1.0 : 0.0) - u[a] * u[b]) + Ia * u[a] * u[b];
    M.m[q.body] += gm[g];
    for (int k = 0; k < 3; k++) M.com[q.body][k] += gm[g] * gc[g][k];
  }
  for (int b = 0; b < DG_NB; b++)
    for (int k = 0; k < 3; k++) M.com[b][k] /= M.m[b];
  for (int g = 0; g < 14; g++) {
    const int b = geoms[g].body;
    const double d[3] = {gc[g][0] - M.com[b][0], gc[g][1] - M.com[b][1], gc[g][2] - M.com[b][2]};
    const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    for (int a = 0; a < 3; a++)
      for (int c = 0; c < 3; c++) M.I[b][3 * a + c] += gI[g][3 * a + c] + gm[g] * ((a == c ? d2 : 0.0) - d[a] * d[c]);
  }
  for (int s = 0; s < DG_NFP; s++) {
    const Fp& f = floorpts[s];
    M.fp_code[s] = f.geom | f.end << 4 | f.rim << 5 | f.dbl << 6 | (f.touch + 1) << 7 | f.half << 11;
  }
  static_assert(DG_NGEOM == 14, "geom table");
  for (int g = 0; g < DG_NGEOM; g++) {
    M.geom_body[g] = geoms[g].body; M.geom_capsule[g] = geoms[g].capsule ? 1 : 0; M.geom_r[g] = geoms[g].r;
    M.geom_touch[g] = geom_touch[g];
    // ankle geoms = the shin capsules on bodies 2, 4 (front legs: blue) and 7, 9 (rear legs: green)
    M.geom_ankle[g] = (geoms[g].body == 2 || geoms[g].body == 4) ? 1 : ((geoms[g].body == 7 || geoms[g].body == 9) ? 2 : 0);
    for (int k = 0; k < 3; k++) { M.geom_a[g][k] = geoms[g].a[k]; M.geom_b[g][k] = geoms[g].b[k]; }
  }
}

// drain finished timing events into the running mean
void drain_events(sag_ctx* c) {
  for (size_t k = 0; k < c->ev_used; k++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev_pool[k].first, c->ev_pool[k].second) == hipSuccess) {
      c->ev_ms += ms; c->ev_n += 1;
    }
  }
  c->ev_used = 0;
}

// a pair of timing events for one launch (nullptr, nullptr when timing is off); bounded pool
int timing_events(sag_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->timing) return 0;
  if (c->ev_used == c->ev_pool.size()) {
    if (c->ev_pool.size() >= 4096) {  // fold what has finished
      HIPCHK(c, hipStreamSynchronize(c->stream));
      drain_events(c);
    } else {
      hipEvent_t a0, a1;
      HIPCHK(c, hipEventCreate(&a0));
      HIPCHK(c, hipEventCreate(&a1));
      c->ev_pool.emplace_back(a0, a1);
    }
  }
  *e0 = c->ev_pool[c->ev_used].first; *e1 = c->ev_pool[c->ev_used].second;
  c->ev_used++;
  return 0;
}

int launch_step(sag_ctx* c, const float* d_act, const float* d_noise, const uint32_t* d_tape,
                int tape_len, int nstep, float* d_obs, float* d_rew, uint8_t* d_cost,
                uint8_t* d_done, uint8_t* d_met, int32_t* d_used, int observe_only) {
  HIPCHK(c, hipSetDevice(c->cfg.device));
  StepArgs a;
  a.S = c->S; a.I = c->I; a.N = c->N;
  a.actions = d_act; a.noise = d_noise; a.tape = d_tape; a.tape_len = tape_len;
  a.nstep = nstep < 0 ? c->rb.nstep : nstep;
  a.nstep_table = c->rb.nstep;
  a.h = (float)c->rb.dt;
  a.car = car_fric_constants(a.h);
  a.key0 = (uint32_t)(c->cfg.seed & 0xffffffffu); a.key1 = (uint32_t)(c->cfg.seed >> 32);  // sag_set_seed
  a.obs = d_obs; a.reward = d_rew; a.cost = d_cost; a.done = d_done; a.goal_met = d_met;
  a.tape_used = d_used; a.max_vases = c->cfg.max_vases; a.max_hazards = c->cfg.max_hazards;
  a.max_pillars = c->cfg.max_pillars; a.max_buttons = c->cfg.max_buttons; a.observe_only = observe_only;
  a.has_box = c->cfg.has_box; a.G = c->G;
  a.phase = c->phase; a.rows = c->d_rows; a.count = nullptr;   // (the busy list: split form, below)
  a.DR = nullptr; a.dg_sched = nullptr; a.dg_phase = -1;
  a.hot = nullptr; a.hot_haz = nullptr;
  // external contact results: for the one step with nstep == 0 that follows sag_set_ext_contacts
  const bool use_ext = c->ext_pending && !observe_only && a.nstep == 0;
  a.ext_cc = use_ext ? c->d_ext_cc : nullptr; a.ext_btn = use_ext ? c->d_ext_btn : nullptr;
  if (!observe_only) c->ext_pending = false;
  {
    // single-launch form: aim for four wavefronts per CU (Doggo: one - only one fits its LDS working
    // set), down to 16 (Doggo 8) envs per wavefront (measured by a sweep of envs per wavefront: Car 4096 envs 0.58 -> 0.48 ms)
    const bool dg = c->cfg.robot == SAG_ROBOT_DOGGO;
    int epw = 64;
    while (epw > (dg ? 8 : 16) && (c->N + epw - 1) / epw < (dg ? 1 : 4) * c->n_cu) epw >>= 1;
    a.envs_per_wave = epw;
    a.busy_kinds = c->busy_kinds < 0 ? c->cfg.robot == SAG_ROBOT_CAR : c->busy_kinds; a.kind = a.busy_kinds ? c->d_kind : nullptr; a.busy_total = c->d_count + 2 * BUSY_CLASSES;
    a.busy_slots = 8 * c->n_cu;   // two busy wavefronts per SIMD
  }
  c->phase_used = c->phase;
  if (!observe_only) c->phase ^= 1;
  const int blocks = (c->N + WAVE - 1) / WAVE;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!observe_only) {
    int rc = timing_events(c, &e0, &e1);
    if (rc) return rc;
    if (e0) HIPCHK(c, hipEventRecord(e0, c->stream));
  }
  const bool btn = c->cfg.max_buttons > 0, tbox = c->cfg.has_box != 0;
  // split form: QUIET kernel over every env whose busy bit is clear, then BUSY kernel over the
  // rest (compacted per 256-env neighbourhood).  observe() and SAG_SPLIT=0 use the single form.
  const bool split = c->split && !observe_only && c->cfg.robot != SAG_ROBOT_DOGGO;
  hipStream_t quiet_stream = c->stream;
  if (split) {
    a.hot = c->d_hot; a.hot_haz = c->d_hot + (size_t)c->N * HOT_FLOATS;
    if (!c->hot_valid) {
      hipLaunchKernelGGL(k_hot_refresh, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N, c->d_hot, c->d_hot + (size_t)c->N * HOT_FLOATS);
      c->hot_valid = true;
    }
    // The quiet kernel needs no list (it reads the busy bits), so its stream forks off BEFORE the
    // compaction: k_compact only looks at this step's copy of the bit, which the quiet kernel never
    // changes (it rewrites tstate words of quiet envs with that bit still clear), so the two may overlap.
    // Only when the batch is large enough to keep the chip full (>= SAG_EARLY_FORK_MIN_ENVS): below that a
    // step is as long as its busy wavefronts, which must then be resident first (1 M envs: 15 % slower
    // with the early fork, 4 M envs: 10 % faster; profiles/r01_v16_early_fork_ab.txt).
    const bool early_fork = c->early_fork < 0 ? (c->N >= SAG_EARLY_FORK_MIN_ENVS && c->cfg.robot != SAG_ROBOT_CAR) : c->early_fork != 0;
    // (Car: its busy kernel is 4x longer than the quiet one and sets the step; with the early fork the quiet grid
    // occupies the chip first and the busy wavefronts start late: 3.49 vs 3.15 ms at 4 M envs)
    if (early_fork) {
      HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
      quiet_stream = c->stream2;
    }
    // two counter sets used alternately: this step's compaction zeroes the one the next step will use
    a.count = c->d_count + c->count_flip * BUSY_CLASSES;
    int32_t* const zero_for_next = c->d_count + (c->count_flip ^ 1) * BUSY_CLASSES;
    if (a.busy_kinds)
      hipLaunchKernelGGL(k_compact<true>, dim3((c->N + COMPACT_ENVS - 1) / COMPACT_ENVS), dim3(256), 0, c->stream, c->I, c->d_kind, c->N, a.phase,
                         a.rows, a.count, zero_for_next, a.busy_total, c->kinds_min >= 0 ? c->kinds_min : 64 * a.busy_slots);
    else
      hipLaunchKernelGGL(k_compact<false>, dim3((c->N + COMPACT_ENVS - 1) / COMPACT_ENVS), dim3(256), 0, c->stream, c->I, c->d_kind, c->N, a.phase,
                         a.rows, a.count, zero_for_next, a.busy_total, 0);
    c->count_flip ^= 1;
    c->last_count = a.count;
    if (!early_fork) {
      HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
      quiet_stream = c->stream2;
    }
  }
  // Side by side with the busy kernel the quiet kernel requests unused LDS on top of its own 10 KB: a quiet
  // wavefront then frees at least what a busy one needs (13 KB), so a waiting busy workgroup (higher stream
  // priority) fits into any hole a quiet one leaves.  With 10-KB holes the busy kernel, which sets the length of
  // a step, is starved of LDS by the far more numerous quiet workgroups once the batch exceeds what is resident
  // at once (measured at 4 M envs: +8 % throughput, tools/ab.sh run).
  size_t quiet_lds_extra = 0;
  if (split) {
    // (the static array differs between the instances of a robot - quiet_lds_rows -, the sum does not)
    const int quiet_own = quiet_lds_rows(c->cfg.robot, btn, tbox) * WAVE * (int)sizeof(float);
    quiet_lds_extra = (size_t)(quiet_lds_total(c->cfg.robot) - quiet_own);
  }
#define SAG_LAUNCH3(ROB, B_, X_)                                                                         \
  do {                                                                                                  \
    if (split) {                                                                                        \
      hipLaunchKernelGGL((k_step_busy<ROB, B_, X_>), dim3(busy_grid(c->N)), dim3(WAVE), 0, c->stream, a); \
      hipLaunchKernelGGL((k_step_quiet<ROB, B_, X_>), dim3(blocks), dim3(WAVE), quiet_lds_extra, quiet_stream, a); \
    } else {                                                                                            \
      hipLaunchKernelGGL((k_step<ROB, B_, X_>), dim3((c->N + a.envs_per_wave - 1) / a.envs_per_wave), dim3(WAVE), 0, c->stream, a); \
    }                                                                                                   \
  } while (0)
#define SAG_LAUNCH(ROB)                            \
  do {                                             \
    if (!btn && !tbox) SAG_LAUNCH3(ROB, false, false); \
    else if (btn && !tbox) SAG_LAUNCH3(ROB, true, false); \
    else if (!btn && tbox) SAG_LAUNCH3(ROB, false, true); \
    else SAG_LAUNCH3(ROB, true, true);             \
  } while (0)
  // (-DSAG_ONLY_ROBOT=<id>: kernel-tuning builds that instantiate one robot's step kernels only - a third of the
  // compile time; the shipped library has them all)
#ifndef SAG_ONLY_ROBOT
#define SAG_ONLY_ROBOT -1
#endif
  if (false) {}
#if SAG_ONLY_ROBOT < 0 || SAG_ONLY_ROBOT == 0
  else if (c->cfg.robot == SAG_ROBOT_POINT) SAG_LAUNCH(SAG_ROBOT_POINT);
#endif
#if SAG_ONLY_ROBOT < 0 || SAG_ONLY_ROBOT == 1
  else if (c->cfg.robot == SAG_ROBOT_CAR) SAG_LAUNCH(SAG_ROBOT_CAR);
#endif
  else if (c->cfg.robot != SAG_ROBOT_DOGGO) return fail(c, SAG_ERR_UNSUPPORTED, "this build holds the step kernels of robot %d only", SAG_ONLY_ROBOT);
  else {
    // Doggo: wave-cooperative physics (32 lanes per env) + the generic step without physics
    a.DR = c->d_dr;
    const bool sched = c->dg_sched_on && c->d_dg_sched && !observe_only;
    a.dg_sched = sched ? c->d_dg_sched : nullptr;
    a.dg_phase = sched ? c->dg_phase : -1;
    if (sched) c->dg_phase = (c->dg_phase + 1) % 6;   // (the kernel uses it mod 2 and mod 3)
    hipLaunchKernelGGL(k_doggo_physics, dim3(sched ? dc_sched_blocks(c->N) : (c->N + DC_EPW - 1) / DC_EPW), dim3(32 * DC_EPW), 0, c->stream, a, c->d_dr);
    hipLaunchKernelGGL((k_step_doggo_post<true, true>), dim3(blocks), dim3(WAVE), 0, c->stream, a);
  }
#undef SAG_LAUNCH
#undef SAG_LAUNCH3
  if (split) {
    HIPCHK(c, hipEventRecord(c->ev_join, c->stream2));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
  }
  if (e1) HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipGetLastError());
  return 0;
}

// A team of lanes per pose (k_lidar_cost_team): lane s of a team takes the points s, s + LPP, ...  Few poses (the reference's own
// 4096): 16 lanes, so that the chip is full and a pose's points are not one serial chain; more poses, smaller teams - 8 up to 262 144
// poses, 4 beyond (4 M poses x 21 points, kernel only: teams of 4 0.474 ms, of 8 0.502, of 2 0.641, of 16 0.684; the lane-per-pose
// kernel with its points in registers 0.537, LDS-staged 0.792 - its 12.8 KB of staging / tile per wavefront hold it at three
// wavefronts per SIMD, a team's 3-KB tile does not; profiles/r04_lidar_forms.txt).  SAG_LIDAR_TEAM = 0 / 2 / 4 / 8 / 16 forces the
// form (0: a lane per pose - K <= 21 the register-resident kernel, more points per env or SAG_LIDAR_REG=0 the LDS-staged one;
// the tests run every form on the same inputs).
void launch_lidar_cost(sag_ctx* c, int n, int K, const float* d_robot, const float* d_pts, const uint8_t* d_grp, float hazard_size,
                       float* d_lid, int32_t* d_bins, uint8_t* d_cost) {
  static const bool use_reg = [] { const char* e = getenv("SAG_LIDAR_REG"); return !e || atoi(e) != 0; }();
  int team = n <= 16384 ? 16 : (n <= 262144 ? 8 : 4);
  if (const char* e = getenv("SAG_LIDAR_TEAM")) team = atoi(e);
  if (team == 2)
    hipLaunchKernelGGL(k_lidar_cost_team<2>, dim3((n + 31) / 32), dim3(WAVE), 0, c->stream, n, K, d_robot, d_pts, d_grp, hazard_size,
                       d_lid, d_bins, d_cost);
  else if (team == 8)
    hipLaunchKernelGGL(k_lidar_cost_team<8>, dim3((n + 7) / 8), dim3(WAVE), 0, c->stream, n, K, d_robot, d_pts, d_grp, hazard_size,
                       d_lid, d_bins, d_cost);
  else if (team >= 16)
    hipLaunchKernelGGL(k_lidar_cost_team<16>, dim3((n + 3) / 4), dim3(WAVE), 0, c->stream, n, K, d_robot, d_pts, d_grp, hazard_size,
                       d_lid, d_bins, d_cost);
  else if (team >= 4)
    hipLaunchKernelGGL(k_lidar_cost_team<4>, dim3((n + 15) / 16), dim3(WAVE), 0, c->stream, n, K, d_robot, d_pts, d_grp, hazard_size,
                       d_lid, d_bins, d_cost);
  else if (K <= LC_KREG && use_reg)
    hipLaunchKernelGGL(k_lidar_cost_reg, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, c->stream, n, K, d_robot, d_pts, d_grp,
                       hazard_size, d_lid, d_bins, d_cost);
  else
    hipLaunchKernelGGL(k_lidar_cost, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), lidar_cost_lds_bytes(K), c->stream, n, K, d_robot, d_pts,
                       d_grp, hazard_size, d_lid, d_bins, d_cost);
}

}  // namespace

extern "C" {

int sag_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sag_robot_info(int32_t robot, int32_t out[5], double* dt) {
  if (robot < 0 || robot > 2 || !out || !dt) return SAG_ERR_ARG;
  const RobotInfo& r = ROBOTS[robot];
  out[0] = r.nu; out[1] = r.obs_dim; out[2] = r.nstep; out[3] = r.nq; out[4] = r.nv;
  *dt = r.dt;
  return SAG_OK;
}

const char* sag_last_error(const sag_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sag_create(const sag_config* cfg, sag_ctx** out) {
  if (!cfg || !out) return fail(nullptr, SAG_ERR_ARG, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SAG_ABI_VERSION)
    return fail(nullptr, SAG_ERR_ARG, "ABI version %d, library is %d", cfg->abi_version, SAG_ABI_VERSION);
  if (cfg->robot < 0 || cfg->robot > 2) return fail(nullptr, SAG_ERR_ARG, "bad robot %d", cfg->robot);
  if (cfg->n_envs <= 0) return fail(nullptr, SAG_ERR_ARG, "n_envs must be positive");
  if (cfg->max_hazards < 0 || cfg->max_hazards > SAG_MAX_HAZARDS || cfg->max_vases < 0 ||
      cfg->max_vases > SAG_MAX_VASES || cfg->max_pillars < 0 || cfg->max_pillars > SAG_MAX_PILLARS ||
      cfg->max_buttons < 0 || cfg->max_buttons > SAG_MAX_BUTTONS)
    return fail(nullptr, SAG_ERR_ARG, "capacity out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(nullptr, SAG_ERR_NODEVICE, "no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev)
    return fail(nullptr, SAG_ERR_NODEVICE, "device %d out of range (%d visible)", cfg->device, ndev);
  sag_ctx* c = new sag_ctx();
  c->cfg = *cfg; c->rb = ROBOTS[cfg->robot]; c->N = cfg->n_envs;
  // below ~one resident round of wavefronts a step is latency-bound and two dependent launches
  // cost more than the divergence they remove
  c->split = c->N >= (cfg->robot == SAG_ROBOT_CAR ? SAG_SPLIT_MIN_ENVS_CAR : SAG_SPLIT_MIN_ENVS);
  if (const char* e = getenv("SAG_SPLIT")) c->split = atoi(e) != 0;
  const size_t N = (size_t)c->N;
#define CREATE_CHK(call)                                                                         \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      int rc_ = fail(nullptr, SAG_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));       \
      sag_destroy(c);                                                                            \
      return rc_;                                                                                \
    }                                                                                            \
  } while (0)
  CREATE_CHK(hipSetDevice(cfg->device));
  CREATE_CHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  {
    int lo = 0, hi = 0;  // (numerically lower = higher priority)
    CREATE_CHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CREATE_CHK(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, lo));
  }
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_xsrc, hipEventDisableTiming));
  CREATE_CHK(hipEventCreateWithFlags(&c->ev_xdone, hipEventDisableTiming));
  if (const char* e = getenv("SAG_EARLY_FORK")) c->early_fork = atoi(e);
  if (const char* e = getenv("SAG_BUSY_KINDS")) c->busy_kinds = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("SAG_BUSY_KINDS_MIN")) c->kinds_min = atoi(e);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
  }
  CREATE_CHK(hipMalloc(&c->S, N * DEV_FLOATS * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->I, icount(N) * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->G, N * 3 * NBODY * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->d_rows, BUSY_CLASSES * N * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->d_kind, N));
  CREATE_CHK(hipMemset(c->d_kind, 0, N));
  CREATE_CHK(hipMalloc(&c->d_count, (2 * BUSY_CLASSES + 1) * sizeof(int32_t)));   // (+ the env count of the last busy launch)
  CREATE_CHK(hipMemset(c->d_count, 0, (2 * BUSY_CLASSES + 1) * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->L_f, N * SAG_REC_FLOATS * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->L_i, N * SAG_REC_INTS * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->st_f, N * SAG_REC_FLOATS * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->st_i, N * SAG_REC_INTS * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->st_ids, N * sizeof(int32_t)));
  CREATE_CHK(hipMalloc(&c->d_act, N * c->rb.nu * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->d_noise, N * c->rb.nu * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->d_obs, N * c->rb.obs_dim * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->d_rew, N * 2 * sizeof(float)));
  CREATE_CHK(hipMalloc(&c->d_cost, N));
  CREATE_CHK(hipMalloc(&c->d_done, N));
  CREATE_CHK(hipMalloc(&c->d_met, N));
  CREATE_CHK(hipMalloc(&c->d_used, N * sizeof(int32_t)));
  if (c->split && cfg->robot != SAG_ROBOT_DOGGO)
    CREATE_CHK(hipMalloc(&c->d_hot, N * (HOT_FLOATS + 20) * sizeof(float)));
  if (cfg->robot == SAG_ROBOT_DOGGO) {
    CREATE_CHK(hipMalloc(&c->d_dr, N * DR_STRIDE * sizeof(double)));
    CREATE_CHK(hipMalloc(&c->d_dg_sched, dc_sched_ints(N) * sizeof(int32_t)));
    CREATE_CHK(hipMemset(c->d_dg_sched, 0, dc_sched_ints(N) * sizeof(int32_t)));
    if (const char* e = getenv("SAG_DOGGO_SCHED")) c->dg_sched_on = atoi(e) != 0;
  }
  if (cfg->robot == SAG_ROBOT_DOGGO) {
    DgModel model;
    dg_build_model(model);
    CREATE_CHK(hipMemcpyToSymbol(HIP_SYMBOL(g_dg), &model, sizeof(model)));
  }
  CREATE_CHK(hipMemsetAsync(c->d_cost, 0, N, c->stream));
  CREATE_CHK(hipMemsetAsync(c->d_obs, 0, N * c->rb.obs_dim * sizeof(float), c->stream));
  CREATE_CHK(hipMemsetAsync(c->S, 0, N * DEV_FLOATS * sizeof(float), c->stream));
  CREATE_CHK(hipMemsetAsync(c->I, 0, icount(N) * sizeof(int32_t), c->stream));
  CREATE_CHK(hipStreamSynchronize(c->stream));
#undef CREATE_CHK
  *out = c;
  return SAG_OK;
}

int sag_destroy(sag_ctx* c) {
  if (!c) return SAG_OK;
  (void)hipSetDevice(c->cfg.device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& e : c->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
  void* bufs[] = {c->S, c->I, c->G, c->d_rows, c->d_count, c->d_kind, c->L_f, c->L_i, c->st_f, c->st_i, c->st_ids, c->d_act, c->d_noise,
                  c->d_tape, c->d_obs, c->d_rew, c->d_cost, c->d_done, c->d_met, c->d_used, c->scratch, c->d_rgb, c->d_dr, c->d_dg_sched, c->d_hot,
                  c->d_ext_cc, c->d_ext_btn, c->d_descs, c->d_desc_of_env, c->d_rstat, c->d_rbound, c->d_rtot, c->d_acc, c->d_ftot, c->d_palive, c->d_prank, c->d_pshift, c->d_pgrad, c->d_lpart, c->d_obsn};
  for (void* b : bufs) if (b) (void)hipFree(b);
  if (c->pin) (void)hipHostFree(c->pin);
  if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_xsrc) (void)hipEventDestroy(c->ev_xsrc);
  if (c->ev_xdone) (void)hipEventDestroy(c->ev_xdone);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return SAG_OK;
}

// a new episode starts without a cost flag: sag_render's cost overlay reads d_cost of the last host-buffer step
__global__ void k_clear_cost(uint8_t* cost, const int32_t* ids, int n) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) cost[ids ? ids[j] : j] = 0;
}

static int upload_records(sag_ctx* c, const int32_t* env_ids, int32_t n, const float* rec_f,
                          const int32_t* rec_i) {
  if (n <= 0 || n > c->N || !rec_f || !rec_i) return fail(c, SAG_ERR_ARG, "bad record batch (n=%d)", n);
  if (env_ids)
    for (int k = 0; k < n; k++)
      if (env_ids[k] < 0 || env_ids[k] >= c->N) return fail(c, SAG_ERR_ARG, "env id %d out of range", env_ids[k]);
  for (int k = 0; k < n; k++) {
    const int32_t* ri = rec_i + (size_t)k * SAG_REC_INTS;
    if (ri[SAG_I_TASK] < 0 || ri[SAG_I_TASK] >= SAG_NUM_TASKS || ri[SAG_I_NH] < 0 ||
        ri[SAG_I_NH] > c->cfg.max_hazards || ri[SAG_I_NV] < 0 || ri[SAG_I_NV] > c->cfg.max_vases ||
        ri[SAG_I_NP] < 0 || ri[SAG_I_NP] > c->cfg.max_pillars || ri[SAG_I_NB] < 0 ||
        ri[SAG_I_NB] > c->cfg.max_buttons || ri[SAG_I_BOX_KIND] < 0 || ri[SAG_I_BOX_KIND] > 3 ||
        (ri[SAG_I_BOX_KIND] != 0 && !c->cfg.has_box) || ri[SAG_I_GOAL_BUTTON] < 0 ||
        ri[SAG_I_GOAL_BUTTON] >= SAG_MAX_BUTTONS || ri[SAG_I_BTN_TIMER] < 0 || ri[SAG_I_BTN_TIMER] > 5 ||
        ri[SAG_I_CATCH_TIMER] < 0 || ri[SAG_I_CATCH_TIMER] > 10 ||
        ri[SAG_I_EPISODE] < 0 || ri[SAG_I_EPISODE] > 0xffffff)   // the nonce is 24 bits of the flags word: no silent truncation
      return fail(c, SAG_ERR_ARG, "record %d exceeds the context's capacities or has a bad field", k);
  }
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(c->st_f, rec_f, (size_t)n * SAG_REC_FLOATS * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->st_i, rec_i, (size_t)n * SAG_REC_INTS * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (env_ids)
    HIPCHK(c, hipMemcpyAsync(c->st_ids, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return 0;
}

int sag_set_layout(sag_ctx* c, const int32_t* env_ids, int32_t n, const float* rec_f, const int32_t* rec_i) {
  if (!c) return SAG_ERR_ARG;
  int rc = upload_records(c, env_ids, n, rec_f, rec_i);
  if (rc) return rc;
  hipLaunchKernelGGL(k_install, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                     env_ids ? c->st_ids : nullptr, n, c->st_f, c->st_i, 1);
  c->hot_valid = false;  // state changed outside a step
  c->ext_pending = false;   // contact results supplied for another state do not carry over (sag_set_ext_contacts: "for the NEXT step")
  hipLaunchKernelGGL(k_clear_cost, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_cost, env_ids ? c->st_ids : nullptr, n);
  // keep a copy for sag_reset: read the installed state back into the AoS layout store
  hipLaunchKernelGGL(k_extract, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                     env_ids ? c->st_ids : nullptr, n, c->st_f, c->st_i);
  HIPCHK(c, hipGetLastError());
  // the layout store keeps the records as installed, by env id (one scatter launch, not 2 n copies)
  if (!env_ids) {
    HIPCHK(c, hipMemcpyAsync(c->L_f, c->st_f, (size_t)n * SAG_REC_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->L_i, c->st_i, (size_t)n * SAG_REC_INTS * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
  } else {
    const size_t pieces = (size_t)n * (SAG_REC_FLOATS / 4 + SAG_REC_INTS / 4);
    hipLaunchKernelGGL(k_move_rows, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, c->stream, c->L_f, c->L_i, c->st_f,
                       c->st_i, c->st_ids, n, 0, 0);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_layout = true;
  return SAG_OK;
}

int sag_set_state(sag_ctx* c, const int32_t* env_ids, int32_t n, const float* rec_f, const int32_t* rec_i) {
  if (!c) return SAG_ERR_ARG;
  int rc = upload_records(c, env_ids, n, rec_f, rec_i);
  if (rc) return rc;
  hipLaunchKernelGGL(k_install, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                     env_ids ? c->st_ids : nullptr, n, c->st_f, c->st_i, 0);
  c->hot_valid = false;  // state changed outside a step
  c->ext_pending = false;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_layout = true;
  return SAG_OK;
}

int sag_get_state(sag_ctx* c, const int32_t* env_ids, int32_t n, float* rec_f, int32_t* rec_i) {
  if (!c) return SAG_ERR_ARG;
  if (n <= 0 || n > c->N || !rec_f || !rec_i) return fail(c, SAG_ERR_ARG, "bad record batch (n=%d)", n);
  if (env_ids)
    for (int k = 0; k < n; k++)
      if (env_ids[k] < 0 || env_ids[k] >= c->N) return fail(c, SAG_ERR_ARG, "env id %d out of range", env_ids[k]);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (env_ids)
    HIPCHK(c, hipMemcpyAsync(c->st_ids, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_extract, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                     env_ids ? c->st_ids : nullptr, n, c->st_f, c->st_i);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(rec_f, c->st_f, (size_t)n * SAG_REC_FLOATS * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(rec_i, c->st_i, (size_t)n * SAG_REC_INTS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_reset(sag_ctx* c, const int32_t* env_ids, int32_t n) {
  if (!c) return SAG_ERR_ARG;
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_reset before sag_set_layout");
  if (n <= 0 || n > c->N) return fail(c, SAG_ERR_ARG, "bad n=%d", n);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  // a new episode of the same layout: the episode nonce of the counter-based generator advances
  if (!env_ids) {
    hipLaunchKernelGGL(k_bump_episode, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->L_i, n);
    hipLaunchKernelGGL(k_install, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                       (const int32_t*)nullptr, n, c->L_f, c->L_i, 0);
  } else {
    for (int k = 0; k < n; k++)
      if (env_ids[k] < 0 || env_ids[k] >= c->N) return fail(c, SAG_ERR_ARG, "env id %d out of range", env_ids[k]);
    // gather the chosen layout rows into staging (one launch), then install
    HIPCHK(c, hipMemcpyAsync(c->st_ids, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const size_t pieces = (size_t)n * (SAG_REC_FLOATS / 4 + SAG_REC_INTS / 4);
    hipLaunchKernelGGL(k_move_rows, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, c->stream, c->st_f, c->st_i, c->L_f,
                       c->L_i, c->st_ids, n, 1, 1);
    hipLaunchKernelGGL(k_install, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, c->N,
                       c->st_ids, n, c->st_f, c->st_i, 0);
  }
  hipLaunchKernelGGL(k_clear_cost, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_cost, env_ids ? c->st_ids : nullptr, n);
  c->hot_valid = false;  // state changed outside a step
  c->ext_pending = false;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_set_tasks(sag_ctx* c, const sag_task_desc* descs, int32_t n_descs, const int32_t* desc_of_env, const sag_world_config* cfg,
                  int32_t env_id0) {
  if (!c) return SAG_ERR_ARG;
  if (!descs || n_descs <= 0 || !desc_of_env || !cfg || env_id0 < 0) return fail(c, SAG_ERR_ARG, "sag_set_tasks: bad arguments");
  for (int k = 0; k < n_descs; k++) {
    const sag_task_desc& d = descs[k];
    if (const char* why = sag_task_desc_check(&d)) return fail(c, SAG_ERR_ARG, "task descriptor %d: %s", k, why);
    if (d.n_hazards > c->cfg.max_hazards || d.n_vases > c->cfg.max_vases || d.n_pillars > c->cfg.max_pillars ||
        d.n_buttons > c->cfg.max_buttons || (d.box_kind != SAG_BOX_NONE && !c->cfg.has_box))
      return fail(c, SAG_ERR_ARG, "task descriptor %d exceeds the context's capacities", k);
  }
  for (int i = 0; i < c->N; i++)
    if (desc_of_env[i] < 0 || desc_of_env[i] >= n_descs) return fail(c, SAG_ERR_ARG, "env %d: descriptor %d of %d", i, desc_of_env[i], n_descs);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (n_descs > c->n_descs) {
    if (c->d_descs) HIPCHK(c, hipFree(c->d_descs));
    c->d_descs = nullptr; c->n_descs = 0;
    HIPCHK(c, hipMalloc(&c->d_descs, (size_t)n_descs * sizeof(sag_task_desc)));
    c->n_descs = n_descs;
  }
  if (!c->d_desc_of_env) HIPCHK(c, hipMalloc(&c->d_desc_of_env, (size_t)c->N * sizeof(int32_t)));
  if (!c->d_rstat) HIPCHK(c, hipMalloc(&c->d_rstat, ((size_t)c->N + 2) * sizeof(int32_t)));
  if (!c->d_rbound) HIPCHK(c, hipMalloc(&c->d_rbound, (size_t)c->N * sizeof(float)));
  if (!c->d_rtot) {
    HIPCHK(c, hipMalloc(&c->d_rtot, 2 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->d_rtot, 0, 2 * sizeof(unsigned long long), c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(c->d_descs, descs, (size_t)n_descs * sizeof(sag_task_desc), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_desc_of_env, desc_of_env, (size_t)c->N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host arrays are the caller's
  c->rcfg = *cfg; c->env_id0 = env_id0;
  c->h_descs.assign(descs, descs + n_descs);
  c->have_tasks = true;
  return SAG_OK;
}

int sag_reset_device(sag_ctx* c, int32_t first_episode, int32_t episode0, const uint8_t* d_mask, int32_t* status, float* bound) {
  if (!c) return SAG_ERR_ARG;
  if (!c->have_tasks) return fail(c, SAG_ERR_STATE, "sag_reset_device before sag_set_tasks");
  if (!first_episode && !c->have_layout) return fail(c, SAG_ERR_STATE, "sag_reset_device: a later episode needs an installed layout");
  if (episode0 < 0 || episode0 > 0xffffff) return fail(c, SAG_ERR_ARG, "episode0 %d is not a 24-bit nonce", episode0);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int N = c->N;
  int32_t* counters = c->d_rstat + N;   // [0] listed envs, [1] failures
  HIPCHK(c, hipMemsetAsync(c->d_rstat, 0, ((size_t)N + 2) * sizeof(int32_t), c->stream));
  int n = N;
  const int32_t* ids = nullptr;
  if (d_mask) {
    hipLaunchKernelGGL(k_reset_list, dim3((N + 255) / 256), dim3(256), 0, c->stream, d_mask, N, c->st_ids, counters);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&n, counters, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ids = c->st_ids;
  }
  int32_t n_fail = 0;
  if (n > 0) {
    ResetArgs a;
    a.descs = c->d_descs; a.desc_of_env = c->d_desc_of_env; a.cfg = c->rcfg; a.S = c->S; a.I = c->I; a.N = N;
    a.ids = ids; a.n = n; a.n_dev = nullptr; a.robot = c->cfg.robot; a.first_episode = first_episode != 0; a.have_state = c->have_layout;
    a.episode0 = (uint32_t)episode0; a.env_id0 = c->env_id0;
    a.k0 = (uint32_t)(c->cfg.seed & 0xffffffffu); a.k1 = (uint32_t)(c->cfg.seed >> 32);
    a.rec_f = c->st_f; a.rec_i = c->st_i; a.status = c->d_rstat; a.n_fail = counters + 1;
    // a persistent grid: the lanes stride over the list, as many wavefronts as the LDS holds (5 per CU)
    const int blocks = std::min((n + RS_BLOCK - 1) / RS_BLOCK, 5 * c->n_cu);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = timing_events(c, &e0, &e1);
    if (rc) return rc;
    if (e0) HIPCHK(c, hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(k_reset_sample, dim3(blocks), dim3(RS_BLOCK), 0, c->stream, a);
    if (e1) HIPCHK(c, hipEventRecord(e1, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&n_fail, counters + 1, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (n > 0 && n_fail == 0) {   // install exactly as sag_set_layout does, from the staging records
    hipLaunchKernelGGL(k_install, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, N, ids, n, c->st_f, c->st_i, 1);
    hipLaunchKernelGGL(k_clear_cost, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->d_cost, ids, n);
    hipLaunchKernelGGL(k_extract, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->S, c->I, N, ids, n, c->st_f, c->st_i);
    HIPCHK(c, hipGetLastError());
    if (!ids) {
      HIPCHK(c, hipMemcpyAsync(c->L_f, c->st_f, (size_t)n * SAG_REC_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(c->L_i, c->st_i, (size_t)n * SAG_REC_INTS * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    } else {
      const size_t pieces = (size_t)n * (SAG_REC_FLOATS / 4 + SAG_REC_INTS / 4);
      hipLaunchKernelGGL(k_move_rows, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, c->stream, c->L_f, c->L_i, c->st_f,
                         c->st_i, ids, n, 0, 0);
      HIPCHK(c, hipGetLastError());
    }
    c->hot_valid = false;
    c->ext_pending = false;
    c->have_layout = true;
  }
  if (status) HIPCHK(c, hipMemcpyAsync(status, c->d_rstat, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (bound && c->have_layout) {
    hipLaunchKernelGGL(k_reset_bound, dim3((N + 255) / 256), dim3(256), 0, c->stream, c->S, N, c->d_rbound);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(bound, c->d_rbound, (size_t)N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return n_fail;
}

// episode accumulators: one float4 per env, allocated and zeroed (stream-ordered) on first use
static int ensure_acc(sag_ctx* c) {
  if (c->d_acc) return 0;
  HIPCHK(c, hipMalloc(&c->d_acc, (size_t)c->N * 4 * sizeof(float)));
  HIPCHK(c, hipMemsetAsync(c->d_acc, 0, (size_t)c->N * 4 * sizeof(float), c->stream));
  return 0;
}

// list -> sample -> commit -> observation, nothing in between that the host decides: the list's length stays on the
// device, so the three launches after the list are sized for n_envs and return at once where their share is empty
int sag_reset_device_async(sag_ctx* c, const uint8_t* d_mask, float* d_obs) {
  if (!c) return SAG_ERR_ARG;
  if (!c->have_tasks) return fail(c, SAG_ERR_STATE, "sag_reset_device_async before sag_set_tasks");
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_reset_device_async: a later episode needs an installed layout");
  const bool doggo = c->cfg.robot == SAG_ROBOT_DOGGO;
  if (doggo && (reinterpret_cast<uintptr_t>(d_obs) & 15)) return fail(c, SAG_ERR_ARG, "sag_reset_device_async: d_obs must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int N = c->N;
  int32_t* counters = c->d_rstat + N;   // [0] listed envs, [1] failures of this call
  HIPCHK(c, hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(k_reset_list, dim3((N + 255) / 256), dim3(256), 0, c->stream, d_mask, N, c->st_ids, counters);
  ResetArgs a;
  a.descs = c->d_descs; a.desc_of_env = c->d_desc_of_env; a.cfg = c->rcfg; a.S = c->S; a.I = c->I; a.N = N;
  a.ids = c->st_ids; a.n = 0; a.n_dev = counters; a.robot = c->cfg.robot; a.first_episode = 0; a.have_state = 1;
  a.episode0 = 0; a.env_id0 = c->env_id0;
  a.k0 = (uint32_t)(c->cfg.seed & 0xffffffffu); a.k1 = (uint32_t)(c->cfg.seed >> 32);
  a.rec_f = c->st_f; a.rec_i = c->st_i; a.status = c->d_rstat; a.n_fail = counters + 1;
  hipLaunchKernelGGL(k_reset_sample, dim3(std::min((N + RS_BLOCK - 1) / RS_BLOCK, 5 * c->n_cu)), dim3(RS_BLOCK), 0, c->stream, a);
  CommitArgs m;
  m.S = c->S; m.I = c->I; m.N = N; m.ids = c->st_ids; m.n_dev = counters; m.rec_f = c->st_f; m.rec_i = c->st_i;
  m.status = c->d_rstat; m.cost = c->d_cost; m.L_f = c->L_f; m.L_i = c->L_i;
  m.hot = c->d_hot; m.hot_haz = c->d_hot ? c->d_hot + (size_t)N * HOT_FLOATS : nullptr;   // (the env's own record: hot_valid stays as it is)
  m.acc = reinterpret_cast<float4*>(c->d_acc); m.totals = c->d_rtot;
  hipLaunchKernelGGL(k_reset_commit, dim3((N + 255) / 256), dim3(256), 0, c->stream, m);
  HIPCHK(c, hipGetLastError());
  c->ext_pending = false;   // contact results were supplied for another state, and the host cannot know that the mask was empty
  if (!d_obs) return SAG_OK;
  if (doggo) {   // the whole batch into the context's own buffer, then the rows of the list
    int rc = launch_step(c, nullptr, nullptr, nullptr, 0, 0, c->d_obs, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
    if (rc) return rc;
    const int Q = c->rb.obs_dim / 4;
    hipLaunchKernelGGL(k_copy_rows, dim3((unsigned)(((size_t)N * Q + 255) / 256)), dim3(256), 0, c->stream, c->st_ids, counters,
                       c->d_rstat, Q, reinterpret_cast<const float4*>(c->d_obs), reinterpret_cast<float4*>(d_obs));
    HIPCHK(c, hipGetLastError());
    return SAG_OK;
  }
  StepArgs o;
  o.S = c->S; o.I = c->I; o.N = N;
  o.actions = nullptr; o.noise = nullptr; o.tape = nullptr; o.tape_len = 0;
  o.nstep = 0; o.nstep_table = c->rb.nstep; o.h = (float)c->rb.dt; o.car = car_fric_constants(o.h);
  o.key0 = a.k0; o.key1 = a.k1;
  o.obs = d_obs; o.reward = nullptr; o.cost = nullptr; o.done = nullptr; o.goal_met = nullptr; o.tape_used = nullptr;
  o.max_vases = c->cfg.max_vases; o.max_hazards = c->cfg.max_hazards; o.max_pillars = c->cfg.max_pillars;
  o.max_buttons = c->cfg.max_buttons; o.has_box = c->cfg.has_box; o.G = c->G; o.observe_only = 1;
  o.phase = c->phase; o.rows = nullptr; o.count = nullptr; o.DR = nullptr; o.dg_sched = nullptr; o.dg_phase = -1;
  o.hot = nullptr; o.hot_haz = nullptr; o.ext_cc = nullptr; o.ext_btn = nullptr;
  o.envs_per_wave = WAVE; o.busy_slots = 8 * c->n_cu; o.busy_kinds = 0; o.kind = nullptr; o.busy_total = nullptr;
  const bool btn = c->cfg.max_buttons > 0, tbox = c->cfg.has_box != 0;
  const dim3 grid((N + WAVE - 1) / WAVE);
#define SAG_OBSERVE_ROWS(ROB, B_, X_) \
  hipLaunchKernelGGL((k_observe_rows<ROB, B_, X_>), grid, dim3(WAVE), 0, c->stream, o, (const int32_t*)c->st_ids, (const int32_t*)counters, (const int32_t*)c->d_rstat)
#define SAG_OBSERVE(ROB)                                \
  do {                                                  \
    if (!btn && !tbox) SAG_OBSERVE_ROWS(ROB, false, false); \
    else if (btn && !tbox) SAG_OBSERVE_ROWS(ROB, true, false); \
    else if (!btn && tbox) SAG_OBSERVE_ROWS(ROB, false, true); \
    else SAG_OBSERVE_ROWS(ROB, true, true);             \
  } while (0)
  // (the context's own instantiation, as sag_observe runs it: the rows equal its rows bit for bit)
  if (false) {}
#if SAG_ONLY_ROBOT < 0 || SAG_ONLY_ROBOT == 0
  else if (c->cfg.robot == SAG_ROBOT_POINT) SAG_OBSERVE(SAG_ROBOT_POINT);
#endif
#if SAG_ONLY_ROBOT < 0 || SAG_ONLY_ROBOT == 1
  else if (c->cfg.robot == SAG_ROBOT_CAR) SAG_OBSERVE(SAG_ROBOT_CAR);
#endif
  else return fail(c, SAG_ERR_UNSUPPORTED, "this build holds the step kernels of robot %d only", SAG_ONLY_ROBOT);
#undef SAG_OBSERVE
#undef SAG_OBSERVE_ROWS
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_reset_device_counts(sag_ctx* c, int32_t clear, uint64_t* n_reset, uint64_t* n_failed) {
  if (!c) return SAG_ERR_ARG;
  unsigned long long tot[2] = {0, 0};
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (c->d_rtot) {
    HIPCHK(c, hipMemcpyAsync(tot, c->d_rtot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    if (clear) HIPCHK(c, hipMemsetAsync(c->d_rtot, 0, sizeof(tot), c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_reset) *n_reset = tot[0];
  if (n_failed) *n_failed = tot[1];
  return SAG_OK;
}

int sag_episode_track_device(sag_ctx* c, const float* d_reward, const uint8_t* d_cost, const uint8_t* d_done, const uint8_t* d_goal_met,
                             int32_t max_steps, uint8_t* d_ended, float* d_episode) {
  if (!c) return SAG_ERR_ARG;
  if (!d_reward || !d_cost || !d_done || !d_goal_met || !d_ended || !d_episode || max_steps < 0)
    return fail(c, SAG_ERR_ARG, "sag_episode_track_device: NULL buffer or negative max_steps");
  if ((reinterpret_cast<uintptr_t>(d_reward) & 7) || (reinterpret_cast<uintptr_t>(d_episode) & 15))
    return fail(c, SAG_ERR_ARG, "sag_episode_track_device: d_reward must be 8-byte and d_episode 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  int rc = ensure_acc(c);
  if (rc) return rc;
  hipLaunchKernelGGL(k_episode_track, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N, d_reward, d_cost, d_done, d_goal_met,
                     max_steps, reinterpret_cast<float4*>(c->d_acc), d_ended, reinterpret_cast<float4*>(d_episode));
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_episode_clear(sag_ctx* c, const uint8_t* d_mask) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const bool fresh = !c->d_acc;   // (then zeroed just now)
  int rc = ensure_acc(c);
  if (rc || fresh) return rc;
  if (!d_mask) {
    HIPCHK(c, hipMemsetAsync(c->d_acc, 0, (size_t)c->N * 4 * sizeof(float), c->stream));
    return SAG_OK;
  }
  hipLaunchKernelGGL(k_episode_clear, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N, d_mask, reinterpret_cast<float4*>(c->d_acc));
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_copy_rows_device(sag_ctx* c, const uint8_t* d_mask, int32_t row_bytes, const void* d_src, void* d_dst) {
  if (!c) return SAG_ERR_ARG;
  if (!d_src || !d_dst || d_src == d_dst) return fail(c, SAG_ERR_ARG, "sag_copy_rows_device: d_src and d_dst must be two buffers, neither NULL");
  if (row_bytes <= 0 || (row_bytes & 15)) return fail(c, SAG_ERR_ARG, "sag_copy_rows_device: row_bytes %d is not a positive multiple of 16", row_bytes);
  if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) & 15)
    return fail(c, SAG_ERR_ARG, "sag_copy_rows_device: d_src and d_dst must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(k_save_rows, dim3((c->N + WAVE - 1) / WAVE), dim3(WAVE), 0, c->stream, c->N, d_mask, row_bytes / 16,
                     reinterpret_cast<const float4*>(d_src), reinterpret_cast<float4*>(d_dst));
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// decide -> state -> layout rows -> int words and what hangs on an env, on dst's stream.  Between two contexts the source's
// stream is joined first (what is enqueued there, a step for one, is seen) and waits for the copy afterwards (its next step
// cannot overtake the reads).
int sag_fork_device(sag_ctx* c, sag_ctx* s, const int32_t* d_src, int32_t flags) {
  if (!c) return SAG_ERR_ARG;
  if (!s) return fail(c, SAG_ERR_ARG, "sag_fork_device: the source context is NULL");
  if (!d_src) return fail(c, SAG_ERR_ARG, "sag_fork_device: d_src is NULL");
  if (flags & ~SAG_FORK_SAME_STREAM) return fail(c, SAG_ERR_ARG, "sag_fork_device: unknown flag bits 0x%x", flags & ~SAG_FORK_SAME_STREAM);
  if (s->cfg.robot != c->cfg.robot) return fail(c, SAG_ERR_ARG, "sag_fork_device: robot %d into robot %d", s->cfg.robot, c->cfg.robot);
  if (s->cfg.device != c->cfg.device) return fail(c, SAG_ERR_ARG, "sag_fork_device: device %d into device %d", s->cfg.device, c->cfg.device);
  if (s->cfg.max_hazards != c->cfg.max_hazards || s->cfg.max_vases != c->cfg.max_vases || s->cfg.max_pillars != c->cfg.max_pillars ||
      s->cfg.max_buttons != c->cfg.max_buttons || (s->cfg.has_box != 0) != (c->cfg.has_box != 0))
    return fail(c, SAG_ERR_ARG, "sag_fork_device: the contexts' capacities differ");
  if (!s->have_layout || !c->have_layout) return fail(c, SAG_ERR_STATE, "sag_fork_device before sag_set_layout");
  if (c->have_tasks && !s->have_tasks)
    return fail(c, SAG_ERR_STATE, "sag_fork_device: the destination has tasks and the source none (a later device reset would sample for the wrong task)");
  const bool tasks = c->have_tasks && s->have_tasks;
  if (tasks && s != c && (s->h_descs.size() != c->h_descs.size() ||
                          memcmp(s->h_descs.data(), c->h_descs.data(), c->h_descs.size() * sizeof(sag_task_desc)) != 0))
    return fail(c, SAG_ERR_ARG, "sag_fork_device: the contexts' task descriptor tables differ");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (!c->d_ftot) {
    HIPCHK(c, hipMalloc(&c->d_ftot, 2 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->d_ftot, 0, 2 * sizeof(unsigned long long), c->stream));
  }
  if (s != c) {
    HIPCHK(c, hipEventRecord(s->ev_xsrc, s->stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, s->ev_xsrc, 0));
  }
  ForkArgs p;
  p.S = c->S; p.I = c->I; p.N = c->N; p.src_S = s->S; p.src_I = s->I; p.src_N = s->N;
  p.src = d_src; p.from = c->st_ids; p.same_stream = (flags & SAG_FORK_SAME_STREAM) != 0;
  p.L_f = c->L_f; p.L_i = c->L_i; p.src_L_f = s->L_f; p.src_L_i = s->L_i;
  p.acc = reinterpret_cast<float4*>(c->d_acc); p.src_acc = reinterpret_cast<const float4*>(s->d_acc);
  p.cost = c->d_cost; p.src_cost = s->d_cost;
  p.desc_of_env = tasks ? c->d_desc_of_env : nullptr; p.src_desc_of_env = tasks ? s->d_desc_of_env : nullptr;
  p.hot = c->d_hot; p.hot_haz = c->d_hot ? c->d_hot + (size_t)c->N * HOT_FLOATS : nullptr;   // (the env's own record: hot_valid stays as it is)
  p.totals = c->d_ftot;
  const unsigned blocks = (unsigned)((c->N + 255) / 256);
  const size_t pieces = (size_t)c->N * FORK_ROW_PIECES;
  hipLaunchKernelGGL(k_fork_decide, dim3(blocks), dim3(256), 0, c->stream, p);
  hipLaunchKernelGGL(k_fork_state, dim3(blocks * FORK_CHUNKS), dim3(256), 0, c->stream, p);
  hipLaunchKernelGGL(k_fork_rows, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, c->stream, p);
  hipLaunchKernelGGL(k_fork_finish, dim3(blocks), dim3(256), 0, c->stream, p);
  HIPCHK(c, hipGetLastError());
  c->ext_pending = false;   // contact results were supplied for another state
  if (s != c) {
    HIPCHK(c, hipEventRecord(c->ev_xdone, c->stream));
    HIPCHK(c, hipStreamWaitEvent(s->stream, c->ev_xdone, 0));
  }
  return SAG_OK;
}

int sag_fork_counts(sag_ctx* c, int32_t clear, uint64_t* n_copied, uint64_t* n_rejected) {
  if (!c) return SAG_ERR_ARG;
  unsigned long long tot[2] = {0, 0};
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (c->d_ftot) {
    HIPCHK(c, hipMemcpyAsync(tot, c->d_ftot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
    if (clear) HIPCHK(c, hipMemsetAsync(c->d_ftot, 0, sizeof(tot), c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_copied) *n_copied = tot[0];
  if (n_rejected) *n_rejected = tot[1];
  return SAG_OK;
}

int sag_wait_for(sag_ctx* c, sag_ctx* producer) {
  if (!c) return SAG_ERR_ARG;
  if (!producer) return fail(c, SAG_ERR_ARG, "sag_wait_for: the producer context is NULL");
  if (producer->cfg.device != c->cfg.device) return fail(c, SAG_ERR_ARG, "sag_wait_for: device %d and device %d", producer->cfg.device, c->cfg.device);
  if (producer == c) return SAG_OK;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipEventRecord(producer->ev_xdone, producer->stream));
  HIPCHK(c, hipStreamWaitEvent(c->stream, producer->ev_xdone, 0));
  return SAG_OK;
}

// ---- shooting planner (sag_plan.hpp) ----
namespace {

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
bool plan_scale_ok(float x) { return std::isfinite(x) && x >= 0.0f; }

// K candidates per group of a context: 0 if the arguments are refused (the message is set)
int plan_groups(sag_ctx* c, const char* who, int32_t K, int32_t H) {
  if (K < 1 || c->N % K != 0) { fail(c, SAG_ERR_ARG, "%s: K = %d does not divide the context's %d envs", who, K, c->N); return 0; }
  if (H < 1) { fail(c, SAG_ERR_ARG, "%s: H = %d", who, H); return 0; }
  return c->N / K;
}

int ensure_plan_scratch(sag_ctx* c) {
  if (c->d_palive) return 0;
  HIPCHK(c, hipMalloc(&c->d_prank, (size_t)c->N * sizeof(int32_t)));
  HIPCHK(c, hipMalloc(&c->d_palive, (size_t)c->N));
  return 0;
}

}  // namespace

int sag_plan_sample_device(sag_ctx* c, int32_t K, int32_t H, const float* d_mean, const float* d_sigma, uint32_t draw, float* d_plans) {
  if (!c) return SAG_ERR_ARG;
  if (!d_mean || !d_sigma || !d_plans || misaligned(d_mean, 8) || misaligned(d_sigma, 8) || misaligned(d_plans, 8))
    return fail(c, SAG_ERR_ARG, "sag_plan_sample_device: NULL buffer, or one that is not 8-byte aligned");
  if (!plan_groups(c, "sag_plan_sample_device", K, H)) return SAG_ERR_ARG;
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_plan_sample_device before sag_set_layout");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t lanes = (size_t)((H * c->rb.nu + 3) / 4) * (size_t)c->N;
  hipLaunchKernelGGL(k_plan_sample, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, c->stream, c->N, K, H, c->rb.nu, (uint32_t)c->env_id0, draw,
                     (uint32_t)(c->cfg.seed & 0xffffffffu), (uint32_t)(c->cfg.seed >> 32), d_mean, d_sigma, d_plans);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// H times: the step on step t's block of the plans - no observation, context-owned reward / cost / done / met - then the accumulation
int sag_plan_score_device(sag_ctx* c, const float* d_plans, int32_t H, float gamma, float* d_score) {
  if (!c) return SAG_ERR_ARG;
  if (!d_plans || !d_score || misaligned(d_plans, 8) || misaligned(d_score, 16))
    return fail(c, SAG_ERR_ARG, "sag_plan_score_device: NULL buffer, d_plans not 8-byte or d_score not 16-byte aligned");
  if (H < 1) return fail(c, SAG_ERR_ARG, "sag_plan_score_device: H = %d", H);
  if (!(gamma > 0.0f && gamma <= 1.0f)) return fail(c, SAG_ERR_ARG, "sag_plan_score_device: gamma = %g is outside (0, 1]", (double)gamma);
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_plan_score_device before sag_set_layout");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  int rc = ensure_plan_scratch(c);
  if (rc) return rc;
  const size_t N = (size_t)c->N;
  HIPCHK(c, hipMemsetAsync(d_score, 0, N * 4 * sizeof(float), c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_palive, 1, N, c->stream));
  float w = 1.0f;
  for (int t = 0; t < H; t++) {
    rc = launch_step(c, d_plans + (size_t)t * N * c->rb.nu, nullptr, nullptr, 0, -1, nullptr, c->d_rew, c->d_cost, c->d_done, c->d_met, nullptr, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(k_plan_accumulate, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, c->N, w, c->d_rew, c->d_cost, c->d_done, c->d_met,
                       c->d_palive, reinterpret_cast<float4*>(d_score));
    HIPCHK(c, hipGetLastError());
    w = w * gamma;
  }
  return SAG_OK;
}

int sag_plan_refit_device(sag_ctx* c, int32_t K, int32_t H, int32_t E, const float* d_plans, const float* d_score, const float* d_budget,
                          float sigma_min, float* d_mean, float* d_sigma, int32_t* d_best, float* d_best_score) {
  if (!c) return SAG_ERR_ARG;
  if (!d_plans || !d_score || !d_mean || !d_sigma || !d_best || misaligned(d_plans, 8) || misaligned(d_score, 16) || misaligned(d_budget, 4) ||
      misaligned(d_mean, 8) || misaligned(d_sigma, 8) || misaligned(d_best, 4) || misaligned(d_best_score, 16))
    return fail(c, SAG_ERR_ARG, "sag_plan_refit_device: NULL or misaligned buffer (plans, mean, sigma 8 bytes; score, best_score 16; budget, best 4)");
  const int G = plan_groups(c, "sag_plan_refit_device", K, H);
  if (!G) return SAG_ERR_ARG;
  if (E < 1 || E > K) return fail(c, SAG_ERR_ARG, "sag_plan_refit_device: E = %d elites of K = %d candidates", E, K);
  if (!plan_scale_ok(sigma_min)) return fail(c, SAG_ERR_ARG, "sag_plan_refit_device: sigma_min = %g", (double)sigma_min);
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_plan_refit_device before sag_set_layout");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  int rc = ensure_plan_scratch(c);
  if (rc) return rc;
  hipLaunchKernelGGL(k_plan_refit, dim3(G), dim3(PLAN_REFIT_THREADS), 0, c->stream, c->N, K, H, c->rb.nu, E, d_plans,
                     reinterpret_cast<const float4*>(d_score), d_budget, sigma_min, c->d_prank, d_mean, d_sigma, d_best,
                     reinterpret_cast<float4*>(d_best_score));
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

static int plan_table_ok(sag_ctx* c, const char* who, int32_t G, int32_t H, const float* d_mean, const float* d_sigma, float sigma_init) {
  if (!d_mean || !d_sigma || misaligned(d_mean, 8) || misaligned(d_sigma, 8))
    return fail(c, SAG_ERR_ARG, "%s: NULL buffer, or one that is not 8-byte aligned", who);
  if (G < 1 || H < 1) return fail(c, SAG_ERR_ARG, "%s: G = %d, H = %d", who, G, H);
  if (!plan_scale_ok(sigma_init)) return fail(c, SAG_ERR_ARG, "%s: sigma_init = %g", who, (double)sigma_init);
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "%s before sag_set_layout", who);
  return 0;
}

int sag_plan_shift_device(sag_ctx* c, int32_t G, int32_t H, float* d_mean, float* d_sigma, float sigma_init) {
  if (!c) return SAG_ERR_ARG;
  int rc = plan_table_ok(c, "sag_plan_shift_device", G, H, d_mean, d_sigma, sigma_init);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t row = (size_t)G * c->rb.nu, total = (size_t)H * row;
  if (c->pshift_floats < total) {   // (the first call for a table of this size; a buffer in use by the stream is not freed under it)
    if (c->d_pshift) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->d_pshift); }
    c->d_pshift = nullptr; c->pshift_floats = 0;
    HIPCHK(c, hipMalloc(&c->d_pshift, total * sizeof(float)));
    c->pshift_floats = total;
  }
  hipLaunchKernelGGL(k_plan_shift, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, H, (int)row, d_mean, c->d_pshift, d_sigma, sigma_init);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(d_mean, c->d_pshift, total * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  return SAG_OK;
}

int sag_plan_clear_device(sag_ctx* c, int32_t G, int32_t H, const uint8_t* d_mask, float* d_mean, float* d_sigma, float sigma_init) {
  if (!c) return SAG_ERR_ARG;
  int rc = plan_table_ok(c, "sag_plan_clear_device", G, H, d_mean, d_sigma, sigma_init);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t total = (size_t)H * G * c->rb.nu;
  hipLaunchKernelGGL(k_plan_clear, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c->stream, H, G, c->rb.nu, d_mask, d_mean, d_sigma, sigma_init);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// ---- rollout buffer (sag_buffer.hpp) ----
int sag_append_rows_device(sag_ctx* c, const uint8_t* d_mask, int32_t row_bytes, const void* d_src, void* d_store, int32_t capacity,
                           int32_t* d_count, int32_t restart, int32_t* d_slot) {
  if (!c) return SAG_ERR_ARG;
  if (!d_mask || !d_src || !d_store || !d_count || !d_slot || d_src == d_store)
    return fail(c, SAG_ERR_ARG, "sag_append_rows_device: d_mask, d_src, d_store, d_count and d_slot must be given, d_src and d_store two buffers");
  if (row_bytes <= 0 || (row_bytes & 15)) return fail(c, SAG_ERR_ARG, "sag_append_rows_device: row_bytes %d is not a positive multiple of 16", row_bytes);
  if (misaligned(d_src, 16) || misaligned(d_store, 16)) return fail(c, SAG_ERR_ARG, "sag_append_rows_device: d_src and d_store must be 16-byte aligned");
  if (misaligned(d_count, 4) || misaligned(d_slot, 4)) return fail(c, SAG_ERR_ARG, "sag_append_rows_device: d_count and d_slot must be 4-byte aligned");
  if (capacity < 1) return fail(c, SAG_ERR_ARG, "sag_append_rows_device: capacity = %d", capacity);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (restart) HIPCHK(c, hipMemsetAsync(d_count, 0, sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(k_append_rows, dim3((c->N + WAVE - 1) / WAVE), dim3(WAVE), 0, c->stream, c->N, d_mask, row_bytes / 16,
                     reinterpret_cast<const float4*>(d_src), reinterpret_cast<float4*>(d_store), capacity, reinterpret_cast<int*>(d_count), d_slot);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_gae_device(sag_ctx* c, const sag_gae_desc* d) {
  if (!c) return SAG_ERR_ARG;
  if (!d) return fail(c, SAG_ERR_ARG, "sag_gae_device: desc is NULL");
  if (d->T < 1 || d->pitch < c->N) return fail(c, SAG_ERR_ARG, "sag_gae_device: T = %d, pitch = %d (%d envs)", d->T, d->pitch, c->N);
  if (c->N >= (1 << 28)) return fail(c, SAG_ERR_UNSUPPORTED, "sag_gae_device: %d envs (the kernel's lane offsets are 32-bit: fewer than 2^28)", c->N);
  auto unit = [](float x) { return x >= 0.0f && x <= 1.0f; };   // (false for a NaN)
  if (!unit(d->gamma) || !unit(d->lam) || !unit(d->cost_gamma) || !unit(d->cost_lam))
    return fail(c, SAG_ERR_ARG, "sag_gae_device: gamma = %g, lam = %g, cost_gamma = %g, cost_lam = %g: each in [0, 1]", (double)d->gamma,
                (double)d->lam, (double)d->cost_gamma, (double)d->cost_lam);
  if (!d->d_reward || !d->d_cost || !d->d_ended || !d->d_value || !d->d_adv || !d->d_ret)
    return fail(c, SAG_ERR_ARG, "sag_gae_device: d_reward, d_cost, d_ended, d_value, d_adv and d_ret must be given");
  const bool cost = d->d_cvalue != nullptr;
  if (cost != (d->d_cadv != nullptr) || cost != (d->d_cret != nullptr))
    return fail(c, SAG_ERR_ARG, "sag_gae_device: d_cadv and d_cret go with d_cvalue - all three or none");
  if (d->d_slot && d->capacity < 1) return fail(c, SAG_ERR_ARG, "sag_gae_device: d_slot with capacity = %d", d->capacity);
  if (misaligned(d->d_reward, 8) || misaligned(d->d_value, 4) || misaligned(d->d_cvalue, 4) || misaligned(d->d_slot, 4) ||
      misaligned(d->d_final_value, 4) || misaligned(d->d_final_cvalue, 4) || misaligned(d->d_adv, 4) || misaligned(d->d_ret, 4) ||
      misaligned(d->d_cadv, 4) || misaligned(d->d_cret, 4))
    return fail(c, SAG_ERR_ARG, "sag_gae_device: a misaligned buffer (d_reward 8 bytes; floats and ints 4)");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  GaeArgs a;
  a.N = c->N; a.T = d->T; a.pitch = d->pitch; a.capacity = d->capacity;
  a.gamma = d->gamma; a.gl = d->gamma * d->lam; a.cgamma = d->cost_gamma; a.cgl = d->cost_gamma * d->cost_lam;
  a.reward = d->d_reward; a.cost = d->d_cost; a.ended = d->d_ended; a.value = d->d_value; a.cvalue = d->d_cvalue;
  a.slot = d->d_slot; a.final_value = d->d_final_value; a.final_cvalue = cost ? d->d_final_cvalue : nullptr;
  a.adv = d->d_adv; a.ret = d->d_ret; a.cadv = d->d_cadv; a.cret = d->d_cret;
  const bool slot = a.slot && (a.final_value || a.final_cvalue);   // (slots without final values change nothing: not loaded)
  const dim3 grid((c->N + WAVE - 1) / WAVE), block(WAVE);
  if (cost && slot) hipLaunchKernelGGL((k_gae<true, true>), grid, block, 0, c->stream, a);
  else if (cost) hipLaunchKernelGGL((k_gae<true, false>), grid, block, 0, c->stream, a);
  else if (slot) hipLaunchKernelGGL((k_gae<false, true>), grid, block, 0, c->stream, a);
  else hipLaunchKernelGGL((k_gae<false, false>), grid, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// ---- actor-critic MLP (sag_policy.hpp) ----
namespace {

// the table and clip of the _norm entry points (table == nullptr: the plain ones)
int norm_args_ok(sag_ctx* c, const char* who, const float* d_table, float clip) {
  if (!d_table || misaligned(d_table, 16)) return fail(c, SAG_ERR_ARG, "%s: d_table is NULL or not 16-byte aligned", who);
  if (!(clip > 0.0f)) return fail(c, SAG_ERR_ARG, "%s: clip = %g is not above 0", who, (double)clip);
  return 0;
}

int policy_forward(sag_ctx* c, const char* who, const sag_policy_desc* d, const float* d_table, float clip) {
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_params || !d->d_obs) return fail(c, SAG_ERR_ARG, "%s: d_params and d_obs must be given", who);
  if (misaligned(d->d_obs, 16) || misaligned(d->d_params, 4) || misaligned(d->d_actions, 4) || misaligned(d->d_logp, 4) ||
      misaligned(d->d_value, 4) || misaligned(d->d_cvalue, 4))
    return fail(c, SAG_ERR_ARG, "%s: a misaligned buffer (d_obs 16 bytes; parameters and outputs 4)", who);
  if (d->hidden < 32 || d->hidden > 32 * POLICY_MAX_TILES || (d->hidden & 31))
    return fail(c, SAG_ERR_ARG, "%s: hidden = %d is not a multiple of 32 in 32 ... %d", who, d->hidden, 32 * POLICY_MAX_TILES);
  if (d->activation != SAG_POLICY_RELU && d->activation != SAG_POLICY_TANH)
    return fail(c, SAG_ERR_ARG, "%s: activation = %d", who, d->activation);
  if (d->flags & ~SAG_POLICY_MEAN) return fail(c, SAG_ERR_ARG, "%s: unknown flag bits 0x%x", who, d->flags & ~SAG_POLICY_MEAN);
  if (d->obs_pitch < c->rb.obs_dim || (d->obs_pitch & 3))
    return fail(c, SAG_ERR_ARG, "%s: obs_pitch = %d (rows of %d floats, a multiple of 4)", who, d->obs_pitch, c->rb.obs_dim);
  if (d->n_rows < 1) return fail(c, SAG_ERR_ARG, "%s: n_rows = %d", who, d->n_rows);
  if (!std::isfinite(d->logp_const)) return fail(c, SAG_ERR_ARG, "%s: logp_const is not finite", who);
  if (c->rb.obs_dim > POLICY_MAX_OBS || (c->rb.obs_dim & 3) || c->rb.nu + 2 > 16)
    return fail(c, SAG_ERR_UNSUPPORTED, "%s: obs_dim = %d, nu = %d", who, c->rb.obs_dim, c->rb.nu);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  PolicyNormArgs a;
  a.n_rows = d->n_rows; a.obs_dim = c->rb.obs_dim; a.nu = c->rb.nu; a.activation = d->activation;
  a.mean_only = (d->flags & SAG_POLICY_MEAN) != 0; a.obs_pitch = d->obs_pitch; a.lds_pitch = policy_lds_pitch(c->rb.obs_dim);
  const size_t lds = (size_t)POLICY_ROWS * a.lds_pitch * sizeof(float);
  a.id0 = (uint32_t)c->env_id0 + d->row0; a.draw = d->draw;
  a.k0 = (uint32_t)(c->cfg.seed & 0xffffffffu); a.k1 = (uint32_t)(c->cfg.seed >> 32);
  a.logp_const = d->logp_const; a.params = d->d_params; a.obs = d->d_obs;
  a.actions = d->d_actions; a.logp = d->d_logp; a.value = d->d_value; a.cvalue = d->d_cvalue;
  a.table = d_table; a.obs_clip = clip;
  const PolicyArgs& plain = a;
  const dim3 grid((unsigned)(((size_t)d->n_rows + POLICY_ROWS - 1) / POLICY_ROWS)), block(WAVE);
  if (!d_table) {
    switch (d->hidden / 32) {
      case 1: hipLaunchKernelGGL((k_policy_forward<1>), grid, block, lds, c->stream, plain); break;
      case 2: hipLaunchKernelGGL((k_policy_forward<2>), grid, block, lds, c->stream, plain); break;
      case 3: hipLaunchKernelGGL((k_policy_forward<3>), grid, block, lds, c->stream, plain); break;
      case 4: hipLaunchKernelGGL((k_policy_forward<4>), grid, block, lds, c->stream, plain); break;
      case 5: hipLaunchKernelGGL((k_policy_forward<5>), grid, block, lds, c->stream, plain); break;
      case 6: hipLaunchKernelGGL((k_policy_forward<6>), grid, block, lds, c->stream, plain); break;
      case 7: hipLaunchKernelGGL((k_policy_forward<7>), grid, block, lds, c->stream, plain); break;
      default: hipLaunchKernelGGL((k_policy_forward<8>), grid, block, lds, c->stream, plain); break;
    }
  } else {
    switch (d->hidden / 32) {
      case 1: hipLaunchKernelGGL((k_policy_forward<1, true>), grid, block, lds, c->stream, a); break;
      case 2: hipLaunchKernelGGL((k_policy_forward<2, true>), grid, block, lds, c->stream, a); break;
      case 3: hipLaunchKernelGGL((k_policy_forward<3, true>), grid, block, lds, c->stream, a); break;
      case 4: hipLaunchKernelGGL((k_policy_forward<4, true>), grid, block, lds, c->stream, a); break;
      case 5: hipLaunchKernelGGL((k_policy_forward<5, true>), grid, block, lds, c->stream, a); break;
      case 6: hipLaunchKernelGGL((k_policy_forward<6, true>), grid, block, lds, c->stream, a); break;
      case 7: hipLaunchKernelGGL((k_policy_forward<7, true>), grid, block, lds, c->stream, a); break;
      default: hipLaunchKernelGGL((k_policy_forward<8, true>), grid, block, lds, c->stream, a); break;
    }
  }
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

}  // namespace

int sag_policy_forward_device(sag_ctx* c, const sag_policy_desc* d) {
  if (!c) return SAG_ERR_ARG;
  return policy_forward(c, "sag_policy_forward_device", d, nullptr, 0.0f);
}

int sag_policy_forward_norm_device(sag_ctx* c, const sag_policy_desc* d, const float* d_table, float clip) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_policy_forward_norm_device";
  if (int rc = norm_args_ok(c, who, d_table, clip)) return rc;
  return policy_forward(c, who, d, d_table, clip);
}

// ---- the update (sag_policy_grad.hpp) ----
namespace {

// d_rows == nullptr: the contiguous entry points; otherwise the batch is the n_index entries of the list
int policy_backward(sag_ctx* c, const char* who, const sag_policy_grad_desc* d, const float* d_table, float obs_clip,
                    const int32_t* d_rows = nullptr, int32_t n_index = 0) {
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_params || !d->d_obs || !d->d_actions || !d->d_logp_old || !d->d_adv || !d->d_ret || !d->d_grad)
    return fail(c, SAG_ERR_ARG, "%s: d_params, d_obs, d_actions, d_logp_old, d_adv, d_ret and d_grad must be given", who);
  if (misaligned(d->d_obs, 16) || misaligned(d->d_params, 4) || misaligned(d->d_actions, 4) || misaligned(d->d_logp_old, 4) ||
      misaligned(d->d_adv, 4) || misaligned(d->d_ret, 4) || misaligned(d->d_cadv, 4) || misaligned(d->d_cret, 4) || misaligned(d->d_grad, 4))
    return fail(c, SAG_ERR_ARG, "%s: a misaligned buffer (d_obs 16 bytes; the others 4)", who);
  if (d->hidden < 32 || d->hidden > 32 * POLICY_MAX_TILES || (d->hidden & 31))
    return fail(c, SAG_ERR_ARG, "%s: hidden = %d is not a multiple of 32 in 32 ... %d", who, d->hidden, 32 * POLICY_MAX_TILES);
  if (d->activation != SAG_POLICY_RELU && d->activation != SAG_POLICY_TANH) return fail(c, SAG_ERR_ARG, "%s: activation = %d", who, d->activation);
  if (d->flags & ~SAG_POLICY_GRAD_ACCUMULATE) return fail(c, SAG_ERR_ARG, "%s: unknown flag bits 0x%x", who, d->flags & ~SAG_POLICY_GRAD_ACCUMULATE);
  if (d->obs_pitch < c->rb.obs_dim || (d->obs_pitch & 3))
    return fail(c, SAG_ERR_ARG, "%s: obs_pitch = %d (rows of %d floats, a multiple of 4)", who, d->obs_pitch, c->rb.obs_dim);
  if (d->n_rows < 1 || d->n_planes < 1 || d->pitch < d->n_rows)
    return fail(c, SAG_ERR_ARG, "%s: n_rows = %d, n_planes = %d, pitch = %d", who, d->n_rows, d->n_planes, d->pitch);
  if (d->max_blocks < 0) return fail(c, SAG_ERR_ARG, "%s: max_blocks = %d", who, d->max_blocks);
  if (!(d->clip > 0.0f && d->clip < 1.0f)) return fail(c, SAG_ERR_ARG, "%s: clip = %g is not inside (0, 1)", who, (double)d->clip);
  for (float x : {d->vf_coef, d->cvf_coef, d->ent_coef, d->adv_mul, d->adv_sub, d->cadv_mul, d->cadv_sub, d->scale})
    if (!std::isfinite(x)) return fail(c, SAG_ERR_ARG, "%s: a coefficient or scale that is not finite", who);
  if (c->rb.obs_dim > POLICY_MAX_OBS || (c->rb.obs_dim & 3) || c->rb.nu + 2 > 14)
    return fail(c, SAG_ERR_UNSUPPORTED, "%s: obs_dim = %d, nu = %d", who, c->rb.obs_dim, c->rb.nu);
  if (d->hidden > 32 * PGRAD_MAX_TILES)
    return fail(c, SAG_ERR_UNSUPPORTED, "%s: hidden = %d: the backward pass is built for hidden <= %d", who, d->hidden, 32 * PGRAD_MAX_TILES);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int od = c->rb.obs_dim, nu = c->rb.nu, H = d->hidden, NO = nu + 2;
  PolicyGradRowsArgs a;
  a.limit = (int64_t)d->n_planes * d->n_rows;
  a.total = d_rows ? (int64_t)n_index : a.limit;
  a.rows = d_rows;
  a.n_rows = d->n_rows; a.pitch = d->pitch; a.obs_dim = od; a.nu = nu; a.activation = d->activation; a.obs_pitch = d->obs_pitch;
  a.n_params = od * H + H + H * H + H + H * NO + NO + nu;
  a.clip = d->clip; a.vf = d->vf_coef; a.cvf = d->cvf_coef; a.ent = d->ent_coef;
  a.adv_mul = d->adv_mul; a.adv_sub = d->adv_sub; a.cadv_mul = d->cadv_mul; a.cadv_sub = d->cadv_sub;
  a.params = d->d_params; a.obs = d->d_obs; a.actions = d->d_actions; a.logp_old = d->d_logp_old; a.adv = d->d_adv; a.ret = d->d_ret;
  a.cadv = d->d_cadv; a.cret = d->d_cret;
  a.table = d_table; a.obs_clip = obs_clip;
  const int grid = pgrad_grid(a.total, d->max_blocks), words = a.n_params + PGRAD_STATS;
  const size_t need = (size_t)grid * words;
  if (c->pgrad_floats < need) {   // (a workspace in use by the stream is not freed under it)
    if (c->d_pgrad) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->d_pgrad); }
    c->d_pgrad = nullptr; c->pgrad_floats = 0;
    HIPCHK(c, hipMalloc(&c->d_pgrad, need * sizeof(float)));
    c->pgrad_floats = need;
  }
  a.part = c->d_pgrad;
  const PolicyGradArgs& plain = a;
  const PolicyGradNormArgs& norm = a;
  const size_t lds = pgrad_lds_floats(od, H) * sizeof(float);
  const dim3 g((unsigned)grid), block(PGRAD_THREADS);
  if (d_rows) {
    const size_t ldr = lds + PGRAD_ROWS_LDS_FLOATS * sizeof(float);
    if (!d_table) {
      switch (H / 32) {
        case 1: hipLaunchKernelGGL((k_policy_backward<1, false, true>), g, block, ldr, c->stream, a); break;
        case 2: hipLaunchKernelGGL((k_policy_backward<2, false, true>), g, block, ldr, c->stream, a); break;
        case 3: hipLaunchKernelGGL((k_policy_backward<3, false, true>), g, block, ldr, c->stream, a); break;
        default: hipLaunchKernelGGL((k_policy_backward<4, false, true>), g, block, ldr, c->stream, a); break;
      }
    } else {
      switch (H / 32) {
        case 1: hipLaunchKernelGGL((k_policy_backward<1, true, true>), g, block, ldr, c->stream, a); break;
        case 2: hipLaunchKernelGGL((k_policy_backward<2, true, true>), g, block, ldr, c->stream, a); break;
        case 3: hipLaunchKernelGGL((k_policy_backward<3, true, true>), g, block, ldr, c->stream, a); break;
        default: hipLaunchKernelGGL((k_policy_backward<4, true, true>), g, block, ldr, c->stream, a); break;
      }
    }
  } else if (!d_table) {
    switch (H / 32) {
      case 1: hipLaunchKernelGGL((k_policy_backward<1>), g, block, lds, c->stream, plain); break;
      case 2: hipLaunchKernelGGL((k_policy_backward<2>), g, block, lds, c->stream, plain); break;
      case 3: hipLaunchKernelGGL((k_policy_backward<3>), g, block, lds, c->stream, plain); break;
      default: hipLaunchKernelGGL((k_policy_backward<4>), g, block, lds, c->stream, plain); break;
    }
  } else {
    switch (H / 32) {
      case 1: hipLaunchKernelGGL((k_policy_backward<1, true>), g, block, lds, c->stream, norm); break;
      case 2: hipLaunchKernelGGL((k_policy_backward<2, true>), g, block, lds, c->stream, norm); break;
      case 3: hipLaunchKernelGGL((k_policy_backward<3, true>), g, block, lds, c->stream, norm); break;
      default: hipLaunchKernelGGL((k_policy_backward<4, true>), g, block, lds, c->stream, norm); break;
    }
  }
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_policy_grad_reduce, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->stream, c->d_pgrad, grid, words, d->scale,
                     (d->flags & SAG_POLICY_GRAD_ACCUMULATE) != 0, d->d_grad);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

}  // namespace

int sag_policy_backward_device(sag_ctx* c, const sag_policy_grad_desc* d) {
  if (!c) return SAG_ERR_ARG;
  return policy_backward(c, "sag_policy_backward_device", d, nullptr, 0.0f);
}

int sag_policy_backward_norm_device(sag_ctx* c, const sag_policy_grad_desc* d, const float* d_table, float clip) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_policy_backward_norm_device";
  if (int rc = norm_args_ok(c, who, d_table, clip)) return rc;
  return policy_backward(c, who, d, d_table, clip);
}

int sag_policy_backward_rows_device(sag_ctx* c, const sag_policy_grad_desc* d, const int32_t* d_rows, int32_t n_index, const float* d_table,
                                    float obs_clip) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_policy_backward_rows_device";
  if (!d_rows || misaligned(d_rows, 4)) return fail(c, SAG_ERR_ARG, "%s: d_rows is NULL or not 4-byte aligned", who);
  if (n_index < 1) return fail(c, SAG_ERR_ARG, "%s: n_index = %d", who, n_index);
  if (d_table) {
    if (int rc = norm_args_ok(c, who, d_table, obs_clip)) return rc;
    if (!std::isfinite(obs_clip)) return fail(c, SAG_ERR_ARG, "%s: obs_clip = %g is not finite", who, (double)obs_clip);
  }
  return policy_backward(c, who, d, d_table, d_table ? obs_clip : 0.0f, d_rows, n_index);
}

// ---- the row list of a shuffled epoch (sag_shuffle.hpp) ----
int sag_permutation_device(sag_ctx* c, int32_t n, uint32_t draw, int32_t* d_index) {
  if (!c) return SAG_ERR_ARG;
  if (!d_index || misaligned(d_index, 4)) return fail(c, SAG_ERR_ARG, "sag_permutation_device: d_index is NULL or not 4-byte aligned");
  if (n < 1) return fail(c, SAG_ERR_ARG, "sag_permutation_device: n = %d", n);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(k_permutation, dim3((unsigned)(((uint32_t)n + SHUFFLE_THREADS - 1) / SHUFFLE_THREADS)), dim3(SHUFFLE_THREADS), 0, c->stream,
                     (uint32_t)n, shuffle_bits(n), draw, (uint32_t)(c->cfg.seed & 0xffffffffu), (uint32_t)(c->cfg.seed >> 32), d_index);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_adam_device(sag_ctx* c, const sag_adam_desc* d) {
  if (!c) return SAG_ERR_ARG;
  if (!d) return fail(c, SAG_ERR_ARG, "sag_adam_device: desc is NULL");
  if (!d->d_param || !d->d_grad || !d->d_m || !d->d_v) return fail(c, SAG_ERR_ARG, "sag_adam_device: d_param, d_grad, d_m and d_v must be given");
  if (misaligned(d->d_param, 4) || misaligned(d->d_grad, 4) || misaligned(d->d_m, 4) || misaligned(d->d_v, 4))
    return fail(c, SAG_ERR_ARG, "sag_adam_device: a buffer that is not 4-byte aligned");
  if (d->n < 1 || d->clamp_first < 0 || d->clamp_first > d->n) return fail(c, SAG_ERR_ARG, "sag_adam_device: n = %d, clamp_first = %d", d->n, d->clamp_first);
  auto beta = [](float x) { return x >= 0.0f && x < 1.0f; };   // (false for a NaN)
  if (!beta(d->beta1) || !beta(d->beta2)) return fail(c, SAG_ERR_ARG, "sag_adam_device: beta1 = %g, beta2 = %g: each in [0, 1)", (double)d->beta1, (double)d->beta2);
  if (!(d->eps > 0.0f) || !std::isfinite(d->eps)) return fail(c, SAG_ERR_ARG, "sag_adam_device: eps = %g", (double)d->eps);
  if (!std::isfinite(d->step) || !std::isfinite(d->clamp_lo)) return fail(c, SAG_ERR_ARG, "sag_adam_device: step = %g, clamp_lo = %g", (double)d->step, (double)d->clamp_lo);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  AdamArgs a;
  a.n = d->n; a.clamp_first = d->clamp_first; a.beta1 = d->beta1; a.beta2 = d->beta2;
  a.omb1 = 1.0f - d->beta1; a.omb2 = 1.0f - d->beta2; a.eps = d->eps; a.step = d->step; a.clamp_lo = d->clamp_lo;
  a.param = d->d_param; a.grad = d->d_grad; a.m = d->d_m; a.v = d->d_v;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((d->n + 255) / 256)), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// ---- moments, the mixed advantage, the multiplier, the clip (sag_learner.hpp) ----
namespace {

// the partials of `grid` blocks: [grid] f32 sums, then [grid] i32 counts (a workspace in use by the stream is not freed under it)
int ensure_lpart(sag_ctx* c, int grid) {
  if (c->lpart_blocks >= (size_t)grid) return 0;
  if (c->d_lpart) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->d_lpart); }
  c->d_lpart = nullptr; c->lpart_blocks = 0;
  HIPCHK(c, hipMalloc(&c->d_lpart, (size_t)grid * 2 * sizeof(float)));
  c->lpart_blocks = (size_t)grid;
  return 0;
}

bool span_ok(int32_t n_rows, int32_t n_planes, int32_t pitch) {
  return n_rows >= 1 && n_planes >= 1 && pitch >= n_rows && (int64_t)n_planes * n_rows < ((int64_t)1 << 31);
}

}  // namespace

int sag_moments_device(sag_ctx* c, const sag_moments_desc* d) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_moments_device";
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_x || !d->d_out) return fail(c, SAG_ERR_ARG, "%s: d_x and d_out must be given", who);
  if (misaligned(d->d_x, 4) || misaligned(d->d_out, 4)) return fail(c, SAG_ERR_ARG, "%s: d_x or d_out is not 4-byte aligned", who);
  if (!span_ok(d->n_rows, d->n_planes, d->pitch) || d->stride < 1)
    return fail(c, SAG_ERR_ARG, "%s: n_rows = %d, n_planes = %d, pitch = %d, stride = %d (n_planes * n_rows below 2^31)", who, d->n_rows,
                d->n_planes, d->pitch, d->stride);
  if (d->max_blocks < 0) return fail(c, SAG_ERR_ARG, "%s: max_blocks = %d", who, d->max_blocks);
  if (!std::isfinite(d->eps) || d->eps < 0.0f) return fail(c, SAG_ERR_ARG, "%s: eps = %g", who, (double)d->eps);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int64_t total = (int64_t)d->n_planes * d->n_rows;
  const int grid = learn_grid(total, d->max_blocks);
  if (int rc = ensure_lpart(c, grid)) return rc;
  LearnPartialArgs a;
  a.span.total = (uint32_t)total; a.span.n_rows = (uint32_t)d->n_rows; a.span.pitch = (uint32_t)d->pitch; a.span.stride = (uint32_t)d->stride;
  a.x_mis = (uint32_t)((reinterpret_cast<uintptr_t>(d->d_x) >> 2) & 3); a.m_mis = (uint32_t)(reinterpret_cast<uintptr_t>(d->d_mask) & 3);
  a.x = d->d_x; a.mask = d->d_mask; a.mom = d->d_out;
  a.part_sum = c->d_lpart; a.part_cnt = reinterpret_cast<int32_t*>(c->d_lpart + grid);
  const dim3 g((unsigned)grid), block(LEARN_THREADS);
  hipLaunchKernelGGL((k_learn_partial<0>), g, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_moments_final, dim3(1), block, 0, c->stream, a.part_sum, a.part_cnt, grid, 0, d->eps, d->d_out);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL((k_learn_partial<1>), g, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_moments_final, dim3(1), block, 0, c->stream, a.part_sum, a.part_cnt, grid, 1, d->eps, d->d_out);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_advantage_mix_device(sag_ctx* c, const sag_advantage_mix_desc* d) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_advantage_mix_device";
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_adv || !d->d_out) return fail(c, SAG_ERR_ARG, "%s: d_adv and d_out must be given", who);
  if (d->adv_mode < 0 || d->adv_mode > 2 || d->cadv_mode < 0 || d->cadv_mode > 2)
    return fail(c, SAG_ERR_ARG, "%s: adv_mode = %d, cadv_mode = %d: each 0 (raw), 1 (centred) or 2 (standardised)", who, d->adv_mode, d->cadv_mode);
  if ((d->adv_mode > 0 && !d->d_adv_mom) || (d->d_cadv && d->cadv_mode > 0 && !d->d_cadv_mom))
    return fail(c, SAG_ERR_ARG, "%s: a mode above 0 needs its moments array", who);
  if (misaligned(d->d_adv, 4) || misaligned(d->d_cadv, 4) || misaligned(d->d_adv_mom, 4) || misaligned(d->d_cadv_mom, 4) ||
      misaligned(d->d_lambda, 4) || misaligned(d->d_out, 4))
    return fail(c, SAG_ERR_ARG, "%s: a buffer that is not 4-byte aligned", who);
  if (!span_ok(d->n_rows, d->n_planes, d->pitch))
    return fail(c, SAG_ERR_ARG, "%s: n_rows = %d, n_planes = %d, pitch = %d (n_planes * n_rows below 2^31)", who, d->n_rows, d->n_planes, d->pitch);
  if (!std::isfinite(d->cost_weight)) return fail(c, SAG_ERR_ARG, "%s: cost_weight is not finite", who);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int64_t total = (int64_t)d->n_planes * d->n_rows;
  MixArgs a;
  a.span.total = (uint32_t)total; a.span.n_rows = (uint32_t)d->n_rows; a.span.pitch = (uint32_t)d->pitch; a.span.stride = 1;
  a.mis = (misaligned(d->d_adv, 16) || misaligned(d->d_cadv, 16) || misaligned(d->d_out, 16)) ? 1u : 0u;
  a.adv_mode = d->adv_mode; a.cadv_mode = d->cadv_mode; a.cost_weight = d->cost_weight;
  a.adv = d->d_adv; a.cadv = d->d_cadv; a.adv_mom = d->d_adv_mom; a.cadv_mom = d->d_cadv_mom; a.lambda = d->d_lambda; a.out = d->d_out;
  const int64_t quads = (total + 3) / 4;
  hipLaunchKernelGGL(k_advantage_mix, dim3((unsigned)((quads + LEARN_THREADS - 1) / LEARN_THREADS)), dim3(LEARN_THREADS), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_lagrange_device(sag_ctx* c, const sag_lagrange_desc* d) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_lagrange_device";
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_mom || !d->d_state) return fail(c, SAG_ERR_ARG, "%s: d_mom and d_state must be given", who);
  if (misaligned(d->d_mom, 4) || misaligned(d->d_state, 4)) return fail(c, SAG_ERR_ARG, "%s: d_mom or d_state is not 4-byte aligned", who);
  if (!std::isfinite(d->lr) || !std::isfinite(d->budget) || d->lr < 0.0f) return fail(c, SAG_ERR_ARG, "%s: lr = %g, budget = %g", who, (double)d->lr, (double)d->budget);
  if (!(d->lambda_max >= 0.0f)) return fail(c, SAG_ERR_ARG, "%s: lambda_max = %g", who, (double)d->lambda_max);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(k_lagrange, dim3(1), dim3(WAVE), 0, c->stream, d->d_mom, d->lr, d->budget, d->lambda_max, d->d_state);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_grad_clip_device(sag_ctx* c, const sag_grad_clip_desc* d) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_grad_clip_device";
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (!d->d_grad || !d->d_out) return fail(c, SAG_ERR_ARG, "%s: d_grad and d_out must be given", who);
  if (misaligned(d->d_grad, 4) || misaligned(d->d_out, 4)) return fail(c, SAG_ERR_ARG, "%s: d_grad or d_out is not 4-byte aligned", who);
  if (d->n < 1) return fail(c, SAG_ERR_ARG, "%s: n = %d", who, d->n);
  if (d->max_blocks < 0) return fail(c, SAG_ERR_ARG, "%s: max_blocks = %d", who, d->max_blocks);
  if (!std::isfinite(d->max_norm) || d->max_norm < 0.0f) return fail(c, SAG_ERR_ARG, "%s: max_norm = %g", who, (double)d->max_norm);
  const uintptr_t g0 = reinterpret_cast<uintptr_t>(d->d_grad), o0 = reinterpret_cast<uintptr_t>(d->d_out);
  if (o0 + 2 * sizeof(float) > g0 && o0 < g0 + (size_t)d->n * sizeof(float)) return fail(c, SAG_ERR_ARG, "%s: d_out lies inside d_grad[0 ... n)", who);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const int grid = learn_grid(d->n, d->max_blocks);
  if (int rc = ensure_lpart(c, grid)) return rc;
  LearnPartialArgs a;
  a.span.total = (uint32_t)d->n; a.span.n_rows = (uint32_t)d->n; a.span.pitch = (uint32_t)d->n; a.span.stride = 1;
  a.x_mis = (uint32_t)((reinterpret_cast<uintptr_t>(d->d_grad) >> 2) & 3); a.m_mis = 0;
  a.x = d->d_grad; a.mask = nullptr; a.mom = nullptr;
  a.part_sum = c->d_lpart; a.part_cnt = reinterpret_cast<int32_t*>(c->d_lpart + grid);
  const dim3 g((unsigned)grid), block(LEARN_THREADS);
  hipLaunchKernelGGL((k_learn_partial<2>), g, block, 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_grad_clip_scale, g, block, 0, c->stream, a.part_sum, grid, d->max_norm, (uint32_t)d->n, d->d_grad, d->d_out);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

// ---- observation statistics and the table (sag_obs_norm.hpp) ----
int sag_obs_stats_device(sag_ctx* c, const sag_obs_stats_desc* d) {
  if (!c) return SAG_ERR_ARG;
  const char* who = "sag_obs_stats_device";
  if (!d) return fail(c, SAG_ERR_ARG, "%s: desc is NULL", who);
  if (d->flags & ~SAG_OBS_STATS_TABLE_ONLY) return fail(c, SAG_ERR_ARG, "%s: unknown flag bits 0x%x", who, d->flags & ~SAG_OBS_STATS_TABLE_ONLY);
  const bool table_only = (d->flags & SAG_OBS_STATS_TABLE_ONLY) != 0;
  if (!d->d_state || !d->d_table) return fail(c, SAG_ERR_ARG, "%s: d_state and d_table must be given", who);
  if (misaligned(d->d_state, 8) || misaligned(d->d_table, 16)) return fail(c, SAG_ERR_ARG, "%s: d_state is not 8-byte or d_table not 16-byte aligned", who);
  if (!std::isfinite(d->eps) || !(d->eps > 0.0f)) return fail(c, SAG_ERR_ARG, "%s: eps = %g", who, (double)d->eps);
  const int od = c->rb.obs_dim;
  if (!table_only) {
    if (!d->d_obs) return fail(c, SAG_ERR_ARG, "%s: d_obs is NULL without SAG_OBS_STATS_TABLE_ONLY", who);
    if (misaligned(d->d_obs, 16)) return fail(c, SAG_ERR_ARG, "%s: d_obs is not 16-byte aligned", who);
    if (!span_ok(d->n_rows, d->n_planes, d->pitch))
      return fail(c, SAG_ERR_ARG, "%s: n_rows = %d, n_planes = %d, pitch = %d (n_planes * n_rows below 2^31)", who, d->n_rows, d->n_planes, d->pitch);
    if (d->obs_pitch < od || (d->obs_pitch & 3))
      return fail(c, SAG_ERR_ARG, "%s: obs_pitch = %d (rows of %d floats, a multiple of 4)", who, d->obs_pitch, od);
    if (d->max_blocks < 0) return fail(c, SAG_ERR_ARG, "%s: max_blocks = %d", who, d->max_blocks);
  }
  if (od > OBSN_MAX_OBS || (od & 3)) return fail(c, SAG_ERR_UNSUPPORTED, "%s: obs_dim = %d", who, od);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (!c->d_obsn) HIPCHK(c, hipMalloc(&c->d_obsn, obsn_ws_bytes(OBSN_MAX_BLOCKS, OBSN_MAX_OBS)));
  double* ws_mean = static_cast<double*>(c->d_obsn);
  float* ws_shift = reinterpret_cast<float*>(ws_mean + OBSN_MAX_OBS);
  float* ws_part = ws_shift + OBSN_MAX_OBS;
  ObsMergeArgs m;
  m.n_blocks = 0; m.obs_dim = od; m.table_only = table_only; m.eps = d->eps; m.n_b = 0.0;
  m.part = ws_part; m.mean_b = ws_mean; m.shift = ws_shift; m.state = d->d_state; m.table = d->d_table;
  const dim3 block(OBSN_THREADS);
  if (!table_only) {
    const int64_t total = (int64_t)d->n_planes * d->n_rows;
    const int grid = obsn_grid(total, d->max_blocks);
    ObsStatsArgs a;
    a.total = (uint32_t)total; a.n_rows = (uint32_t)d->n_rows; a.pitch = (uint32_t)d->pitch; a.obs_pitch = (uint32_t)d->obs_pitch;
    a.obs_dim = od; a.obs = d->d_obs; a.shift = ws_shift; a.part = ws_part;
    m.n_blocks = grid; m.n_b = (double)total;
    const dim3 g((unsigned)grid);
    hipLaunchKernelGGL((k_obs_partial<0>), g, block, 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_obs_mean, dim3(1), block, 0, c->stream, ws_part, grid, od, m.n_b, ws_mean, ws_shift);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL((k_obs_partial<1>), g, block, 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_obs_merge, dim3(1), block, 0, c->stream, m);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_step_device(sag_ctx* c, const float* d_actions, const float* d_noise, int32_t nstep, float* d_obs,
                    float* d_reward, uint8_t* d_cost, uint8_t* d_done, uint8_t* d_goal_met) {
  if (!c) return SAG_ERR_ARG;
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_step before sag_set_layout");
  if (!d_actions) return fail(c, SAG_ERR_ARG, "actions is NULL");
  return launch_step(c, d_actions, d_noise, nullptr, 0, nstep, d_obs, d_reward, d_cost, d_done, d_goal_met,
                     nullptr, 0);
}

int sag_wait(sag_ctx* c) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_set_seed(sag_ctx* c, uint64_t seed) {
  if (!c) return SAG_ERR_ARG;
  c->cfg.seed = seed;   // read by the next launch (StepArgs::key0/1)
  return SAG_OK;
}

int sag_step(sag_ctx* c, const float* actions, const float* noise, const uint32_t* tape, int32_t tape_len,
             int32_t nstep, float* obs, float* reward, uint8_t* cost, uint8_t* done, uint8_t* goal_met,
             int32_t* tape_used) {
  if (!c) return SAG_ERR_ARG;
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_step before sag_set_layout");
  if (!actions) return fail(c, SAG_ERR_ARG, "actions is NULL");
  if (tape && tape_len <= 0) return fail(c, SAG_ERR_ARG, "tape without tape_len");
  const size_t N = (size_t)c->N, nu = (size_t)c->rb.nu, od = (size_t)c->rb.obs_dim;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(c->d_act, actions, N * nu * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (noise) HIPCHK(c, hipMemcpyAsync(c->d_noise, noise, N * nu * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (tape) {
    size_t need = N * (size_t)tape_len * sizeof(uint32_t);
    if (c->tape_cap < need) {
      if (c->d_tape) (void)hipFree(c->d_tape);
      c->d_tape = nullptr; c->tape_cap = 0;
      HIPCHK(c, hipMalloc(&c->d_tape, need));
      c->tape_cap = need;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_tape, tape, need, hipMemcpyHostToDevice, c->stream));
  }
  int rc = launch_step(c, c->d_act, noise ? c->d_noise : nullptr, tape ? c->d_tape : nullptr, tape_len, nstep,
                       obs ? c->d_obs : nullptr, reward ? c->d_rew : nullptr, cost ? c->d_cost : nullptr,
                       done ? c->d_done : nullptr, goal_met ? c->d_met : nullptr,
                       tape_used ? c->d_used : nullptr, 0);
  if (rc) return rc;
  if (obs) HIPCHK(c, hipMemcpyAsync(obs, c->d_obs, N * od * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (reward) HIPCHK(c, hipMemcpyAsync(reward, c->d_rew, N * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (cost) HIPCHK(c, hipMemcpyAsync(cost, c->d_cost, N, hipMemcpyDeviceToHost, c->stream));
  if (done) HIPCHK(c, hipMemcpyAsync(done, c->d_done, N, hipMemcpyDeviceToHost, c->stream));
  if (goal_met) HIPCHK(c, hipMemcpyAsync(goal_met, c->d_met, N, hipMemcpyDeviceToHost, c->stream));
  if (tape_used) HIPCHK(c, hipMemcpyAsync(tape_used, c->d_used, N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_set_ext_contacts(sag_ctx* c, const int32_t* cost_contacts, const uint32_t* btn_mask) {
  if (!c) return SAG_ERR_ARG;
  if (!cost_contacts && !btn_mask) { c->ext_pending = false; return SAG_OK; }
  if (!cost_contacts || !btn_mask) return fail(c, SAG_ERR_ARG, "sag_set_ext_contacts: both arrays or neither");
  const size_t N = (size_t)c->N;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  if (!c->d_ext_cc) {
    HIPCHK(c, hipMalloc(&c->d_ext_cc, N * sizeof(int32_t)));
    HIPCHK(c, hipMalloc(&c->d_ext_btn, N * sizeof(uint32_t)));
  }
  HIPCHK(c, hipMemcpyAsync(c->d_ext_cc, cost_contacts, N * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_ext_btn, btn_mask, N * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));   // the host arrays are the caller's: do not keep reading them
  c->ext_pending = true;
  return SAG_OK;
}

int sag_observe(sag_ctx* c, float* obs) {
  if (!c || !obs) return SAG_ERR_ARG;
  if (!c->have_layout) return fail(c, SAG_ERR_STATE, "sag_observe before sag_set_layout");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  int rc = launch_step(c, nullptr, nullptr, nullptr, 0, 0, c->d_obs, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(obs, c->d_obs, (size_t)c->N * c->rb.obs_dim * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_lidar_cost(sag_ctx* c, int32_t n, int32_t K, const float* robot, const float* points,
                   const uint8_t* group, float hazard_size, float* lidar, int32_t* bins, uint8_t* cost) {
  if (!c) return SAG_ERR_ARG;
  if (n <= 0 || K < 0 || !robot || (K > 0 && (!points || !group)) || !lidar || !cost)
    return fail(c, SAG_ERR_ARG, "bad sag_lidar_cost arguments");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };   // every buffer 256-byte aligned (vector loads)
  const size_t b_robot = up((size_t)n * 3 * 4), b_pts = up((size_t)n * K * 2 * 4), b_grp = up((size_t)n * K),
               b_lid = up((size_t)n * 48 * 4), b_bins = up((size_t)n * K * 4), b_cost = up((size_t)n);
  int rc = ensure_scratch(c, b_robot + b_pts + b_grp + b_lid + b_bins + b_cost + 256);
  if (rc) return rc;
  char* base = (char*)c->scratch;
  float* d_robot = (float*)base; base += b_robot;
  float* d_pts = (float*)base; base += b_pts;
  float* d_lid = (float*)base; base += b_lid;
  int32_t* d_bins = (int32_t*)base; base += b_bins;
  uint8_t* d_grp = (uint8_t*)base; base += b_grp;
  uint8_t* d_cost = (uint8_t*)base;
  if (lidar_cost_lds_bytes(K) > 64 * 1024) return fail(c, SAG_ERR_ARG, "K = %d points per env exceed the kernel's LDS staging (K <= 100)", K);
  HIPCHK(c, hipMemcpyAsync(d_robot, robot, (size_t)n * 3 * 4, hipMemcpyHostToDevice, c->stream));
  if (K > 0) {
    HIPCHK(c, hipMemcpyAsync(d_pts, points, (size_t)n * K * 2 * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_grp, group, (size_t)n * K, hipMemcpyHostToDevice, c->stream));
  }
  launch_lidar_cost(c, n, K, d_robot, d_pts, d_grp, hazard_size, d_lid, bins ? d_bins : nullptr, d_cost);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(lidar, d_lid, (size_t)n * 48 * 4, hipMemcpyDeviceToHost, c->stream));
  if (bins && K > 0) HIPCHK(c, hipMemcpyAsync(bins, d_bins, (size_t)n * K * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(cost, d_cost, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_lidar_cost_device(sag_ctx* c, int32_t n, int32_t K, const float* d_robot, const float* d_points,
                          const uint8_t* d_group, float hazard_size, float* d_lidar, int32_t* d_bins, uint8_t* d_cost) {
  if (!c) return SAG_ERR_ARG;
  if (n <= 0 || K < 0 || !d_robot || (K > 0 && (!d_points || !d_group)) || !d_lidar || !d_cost)
    return fail(c, SAG_ERR_ARG, "bad sag_lidar_cost_device arguments");
  // (every argument is checked BEFORE a timing-event pair is reserved: a pair that is counted but never recorded would
  //  add an earlier launch's timestamps to the kernel-time mean)
  if (lidar_cost_lds_bytes(K) > 64 * 1024) return fail(c, SAG_ERR_ARG, "K = %d points per env exceed the kernel's LDS staging (K <= 100)", K);
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = timing_events(c, &e0, &e1);
  if (rc) return rc;
  if (e0) HIPCHK(c, hipEventRecord(e0, c->stream));
  launch_lidar_cost(c, n, K, d_robot, d_points, d_group, hazard_size, d_lidar, d_bins, d_cost);
  if (e1) HIPCHK(c, hipEventRecord(e1, c->stream));
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_dev_alloc(sag_ctx* c, uint64_t bytes, void** dptr) {
  if (!c || !dptr) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMalloc(dptr, bytes));
  return SAG_OK;
}
int sag_dev_free(sag_ctx* c, void* dptr) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipFree(dptr));
  return SAG_OK;
}
int sag_dev_upload(sag_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}
int sag_dev_download(sag_ctx* c, void* dst, const void* src, uint64_t bytes) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}
int sag_dev_fill_actions(sag_ctx* c, float* d_actions, uint32_t step_index) {
  if (!c || !d_actions) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  hipLaunchKernelGGL(k_fill_actions, dim3((c->N + 255) / 256), dim3(256), 0, c->stream, d_actions, c->I, c->N,
                     c->rb.nu, (uint32_t)(c->cfg.seed & 0xffffffffu), (uint32_t)(c->cfg.seed >> 32), step_index);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}

int sag_enable_timing(sag_ctx* c, int32_t on) {
  if (!c) return SAG_ERR_ARG;
  c->timing = on != 0;
  return SAG_OK;
}

int sag_kernel_time_ms(sag_ctx* c, int32_t reset, double* mean_ms, int64_t* launches) {
  if (!c) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  drain_events(c);
  if (mean_ms) *mean_ms = c->ev_n ? c->ev_ms / (double)c->ev_n : 0.0;
  if (launches) *launches = c->ev_n;
  if (reset) { c->ev_ms = 0; c->ev_n = 0; }
  return SAG_OK;
}

int sag_debug_cycles(sag_ctx* c, int32_t reset, uint64_t* out, int32_t n) {
  if (!c || !out || n < 0) return SAG_ERR_ARG;
#ifdef SAG_WAVE_TIMES   // (start, end) per busy wavefront of the last launch; reset: cleared
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
  {
    // out: [WT_MAX][2] times, then [WT_MAX][32] env ids (two per word), then [WT_MAX][64] work bytes (eight per word)
    std::vector<uint64_t> host((size_t)(2 + 32 + 64 + 2) * WT_MAX);   // ... then [WT_MAX][8] wavefront passes (four per word)
    HIPCHK(c, hipMemcpyFromSymbol(host.data() + (size_t)98 * WT_MAX, HIP_SYMBOL(g_wt_trips), (size_t)2 * WT_MAX * sizeof(uint64_t)));
    HIPCHK(c, hipMemcpyFromSymbol(host.data(), HIP_SYMBOL(g_wt), (size_t)2 * WT_MAX * sizeof(uint64_t)));
    HIPCHK(c, hipMemcpyFromSymbol(host.data() + (size_t)2 * WT_MAX, HIP_SYMBOL(g_wt_env), (size_t)32 * WT_MAX * sizeof(uint64_t)));
    HIPCHK(c, hipMemcpyFromSymbol(host.data() + (size_t)34 * WT_MAX, HIP_SYMBOL(g_wt_work), (size_t)64 * WT_MAX * sizeof(uint64_t)));
    for (int k = 0; k < n; k++) out[k] = (size_t)k < host.size() ? host[k] : 0;
    if (reset) {
      std::fill(host.begin(), host.end(), 0);
      HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_wt), host.data(), (size_t)2 * WT_MAX * sizeof(uint64_t)));
    }
  }
  return SAG_OK;
#elif defined(SAG_CYCLES)
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // out[0 .. 48): sums per kernel form and section (+ wavefront count); out[48 .. 96): the sections of the slowest wavefront;
  // out[96 .. 99): its block index; out[99 .. 291): wavefronts by total ticks, 3 x 64 buckets of a quarter octave from 2^10
  constexpr int M = 3 * (CY_N + 1);
  uint64_t host[2 * M + 3 + 192];
  HIPCHK(c, hipMemcpyFromSymbol(host, HIP_SYMBOL(g_cyc), M * sizeof(uint64_t)));
  HIPCHK(c, hipMemcpyFromSymbol(host + M, HIP_SYMBOL(g_cyc_worst), M * sizeof(uint64_t)));
  HIPCHK(c, hipMemcpyFromSymbol(host + 2 * M, HIP_SYMBOL(g_cyc_worst_block), 3 * sizeof(uint64_t)));
  HIPCHK(c, hipMemcpyFromSymbol(host + 2 * M + 3, HIP_SYMBOL(g_cyc_hist), 192 * sizeof(uint64_t)));
  for (int k = 0; k < n; k++) out[k] = k < 2 * M + 3 + 192 ? host[k] : 0;
  if (reset) {
    memset(host, 0, sizeof(host));
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_cyc), host, M * sizeof(uint64_t)));
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_cyc_worst), host, M * sizeof(uint64_t)));
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_cyc_hist), host, 192 * sizeof(uint64_t)));
  }
  return SAG_OK;
#else
  (void)reset;
  for (int k = 0; k < n; k++) out[k] = 0;
  return SAG_ERR_UNSUPPORTED;
#endif
}

// diagnostic (tests): mass matrix, bias, contact-free qacc and M^-1 of every Doggo env from the
// wave-cooperative routines; out[n_envs][2*361 + 38] doubles (host)
int sag_debug_doggo_coop(sag_ctx* c, double* out) {
  if (!c || !out) return SAG_ERR_ARG;
  if (c->cfg.robot != SAG_ROBOT_DOGGO) return fail(c, SAG_ERR_ARG, "not a doggo context");
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t bytes = (size_t)c->N * (2 * DG_NV * DG_NV + 2 * DG_NV) * sizeof(double);
  double* d = nullptr;
  HIPCHK(c, hipMalloc(&d, bytes));
  hipLaunchKernelGGL(k_doggo_coop_debug, dim3((c->N + DC_EPW - 1) / DC_EPW), dim3(32 * DC_EPW), 0, c->stream, c->S, c->N, d);
  hipError_t e = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIPCHK(c, e);
  return SAG_OK;
}

// Images of the envs at their current state, ray-cast on the device (sag_render.hpp).  output: 0 the colour image
// [rows][height][width][3] uint8, or one of enum sag_render_output.  -> bytes per pixel, 0 for an unknown output
static size_t render_pixel_bytes(int32_t output) {
  return output == R_OUT_RGB ? 3 : output == SAG_RENDER_DEPTH ? sizeof(float) : output == SAG_RENDER_SEGMENTATION ? sizeof(RSegPixel) : 0;
}
static int render_args_ok(sag_ctx* c, const char* who, int32_t output, int32_t camera, int32_t width, int32_t height) {
  if (!render_pixel_bytes(output)) return fail(c, SAG_ERR_ARG, "%s: unknown output %d", who, output);
  if (camera < 0 || camera > SAG_CAM_TRACK || width <= 0 || height <= 0 || width > 4096 || height > 4096)
    return fail(c, SAG_ERR_ARG, "%s: bad camera %d or image size %d x %d", who, camera, width, height);
  return SAG_OK;
}
extern "C++" template <int OUT>   // (this file's functions are extern "C")
void render_launch_as(sag_ctx* c, const RenderArgs& a, const uint8_t* d_mask, const int32_t* d_ids, int rows) {
  if (d_ids) hipLaunchKernelGGL(k_render_list<OUT>, dim3(rows), dim3(256), 0, c->stream, a, d_ids);
  else hipLaunchKernelGGL(k_render_rows<OUT>, dim3(rows), dim3(256), 0, c->stream, a, d_mask);
}
// One launch, stream-ordered, no wait: `rows` workgroups, listed (d_ids: workgroup j renders env d_ids[j] into row j) or
// masked in place (d_mask; NULL: every env, rows = n_envs).  d_obs / d_cost: the observation and cost flags the overlays show
// (device pointers or NULL).  d_out: aligned to its pixel, 4 B depth / 8 B segmentation.  A refused call launches nothing.
static int render_launch(sag_ctx* c, const char* who, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags,
                         const float* d_obs, const uint8_t* d_cost, const uint8_t* d_mask, const int32_t* d_ids, int rows, void* d_out) {
  if (!c) return SAG_ERR_ARG;
  if (int rc = render_args_ok(c, who, output, camera, width, height)) return rc;
  if (!d_out) return fail(c, SAG_ERR_ARG, "%s: null argument", who);
  if (output != R_OUT_RGB && reinterpret_cast<uintptr_t>(d_out) % render_pixel_bytes(output))
    return fail(c, SAG_ERR_ARG, "%s: d_out is not aligned to %d bytes", who, (int)render_pixel_bytes(output));
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const RenderArgs a = {c->S, c->I, c->N, c->cfg.robot, camera, width, height, flags, d_obs, c->rb.obs_dim, d_cost, d_out};
  if (output == SAG_RENDER_DEPTH) render_launch_as<R_OUT_DEPTH>(c, a, d_mask, d_ids, rows);
  else if (output == SAG_RENDER_SEGMENTATION) render_launch_as<R_OUT_SEG>(c, a, d_mask, d_ids, rows);
  else if (d_ids || d_mask) render_launch_as<R_OUT_RGB>(c, a, d_mask, d_ids, rows);
  else hipLaunchKernelGGL(k_render_rgb, dim3(rows), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  return SAG_OK;
}
// the staging buffer of render_to_host holds at least `bytes`; rgb_bytes is what d_rgb really has
static int ensure_rgb(sag_ctx* c, size_t bytes) {
  if (c->rgb_bytes >= bytes) return 0;
  if (c->d_rgb) (void)hipFree(c->d_rgb);
  c->d_rgb = nullptr; c->rgb_bytes = 0;
  HIPCHK(c, hipMalloc(&c->d_rgb, bytes ? bytes : 1));
  c->rgb_bytes = bytes;
  return 0;
}
// Into a host buffer, joined: row j = env env_ids[j] of n listed envs, or (env_ids == NULL, n = n_envs) every env.  The
// staging buffer holds the index list (4 n bytes, rounded up to 16) in front of the n images, so it is sized for the rows asked
// for.  The overlays show what the last host-buffer step / observe left in the context's output buffers.
static int render_to_host(sag_ctx* c, const char* who, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags,
                          const int32_t* env_ids, int32_t n, void* out) {
  if (!c) return SAG_ERR_ARG;
  if (int rc = render_args_ok(c, who, output, camera, width, height)) return rc;   // (before the sizes below are taken from it)
  if (n < 0 || (n > 0 && !out)) return fail(c, SAG_ERR_ARG, "%s: n %d or a null argument", who, n);
  for (int32_t j = 0; env_ids && j < n; j++)
    if (env_ids[j] < 0 || env_ids[j] >= c->N) return fail(c, SAG_ERR_ARG, "%s: env %d (entry %d) of %d envs", who, env_ids[j], j, c->N);
  if (n == 0) return SAG_OK;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  const size_t list = env_ids ? ((size_t)n * sizeof(int32_t) + 15) & ~(size_t)15 : 0;
  const size_t bytes = (size_t)n * width * height * render_pixel_bytes(output);
  if (int rc = ensure_rgb(c, list + bytes)) return rc;
  // (the stream is joined below: env_ids has been read when the call returns)
  if (env_ids) HIPCHK(c, hipMemcpyAsync(c->d_rgb, env_ids, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (int rc = render_launch(c, who, output, camera, width, height, flags, (const float*)c->d_obs, (const uint8_t*)c->d_cost, nullptr,
                             env_ids ? reinterpret_cast<const int32_t*>(c->d_rgb) : nullptr, n, c->d_rgb + list)) return rc;
  HIPCHK(c, hipMemcpyAsync(out, c->d_rgb + list, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SAG_OK;
}

int sag_render_device(sag_ctx* c, int32_t camera, int32_t width, int32_t height, int32_t flags, const float* d_obs,
                      const uint8_t* d_cost, void* d_out) {
  return sag_render_rows_device(c, camera, width, height, flags, d_obs, d_cost, nullptr, d_out);
}
// the envs of a device mask, each into its own row: the grid is sized for n_envs whatever the mask holds, and a workgroup
// whose byte is zero returns at once (k_render_rows) - nothing the host decides, so it follows a reset on the stream.
// A NULL mask launches k_render_rgb.
int sag_render_rows_device(sag_ctx* c, int32_t camera, int32_t width, int32_t height, int32_t flags, const float* d_obs,
                           const uint8_t* d_cost, const uint8_t* d_mask, void* d_out) {
  return render_launch(c, d_mask ? "sag_render_rows_device" : "sag_render_device", R_OUT_RGB, camera, width, height, flags, d_obs, d_cost,
                       d_mask, nullptr, c ? c->N : 0, d_out);
}
int sag_render(sag_ctx* c, int32_t camera, int32_t width, int32_t height, int32_t flags, uint8_t* out) {
  return render_to_host(c, "sag_render", R_OUT_RGB, camera, width, height, flags, nullptr, c ? c->N : 0, out);
}
int sag_render_envs(sag_ctx* c, int32_t camera, int32_t width, int32_t height, int32_t flags, const int32_t* env_ids, int32_t n,
                    uint8_t* out) {
  if (c && !env_ids)   // (no list is not "every env" here: it goes with n == 0 alone)
    return n ? fail(c, SAG_ERR_ARG, "sag_render_envs: n %d or a null argument", n) : render_args_ok(c, "sag_render_envs", R_OUT_RGB, camera, width, height);
  return render_to_host(c, "sag_render_envs", R_OUT_RGB, camera, width, height, flags, env_ids, n, out);
}
// depth / segmentation: output 0, the colour image, has the entry points above
int sag_render_aux_device(sag_ctx* c, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags,
                          const float* d_obs, const uint8_t* d_cost, const uint8_t* d_mask, void* d_out) {
  if (c && output == R_OUT_RGB) return fail(c, SAG_ERR_ARG, "sag_render_aux_device: unknown output 0");
  return render_launch(c, "sag_render_aux_device", output, camera, width, height, flags, d_obs, d_cost, d_mask,
                       nullptr, c ? c->N : 0, d_out);
}
// env_ids == NULL: every env, n is ignored
int sag_render_aux(sag_ctx* c, int32_t output, int32_t camera, int32_t width, int32_t height, int32_t flags, const int32_t* env_ids,
                   int32_t n, void* out) {
  if (c && output == R_OUT_RGB) return fail(c, SAG_ERR_ARG, "sag_render_aux: unknown output 0");
  return render_to_host(c, "sag_render_aux", output, camera, width, height, flags, env_ids, c && !env_ids ? c->N : n, out);
}
// rgb_observation: the 64 x 64 image of the robot's own camera, no overlays
int sag_render_rgb_device(sag_ctx* c, void* d_out) { return sag_render_device(c, SAG_CAM_VISION, R_W, R_H, 0, nullptr, nullptr, d_out); }
int sag_render_rgb(sag_ctx* c, uint8_t* out) { return sag_render(c, SAG_CAM_VISION, R_W, R_H, 0, out); }

int sag_busy_count(sag_ctx* c, int32_t* count) {
  if (!c || !count) return SAG_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->cfg.device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!c->last_count) { *count = 0; return SAG_OK; }
  int32_t per_kind[BUSY_CLASSES];   // the lists the last step consumed
  HIPCHK(c, hipMemcpy(per_kind, c->last_count, sizeof(per_kind), hipMemcpyDeviceToHost));
  *count = 0;
  for (int k = 0; k < BUSY_CLASSES; k++) *count += per_kind[k];
  return SAG_OK;
}

}  // extern "C"
