// sag_reset.hpp - throughput mode's reset on the device (sag_reset_device): World.sample_layout + _build_world_config +
// task.reset for a batch of envs, the same steps as sample_one / try_layout of sag_sampler.cpp with one change: the words
// come from Philox4x32-10 under the context key on stream 3 instead of one MT19937 per env.
//
// Every draw is addressed by what it is for, not by a running stream position:
//   candidate t of placement k in layout attempt a:  counter (env id, a << 8 | k, t, nonce << 2 | 3)
//   draws after the layout:                          counter (env id, 0x80000000 | purpose, block, nonce << 2 | 3)
// A block gives x from words 0-1 and y from words 2-3 (53 bits each, Rng::sample).  Candidates are i.i.d. uniforms as on
// the host, so the layouts follow the host sampler's distribution, and any schedule yields the same records.
//
// Schedule: one env per lane with the candidate loop flattened - one loop trip draws and tests ONE candidate in every lane,
// whatever placement (or goal resample) that lane's env is at; a lane whose env is done starts its next env in the next
// trip.  A wavefront therefore waits for its slowest lane only once, at the end of its share of the batch, not once per
// env (the rejection work is very uneven: Point/GoToGoal mean 69 candidates per layout, p99 729).  The placed positions
// live in LDS, [item][lane] (30 KB per wavefront).
//
// Arithmetic: fp64 without contraction, the host's operation order; the keep-out test is the host's
// sqrt(dx^2 + dy^2) < k, decided on the squares outside a relative guard band of 1e-9 and exactly inside it.
#pragma once
#include "sag_device.hpp"

namespace sag {

constexpr int RS_MAX_ITEMS = 1 + SAG_MAX_HAZARDS + SAG_MAX_VASES + SAG_MAX_PILLARS + 2 + SAG_MAX_BUTTONS;
constexpr int RS_BLOCK = 64;                 // one wavefront per workgroup (LDS: RS_MAX_ITEMS x 2 x 64 doubles)
constexpr int RS_PLACE_TRIES = 1000, RS_LAYOUT_TRIES = 10000, RS_GOAL_TRIES = 10000;   // world.py:191-217, go_to_goal.py:59-80
constexpr uint32_t RS_STREAM = 3;            // counter word 3 = nonce << 2 | stream (0 in-step, 1 noise, 2 bench policy)
constexpr uint32_t RS_POST = 0x80000000u;    // counter word 1 of the draws after the layout: RS_POST | purpose
enum : uint32_t {
  RS_P_ROT = 0x000,      // robot rotation (block 0)
  RS_P_YAW = 0x100,      // | item: yaw of a vase / the task object (block 0)
  RS_P_GOAL = 0x200,     // goal resample: block = candidate index
  RS_P_BUTTON = 0x300,   // rs.choice(n_buttons): masked rejection over words 0..3 of blocks 0, 1, ...
  RS_P_CTRL = 0x400,     // | actuator: Cauchy ctrl scale, a point of the unit disc by rejection over blocks 0, 1, ...
  RS_P_BOUND = 0x500     // U(0, max_bound) (block 0)
};
constexpr int RS_REJECT_BLOCKS = 64;         // rejection draws give up after this many blocks (probability < 1e-40)

struct ResetArgs {
  const sag_task_desc* descs;   // [n_descs]
  const int32_t* desc_of_env;   // [N]
  sag_world_config cfg;
  const float* S;               // current state (later episodes keep a few fields of it)
  const int32_t* I;
  int32_t N;
  const int32_t* ids;           // envs to sample: ids[j], or j when nullptr
  int32_t n;
  const int32_t* n_dev;         // the length of the list in device memory (stream-ordered form: the host never sees it), or nullptr: n
  int32_t robot, first_episode, have_state;
  uint32_t episode0;            // nonce of an env that has no layout yet
  int32_t env_id0;              // global id of env 0 of the context
  uint32_t k0, k1;
  float* rec_f;                 // [n][SAG_REC_FLOATS] staging, record of ids[j] at j
  int32_t* rec_i;               // [n][SAG_REC_INTS]
  int32_t* status;              // [N] by env: 0, -1 (layout attempts exhausted), -2 (goal resample exhausted)
  int32_t* n_fail;
};

__device__ inline float rs_state(const ResetArgs& p, int field, size_t i) { return p.S[saddr(field, (size_t)p.N, i)]; }

__device__ inline void rs_block(uint32_t gid, uint32_t w1, uint32_t w2, uint32_t nonce4, uint32_t k0, uint32_t k1, uint32_t c[4]) {
  c[0] = gid; c[1] = w1; c[2] = w2; c[3] = nonce4;
  philox4x32_10(c, k0, k1);
}
// numpy's random_sample from two words (Rng::sample)
__device__ inline double rs_u53(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}
__device__ inline double rs_uniform(double lo, double hi, double u) {
#pragma clang fp contract(off)
  return lo + (hi - lo) * u;
}
// the host's `sqrt(dx * dx + dy * dy) < k`
__device__ inline bool rs_closer(double dx, double dy, double k) {
#pragma clang fp contract(off)
  if (!(k > 0)) return false;
  const double d2 = dx * dx + dy * dy, k2 = k * k;
  if (d2 < k2 * (1.0 - 1e-9)) return true;
  if (d2 > k2 * (1.0 + 1e-9)) return false;
  return sqrt(d2) < k;
}

// the placements of a descriptor in the reference's dict order: robot, hazards, vases, pillars, goal, box, buttons
struct RsItems {
  int nH, nV, nP, i_goal, i_box, i_btn, n;
  double k_rob, k_haz, k_vase, k_pil, k_goal, k_box, k_btn;
  __device__ int kind(int q) const {   // 0 robot 1 hazard 2 vase 3 pillar 4 goal 5 box 6 button
    return q == 0 ? 0 : q <= nH ? 1 : q <= nH + nV ? 2 : q <= nH + nV + nP ? 3 : q == i_goal ? 4 : q == i_box ? 5 : 6;
  }
  __device__ double keepout(int q) const {
    const int c = kind(q);
    return c == 0 ? k_rob : c == 1 ? k_haz : c == 2 ? k_vase : c == 3 ? k_pil : c == 4 ? k_goal : c == 5 ? k_box : k_btn;
  }
};

__device__ inline RsItems rs_items(const sag_task_desc& T, const sag_world_config& cfg) {
  RsItems it;
  it.nH = T.n_hazards; it.nV = T.n_vases; it.nP = T.n_pillars;
  int n = 1 + it.nH + it.nV + it.nP;
  it.i_goal = T.has_goal ? n++ : -1;
  it.i_box = T.box_kind ? n++ : -1;
  it.i_btn = T.n_buttons ? n : -1;
  n += T.n_buttons;
  it.n = n;
  it.k_rob = cfg.robot_keepout;
  it.k_haz = fmax(cfg.hazards_keepout, cfg.hazards_size);
  it.k_vase = fmax(cfg.vases_keepout, cfg.vases_size);
  it.k_pil = fmax(cfg.pillars_keepout, cfg.pillars_size);
  it.k_goal = T.goal_keepout; it.k_box = T.box_keepout; it.k_btn = T.button_keepout;
  return it;
}

// the rectangle placement q draws from (its own, or the task extents)
__device__ inline void rs_rect(const sag_task_desc& T, const RsItems& it, int q, double r[4]) {
  const int c = it.kind(q);
  const double* own = c == 5 ? T.box_rect : c == 6 ? T.button_rect : nullptr;
  const bool none = !own || (own[0] == 0 && own[1] == 0 && own[2] == 0 && own[3] == 0);
  if (c == 4) { r[0] = r[1] = -1.5; r[2] = r[3] = 1.5; }   // goal: (-1.5, -1.5, 1.5, 1.5) (go_to_goal.py)
  else for (int e = 0; e < 4; e++) r[e] = none ? T.extents[e] : own[e];
}

// a sampled env's record (as sample_one writes it; later episodes keep the Task-object fields of the current state)
__device__ inline void rs_write(const ResetArgs& p, const sag_task_desc& T, const RsItems& it, int j, int i, uint32_t gid,
                                uint32_t nonce, const double (*sx)[RS_BLOCK], const double (*sy)[RS_BLOCK], int lane) {
#pragma clang fp contract(off)
  const uint32_t n4 = nonce << 2 | RS_STREAM;
  const double two_pi = 2 * 3.14159265358979323846;
  float* rf = p.rec_f + (size_t)j * SAG_REC_FLOATS;
  int32_t* ri = p.rec_i + (size_t)j * SAG_REC_INTS;
  uint32_t c[4];
  for (int k = 0; k < SAG_REC_FLOATS; k++) rf[k] = 0.f;
  for (int k = 0; k < SAG_REC_INTS; k++) ri[k] = 0;
  rs_block(gid, RS_POST | RS_P_ROT, 0, n4, p.k0, p.k1, c);
  const double robot_rot = rs_uniform(0, two_pi, rs_u53(c[0], c[1]));
  // ctrl scale and bound: drawn for a new Task object (world.py:72-78), kept from the current state otherwise
  const int nu = p.robot == SAG_ROBOT_DOGGO ? 12 : 2;
  for (int k = 0; k < SAG_MAX_NU; k++) {
    double v = 1.0;
    if (!p.first_episode) {
      v = rs_state(p, SAG_F_CTRL_SCALE + k, i);
    } else if (k < nu) {
      for (int b = 0; b < RS_REJECT_BLOCKS; b++) {   // standard Cauchy = x1 / x2 of a uniform point of the unit disc
        rs_block(gid, RS_POST | RS_P_CTRL | (uint32_t)k, (uint32_t)b, n4, p.k0, p.k1, c);
        const double x1 = 2.0 * rs_u53(c[0], c[1]) - 1.0, x2 = 2.0 * rs_u53(c[2], c[3]) - 1.0;
        const double r2 = x1 * x1 + x2 * x2;
        if (r2 >= 1.0 || r2 == 0.0) continue;
        v = x1 / x2 * p.cfg.robot_ctrl_range_scale + 1.0;
        break;
      }
    }
    rf[SAG_F_CTRL_SCALE + k] = (float)v;
  }
  float bound = (float)p.cfg.max_bound;
  if (!p.first_episode) bound = rs_state(p, SAG_F_BOUND, i);
  else if (p.cfg.random_bound) {
    rs_block(gid, RS_POST | RS_P_BOUND, 0, n4, p.k0, p.k1, c);
    bound = (float)rs_uniform(0.0, p.cfg.max_bound, rs_u53(c[0], c[1]));
  }
  // task.reset (App. B.5)
  int goal_button = 0, btn_timer = 0;
  uint32_t active_mask = 0;
  if (T.button_reset == 1) {   // rs.choice(n_buttons): masked rejection bounded integer in [0, n_buttons - 1]
    const uint32_t mx = (uint32_t)T.n_buttons - 1;
    uint32_t mask = mx;
    mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
    bool got = mx == 0;
    for (int b = 0; b < RS_REJECT_BLOCKS && !got; b++) {
      rs_block(gid, RS_POST | RS_P_BUTTON, (uint32_t)b, n4, p.k0, p.k1, c);
      for (int q = 0; q < 4 && !got; q++)
        if ((c[q] & mask) <= mx) { goal_button = (int)(c[q] & mask); got = true; }
    }
    btn_timer = T.button_timer;
  }
  if (T.button_reset == 2) active_mask = (1u << T.n_buttons) - 1;
  int btn_state = 1, catch_timer = 0;
  float catch_cur = 1.0f, catch_next = 0.2f;
  if (!p.first_episode) {
    const uint32_t ts = (uint32_t)p.I[iaddr(DI_TSTATE, (size_t)p.N, (size_t)i)];
    btn_state = ts >> 3 & 1; catch_timer = ts >> 7 & 15;
    catch_cur = rs_state(p, SAG_F_CATCH + 2, i); catch_next = rs_state(p, SAG_F_CATCH + 3, i);
  }
  ri[SAG_I_TASK] = T.task_id; ri[SAG_I_NH] = T.n_hazards; ri[SAG_I_NV] = T.n_vases; ri[SAG_I_NP] = T.n_pillars;
  ri[SAG_I_NB] = T.n_buttons; ri[SAG_I_BOX_KIND] = T.box_kind; ri[SAG_I_ENV_ID] = (int32_t)gid;
  ri[SAG_I_GOAL_BUTTON] = goal_button; ri[SAG_I_BTN_STATE] = btn_state; ri[SAG_I_BTN_TIMER] = btn_timer;
  ri[SAG_I_CATCH_TIMER] = catch_timer; ri[SAG_I_ACTIVE_MASK] = (int32_t)active_mask;
  ri[SAG_I_EPISODE] = (int32_t)nonce;
  rf[SAG_F_ROBOT] = (float)sx[0][lane]; rf[SAG_F_ROBOT + 1] = (float)sy[0][lane]; rf[SAG_F_ROBOT + 2] = (float)robot_rot;
  for (int k = 0; k < 3; k++) rf[SAG_F_ROBOT0 + k] = rf[SAG_F_ROBOT + k];
  if (p.robot == SAG_ROBOT_CAR) rf[SAG_F_ROBOT_EXT + 5] = 1.0f;   // rear ball quaternion w; doggo: all zero = reset pose
  rf[SAG_F_GEAR] = (float)T.gear; rf[SAG_F_DAMP] = (float)T.damping;
  rf[SAG_F_ACTION_NOISE] = (float)p.cfg.action_noise;
  rf[SAG_F_HAZARD_SIZE] = (float)p.cfg.hazards_size; rf[SAG_F_VASE_SIZE] = (float)p.cfg.vases_size;
  rf[SAG_F_PILLAR_SIZE] = (float)p.cfg.pillars_size;
  rf[SAG_F_KEEPOUT] = (float)it.k_rob; rf[SAG_F_KEEPOUT + 1] = (float)it.k_haz;
  rf[SAG_F_KEEPOUT + 2] = (float)it.k_vase; rf[SAG_F_KEEPOUT + 3] = (float)it.k_pil;
  rf[SAG_F_KEEPOUT + 4] = (float)T.box_keepout;
  rf[SAG_F_CATCH + 2] = catch_cur; rf[SAG_F_CATCH + 3] = catch_next;
  rf[SAG_F_BOUND] = bound;
  int h = 0, v = 0, pl = 0, b = 0;
  for (int k = 1; k < it.n; k++) {
    const float x = (float)sx[k][lane], y = (float)sy[k][lane];
    switch (it.kind(k)) {
      case 1: rf[SAG_F_HAZARDS + 2 * h] = x; rf[SAG_F_HAZARDS + 2 * h + 1] = y; h++; break;
      case 2:
        rs_block(gid, RS_POST | RS_P_YAW | (uint32_t)k, 0, n4, p.k0, p.k1, c);
        rf[SAG_F_VASES + 6 * v] = x; rf[SAG_F_VASES + 6 * v + 1] = y; rf[SAG_F_VASES + 6 * v + 2] = (float)rs_uniform(0, two_pi, rs_u53(c[0], c[1]));
        v++;
        break;
      case 3: rf[SAG_F_PILLARS + 2 * pl] = x; rf[SAG_F_PILLARS + 2 * pl + 1] = y; pl++; break;
      case 4:
        rf[SAG_F_GOAL] = x; rf[SAG_F_GOAL + 1] = y;
        if (T.task_id == SAG_TASK_CATCH_GOAL) { rf[SAG_F_CATCH] = x; rf[SAG_F_CATCH + 1] = y; }
        break;
      case 5: {
        double yaw = 0;
        if (T.box_yaw) {
          rs_block(gid, RS_POST | RS_P_YAW | (uint32_t)k, 0, n4, p.k0, p.k1, c);
          yaw = rs_uniform(0, two_pi, rs_u53(c[0], c[1]));
        }
        rf[SAG_F_BOX] = x; rf[SAG_F_BOX + 1] = y; rf[SAG_F_BOX + 2] = (float)yaw;
        break;
      }
      default: rf[SAG_F_BUTTONS + 2 * b] = x; rf[SAG_F_BUTTONS + 2 * b + 1] = y; b++; break;
    }
  }
}

// One env per lane, one candidate per lane per loop trip (see the head of this file).  The grid strides over the list,
// whose length is p.n or, where the host never learns it, *p.n_dev (the grid is then sized for the upper bound).
__global__ __launch_bounds__(RS_BLOCK) void k_reset_sample(ResetArgs p) {
#pragma clang fp contract(off)
  __shared__ double sx[RS_MAX_ITEMS][RS_BLOCK], sy[RS_MAX_ITEMS][RS_BLOCK];
  const int lane = threadIdx.x;
  const int stride = gridDim.x * RS_BLOCK;
  const int n = p.n_dev ? *p.n_dev : p.n;
  enum { PLACE = 0, GOAL = 1, NEXT = 2 };
  // Entry j of the list goes to wavefront j mod gridDim: a list shorter than the grid (a few envs ending per step) gives
  // every env a wavefront of its own, which then walks only that env's loops instead of the union over 64 envs' phases
  int j = lane * gridDim.x + blockIdx.x - stride;   // the first NEXT moves to the lane's first env
  int phase = NEXT, i = 0, a = 0, k = 0, t = 0;
  uint32_t gid = 0, n4 = 0, nonce = 0;
  const sag_task_desc* T = nullptr;
  RsItems it{};
  double margin = 0, ko = 0, lo_x = 0, hi_x = 0, lo_y = 0, hi_y = 0, g = 0;
  bool live = true;
  auto setup_place = [&]() {   // the rectangle and keep-out of placement k
    double r[4];
    rs_rect(*T, it, k, r);
    ko = it.keepout(k);
    lo_x = r[0] + ko; hi_x = r[2] - ko; lo_y = r[1] + ko; hi_y = r[3] - ko;
  };
  auto fail = [&](int code) {
    p.status[i] = code;
    atomicAdd(p.n_fail, 1);
    phase = NEXT;
  };
  while (__ballot(live)) {
    if (!live) continue;
    if (phase == NEXT) {
      j += stride;
      if (j >= n) { live = false; continue; }
      i = p.ids ? p.ids[j] : j;
      // a later episode draws under the id the env carries: its own (env_id0 + i) unless a fork with SAG_FORK_SAME_STREAM gave
      // it its source's, in which case source and copy go on sampling the same layouts
      gid = p.have_state && !p.first_episode ? (uint32_t)p.I[iaddr(DI_ENVID, (size_t)p.N, (size_t)i)] : (uint32_t)(p.env_id0 + i);
      T = &p.descs[p.desc_of_env[i]];
      it = rs_items(*T, p.cfg);
      margin = p.cfg.placements_margin + (p.robot == SAG_ROBOT_DOGGO ? 0.165 : 0.0);
      nonce = p.have_state ? (((uint32_t)p.I[iaddr(DI_FLAGS, (size_t)p.N, (size_t)i)] >> FLAG_EPISODE_SHIFT) + 1) & 0xffffffu
                           : p.episode0 & 0xffffffu;
      n4 = nonce << 2 | RS_STREAM;
      a = 0; k = 0; t = 0;
      phase = PLACE;
      setup_place();
      continue;
    }
    uint32_t c[4];
    double x, y, gk = 0;
    int jmax, skip;
    if (phase == PLACE) {
      rs_block(gid, (uint32_t)a << 8 | (uint32_t)k, (uint32_t)t, n4, p.k0, p.k1, c);
      x = rs_uniform(lo_x, hi_x, rs_u53(c[0], c[1]));
      y = rs_uniform(lo_y, hi_y, rs_u53(c[2], c[3]));
      jmax = k; skip = -1;
    } else {   // GoToGoal._resample_goal_position: a square of half extent g, g *= 1.01 per rejection, no margin
      rs_block(gid, RS_POST | RS_P_GOAL, (uint32_t)t, n4, p.k0, p.k1, c);
      gk = it.k_goal;
      x = rs_uniform(-g + gk, g - gk, rs_u53(c[0], c[1]));
      y = rs_uniform(-g + gk, g - gk, rs_u53(c[2], c[3]));
      jmax = it.n; skip = it.i_goal;
    }
    bool ok = true;
    for (int q = 0; q < jmax && ok; q++) {
      if (q == skip) continue;
      const double thr = phase == PLACE ? it.keepout(q) + margin + ko : it.keepout(q) + gk;
      if (rs_closer(x - sx[q][lane], y - sy[q][lane], thr)) ok = false;
    }
    if (phase == PLACE) {
      if (ok) {
        sx[k][lane] = x; sy[k][lane] = y;
        t = 0;
        if (++k < it.n) { setup_place(); continue; }
        if (it.i_box >= 0 && T->box_at_robot) {   // haul_box.py:17-18: the object at robot + (box_offset, 0)
          sx[it.i_box][lane] = sx[0][lane] + T->box_offset;
          sy[it.i_box][lane] = sy[0][lane];
        }
        if (it.i_goal >= 0) { phase = GOAL; g = 1.5; continue; }
      } else {
        if (++t < RS_PLACE_TRIES) continue;
        t = 0; k = 0;
        if (++a >= RS_LAYOUT_TRIES) { fail(-1); continue; }
        setup_place();
        continue;
      }
    } else if (!ok) {
      g = g * 1.01;   // utils.increase_extents
      if (++t >= RS_GOAL_TRIES) fail(-2);
      continue;
    } else {
      sx[it.i_goal][lane] = x; sy[it.i_goal][lane] = y;
    }
    rs_write(p, *T, it, j, i, gid, nonce, sx, sy, lane);
    p.status[i] = 0;   // (every listed env leaves with its status written: k_reset_commit reads it without a memset between calls)
    phase = NEXT;
  }
}

// masked envs (nullptr: every env) -> a list of their indices (in any order; the records are keyed by env, not by position).  One atomic per
// wavefront: the adds all hit one counter and serialise
__global__ void k_reset_list(const uint8_t* mask, int N, int32_t* ids, int32_t* count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  const bool on = i < N && (!mask || mask[i]);
  const uint64_t m = __ballot(on);
  int base = 0;
  if (lane == 0 && m) base = atomicAdd(count, __popcll(m));
  base = __shfl(base, 0);
  if (on) ids[base + __popcll(m & ((1ull << lane) - 1))] = i;
}

// info['bound'] of every env from the installed state
__global__ void k_reset_bound(const float* S, int N, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) out[i] = S[saddr(SAG_F_BOUND, (size_t)N, (size_t)i)];
}

}  // namespace sag
