// obs_norm_main.cpp - TEST INFRASTRUCTURE: sag_obs_stats_device, sag_policy_forward_norm_device and
// sag_policy_backward_norm_device of the host build of the device sources (tests/hostemu/build.py) driven from a program of its
// own, so that the whole process - this file and the library - runs under AddressSanitizer and UndefinedBehaviorSanitizer
// (test_obs_norm_hostemu.py compiles and runs it).  "Device" memory is malloc'ed there.  Every input is allocated at its exact
// size - the last plane ends with the last column of its last counted row, so a read of a pad row or a pad column behind it is
// a heap overflow - and the state, the table and every output have guard words behind them that must keep their fill.
// The moments are compared with plain loops in double precision (1e-5 on the column's deviation and of M2: fp32 sums of <= 3075
// terms stay below 1e-6, a dropped row costs >= 1 / 3075), the table bit for bit with the header's expression on the library's
// own state, and the normalised forward and backward bit for bit with the plain entry points on rows normalised here.
// Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "obs_norm_main: ok" on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sag.h"

namespace {

constexpr int GUARD = 8;
constexpr float FILL = 7.0f;
sag_ctx* g_ctx = nullptr;
int g_failures = 0;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      printf("FAILED %s:%d: ", __FILE__, __LINE__);       \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      if (++g_failures > 20) exit(1);                      \
    }                                                      \
  } while (0)

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_rng >> 33);
}
float sym(float s) { return s * ((float)(rnd() & 0xffffff) / 8388608.0f - 1.0f); }

template <class T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;
  explicit Dev(const std::vector<T>& v) : n(v.size()) {
    void* q = nullptr;
    if (sag_dev_alloc(g_ctx, n * sizeof(T), &q) != SAG_OK) { printf("sag_dev_alloc failed\n"); exit(1); }
    p = (T*)q;
    if (n) sag_dev_upload(g_ctx, p, v.data(), n * sizeof(T));
  }
  ~Dev() { sag_dev_free(g_ctx, p); }
  std::vector<T> get() const {
    std::vector<T> v(n);
    if (n) sag_dev_download(g_ctx, v.data(), p, n * sizeof(T));
    return v;
  }
};

// column k: deviation 10^(-3 ... 3), a mean of about one deviation
float col_scale(int k, int od) { return powf(10.0f, -3.0f + 6.0f * (float)((k * 37) % od) / (float)(od - 1)); }

// [n_planes][pitch][obs_pitch], cut behind column od - 1 of row n_rows - 1 of the last plane; pad rows and pad columns are NaN
std::vector<float> obs_rows(int od, int n_rows, int n_planes, int pitch, int obs_pitch) {
  std::vector<float> v(((size_t)(n_planes - 1) * pitch + n_rows - 1) * obs_pitch + od, nanf(""));
  for (int p = 0; p < n_planes; p++)
    for (int r = 0; r < n_rows; r++)
      for (int k = 0; k < od; k++) v[((size_t)p * pitch + r) * obs_pitch + k] = col_scale(k, od) * (1.3f + sym(3.0f));
  return v;
}

float norm_chain(float x, float m, float r, float clip) {
  volatile float d = x - m;
  volatile float t = d * r;
  float xh = t;
  xh = xh < -clip ? -clip : xh;
  xh = xh > clip ? clip : xh;
  return xh;
}

bool table_is_of_state(const std::vector<double>& s, const std::vector<float>& t, int od, float eps) {
  for (int k = 0; k < od; k++) {
    const float m = s[0] > 0 ? (float)s[1 + k] : 0.0f;
    const float r = s[0] > 0 ? (float)(1.0 / sqrt(s[1 + od + k] / s[0] + (double)eps)) : 1.0f;
    if (memcmp(&m, &t[k], 4) != 0 || memcmp(&r, &t[od + k], 4) != 0) return false;
  }
  return true;
}

// two successive batches into one state, then TABLE_ONLY
void stats_case(int od, int n_rows, int n_planes, int pitch, int obs_pitch, int max_blocks) {
  const float eps = 1e-8f;
  std::vector<double> s0(1 + 2 * od + GUARD, (double)FILL);
  for (int k = 0; k < 1 + 2 * od; k++) s0[k] = 0.0;
  Dev<double> d_state(s0);
  Dev<float> d_table(std::vector<float>(2 * od + GUARD, FILL));
  std::vector<double> sum(od, 0.0), all;
  double n = 0;
  std::vector<std::vector<float>> kept;
  for (int call = 0; call < 2; call++) {
    const int rows = call == 0 ? n_rows : (n_rows > 7 ? 7 : 1), planes = call == 0 ? n_planes : 1, pt = call == 0 ? pitch : rows;
    const std::vector<float> x = obs_rows(od, rows, planes, pt, obs_pitch);
    kept.push_back(x);
    Dev<float> d_x(x);
    sag_obs_stats_desc d;
    memset(&d, 0, sizeof(d));
    d.n_rows = rows; d.n_planes = planes; d.pitch = pt; d.obs_pitch = obs_pitch; d.max_blocks = max_blocks; d.eps = eps;
    d.d_obs = d_x.p; d.d_state = d_state.p; d.d_table = d_table.p;
    const int rc = sag_obs_stats_device(g_ctx, &d);
    CHECK(rc == SAG_OK, "sag_obs_stats_device: %d %s", rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
    for (int p = 0; p < planes; p++)
      for (int r = 0; r < rows; r++) {
        for (int k = 0; k < od; k++) { const double v = x[((size_t)p * pt + r) * obs_pitch + k]; sum[k] += v; all.push_back(v); }
        n += 1;
      }
  }
  const auto s = d_state.get();
  const auto t = d_table.get();
  bool guards = true;
  for (int k = 0; k < GUARD; k++) guards = guards && s[1 + 2 * od + k] == (double)FILL && t[2 * od + k] == FILL;
  CHECK(guards, "stats od %d rows %d x %d: a guard word behind the state or the table was written", od, n_rows, n_planes);
  CHECK(s[0] == n, "stats od %d rows %d x %d: count %g for %g", od, n_rows, n_planes, s[0], n);
  for (int k = 0; k < od; k++) {
    const double mean = sum[k] / n;
    double m2 = 0;
    for (size_t i = k; i < all.size(); i += od) m2 += (all[i] - mean) * (all[i] - mean);
    const double sd = sqrt(m2 / n);
    CHECK(fabs(s[1 + k] - mean) <= 1e-5 * (sd > 0 ? sd : fabs(mean)) && fabs(s[1 + od + k] - m2) <= 1e-5 * m2 + 1e-30,
          "stats od %d rows %d x %d column %d: mean %g M2 %g for %g %g", od, n_rows, n_planes, k, s[1 + k], s[1 + od + k], mean, m2);
  }
  CHECK(table_is_of_state(s, t, od, eps), "stats od %d rows %d x %d: the table is not the header's expression of the state", od, n_rows, n_planes);
  // TABLE_ONLY: d_obs NULL, the state's bytes stay, the table comes back with the same bits
  Dev<float> d_t2(std::vector<float>(2 * od + GUARD, FILL));
  sag_obs_stats_desc d;
  memset(&d, 0, sizeof(d));
  d.flags = SAG_OBS_STATS_TABLE_ONLY; d.eps = eps; d.d_state = d_state.p; d.d_table = d_t2.p;
  const int rc = sag_obs_stats_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_obs_stats_device(TABLE_ONLY): %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto s2 = d_state.get();
  const auto t2 = d_t2.get();
  CHECK(memcmp(s2.data(), s.data(), s.size() * 8) == 0 && memcmp(t2.data(), t.data(), t.size() * 4) == 0, "TABLE_ONLY od %d: the state moved or the table differs", od);
}

struct Net {
  int od, nu, H, NO;
  std::vector<float> prm, table;
  Net(int od_, int nu_, int H_) : od(od_), nu(nu_), H(H_), NO(nu_ + 2) {
    const size_t np_ = (size_t)od * H + H + (size_t)H * H + H + (size_t)H * NO + NO + nu;
    prm.resize(np_);
    for (size_t k = 0; k < np_; k++) prm[k] = sym(0.2f);
    for (int u = 0; u < nu; u++) prm[np_ - nu + u] = 0.5f + 0.05f * u;
    table.resize(2 * od);
    for (int k = 0; k < od; k++) { table[k] = 1.3f * col_scale(k, od); table[od + k] = 1.0f / col_scale(k, od); }
  }
  // the rows of x (same layout) normalised under the table; NaN pads stay NaN
  std::vector<float> normalised(const std::vector<float>& x, int obs_pitch, float clip) const {
    std::vector<float> y = x;
    for (size_t i = 0; i < y.size(); i++) {
      const int k = (int)(i % obs_pitch);
      if (k < od && y[i] == y[i]) y[i] = norm_chain(x[i], table[k], table[od + k], clip);
    }
    return y;
  }
};

void forward_case(const Net& N, int rows, int activation, float clip) {
  const int od = N.od, nu = N.nu, obs_pitch = od + 4;
  const std::vector<float> x = obs_rows(od, rows, 1, rows, obs_pitch), xh = N.normalised(x, obs_pitch, clip);
  bool clamped = false;
  for (float v : xh) clamped = clamped || v == clip || v == -clip;
  Dev<float> d_prm(N.prm), d_table(N.table);
  std::vector<std::vector<float>> out[2];
  for (int norm = 0; norm < 2; norm++) {
    Dev<float> d_x(norm ? x : xh);
    Dev<float> d_a(std::vector<float>((size_t)rows * nu + GUARD, FILL)), d_l(std::vector<float>(rows + GUARD, FILL));
    Dev<float> d_v(std::vector<float>(rows + GUARD, FILL)), d_c(std::vector<float>(rows + GUARD, FILL));
    sag_policy_desc d;
    memset(&d, 0, sizeof(d));
    d.n_rows = rows; d.hidden = N.H; d.activation = activation; d.obs_pitch = obs_pitch; d.draw = 3; d.row0 = 1; d.logp_const = 0.25f;
    d.d_params = d_prm.p; d.d_obs = d_x.p; d.d_actions = d_a.p; d.d_logp = d_l.p; d.d_value = d_v.p; d.d_cvalue = d_c.p;
    const int rc = norm ? sag_policy_forward_norm_device(g_ctx, &d, d_table.p, clip) : sag_policy_forward_device(g_ctx, &d);
    CHECK(rc == SAG_OK, "forward (norm %d): %d %s", norm, rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
    out[norm] = {d_a.get(), d_l.get(), d_v.get(), d_c.get()};
  }
  for (int k = 0; k < 4; k++) {
    const auto &a = out[0][k], &b = out[1][k];
    CHECK(memcmp(a.data(), b.data(), a.size() * 4) == 0, "forward od %d H %d rows %d act %d output %d: norm differs from plain on normalised rows", od,
          N.H, rows, activation, k);
    bool guards = true;
    for (int g = 0; g < GUARD; g++) guards = guards && b[b.size() - 1 - g] == FILL;
    CHECK(guards && b[0] == b[0], "forward od %d rows %d output %d: a guard word was written or the output is NaN", od, rows, k);
  }
  CHECK(clamped || clip > 1e30f, "forward od %d rows %d: no element met the clamp", od, rows);
}

void backward_case(const Net& N, int n_rows, int n_planes, int pitch, int activation, int flags, float clip) {
  const int od = N.od, nu = N.nu;
  const size_t n_words = N.prm.size() + 8;
  const std::vector<float> x = obs_rows(od, n_rows, n_planes, pitch, od), xh = N.normalised(x, od, clip);
  const size_t span = (size_t)(n_planes - 1) * pitch + n_rows;
  auto plane = [&](int width, float scale, float off) {
    std::vector<float> v(span * width);
    for (size_t k = 0; k < v.size(); k++) v[k] = (int)((k / width) % pitch) < n_rows ? off + sym(scale) : nanf("");
    return v;
  };
  Dev<float> d_prm(N.prm), d_table(N.table), d_act(plane(nu, 0.8f, 0.0f)), d_lpo(plane(1, 0.3f, -1.5f * nu)), d_adv(plane(1, 1.0f, 0.0f));
  Dev<float> d_ret(plane(1, 1.0f, 0.0f)), d_cadv(plane(1, 1.0f, 0.0f)), d_cret(plane(1, 1.0f, 0.0f));
  std::vector<float> out[2];
  for (int norm = 0; norm < 2; norm++) {
    Dev<float> d_x(norm ? x : xh);
    Dev<float> d_grad(std::vector<float>(n_words + GUARD, flags ? 0.25f : FILL));
    sag_policy_grad_desc d;
    memset(&d, 0, sizeof(d));
    d.n_rows = n_rows; d.n_planes = n_planes; d.pitch = pitch; d.obs_pitch = od; d.hidden = N.H; d.activation = activation; d.flags = flags;
    d.clip = 0.2f; d.vf_coef = 0.5f; d.cvf_coef = 0.25f; d.ent_coef = 0.01f; d.adv_mul = 1.0f; d.adv_sub = 0.1f; d.cadv_mul = 0.5f; d.cadv_sub = -0.1f;
    d.scale = 1.0f / (float)(n_rows * n_planes);
    d.d_params = d_prm.p; d.d_obs = d_x.p; d.d_actions = d_act.p; d.d_logp_old = d_lpo.p; d.d_adv = d_adv.p; d.d_ret = d_ret.p;
    d.d_cadv = d_cadv.p; d.d_cret = d_cret.p; d.d_grad = d_grad.p;
    const int rc = norm ? sag_policy_backward_norm_device(g_ctx, &d, d_table.p, clip) : sag_policy_backward_device(g_ctx, &d);
    CHECK(rc == SAG_OK, "backward (norm %d): %d %s", norm, rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
    out[norm] = d_grad.get();
  }
  CHECK(memcmp(out[0].data(), out[1].data(), out[0].size() * 4) == 0, "backward od %d H %d act %d flags %d: norm differs from plain on normalised rows", od,
        N.H, activation, flags);
  bool guards = true, finite = true;
  for (size_t k = 0; k < n_words + GUARD; k++) {
    if (k >= n_words) guards = guards && out[1][k] == (flags ? 0.25f : FILL);
    else finite = finite && out[1][k] == out[1][k];
  }
  CHECK(guards && finite, "backward od %d H %d: a guard word behind d_grad was written (%d) or a word is NaN (%d)", od, N.H, (int)!guards, (int)!finite);
}

}  // namespace

int main() {
  static const int robots[3][3] = {{SAG_ROBOT_POINT, 60, 2}, {SAG_ROBOT_CAR, 72, 2}, {SAG_ROBOT_DOGGO, 104, 12}};
  for (const auto& rb : robots) {
    sag_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = SAG_ABI_VERSION; cfg.robot = rb[0]; cfg.n_envs = 8; cfg.device = 0;
    cfg.max_hazards = SAG_MAX_HAZARDS; cfg.max_vases = SAG_MAX_VASES; cfg.max_pillars = SAG_MAX_PILLARS; cfg.max_buttons = SAG_MAX_BUTTONS;
    cfg.has_box = 1; cfg.seed = 12345;
    int rc = sag_create(&cfg, &g_ctx);
    if (rc != SAG_OK) { printf("sag_create: %d %s (SAG_HOSTEMU=1 set?)\n", rc, sag_last_error(nullptr)); return 2; }
    const int od = rb[1], nu = rb[2];
    stats_case(od, 1, 1, 1, od, 0);
    stats_case(od, 33, 3, 38, od + 4, 0);
    stats_case(od, 1025, 3, 1025, od, 0);       // planes end inside a chunk
    stats_case(od, 2049, 1, 2049, od + 4, 2);   // three chunks on two blocks
    const Net net(od, nu, 32);
    for (int rows : {1, 33, 65})
      for (int act = 0; act < 2; act++) forward_case(net, rows, act, 2.0f);
    forward_case(net, 33, 1, INFINITY);
    for (int act = 0; act < 2; act++)
      for (int flags = 0; flags < 2; flags++) backward_case(net, 33, 3, 38, act, flags, 2.0f);
    sag_destroy(g_ctx);
  }
  if (g_failures) { printf("obs_norm_main: %d failures\n", g_failures); return 1; }
  printf("obs_norm_main: ok\n");
  return 0;
}
