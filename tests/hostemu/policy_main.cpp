// policy_main.cpp - TEST INFRASTRUCTURE: sag_policy_forward_device of the host build of the device sources
// (tests/hostemu/build.py) driven from a program of its own, so that the whole process - this file and the library - runs under
// AddressSanitizer and UndefinedBehaviorSanitizer (test_policy_hostemu.py compiles and runs it).  "Device" memory is malloc'ed
// there and every array below is allocated at its exact size: the observations end with their last element, every output has a
// block of guard rows behind it that must keep its fill.  The results are compared bit for bit with the plain loops of the
// header's chain in this file.  Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "policy_main: ok" on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sag.h"

namespace {

constexpr int GUARD = 5;   // rows behind every output
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

// y[j] = act(b[j] + sum over ascending k of x[k] W[k][j]), every step one fmaf
void layer(const float* x, int K, const float* W, const float* b, int J, bool relu, float* y) {
  for (int j = 0; j < J; j++) {
    float acc = b[j];
    for (int k = 0; k < K; k++) acc = fmaf(x[k], W[(size_t)k * J + j], acc);
    y[j] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
  }
}

void forward_case(int od, int nu, int H, int rows, int pad) {
  const int NO = nu + 2, pitch = od + pad;
  std::vector<float> prm((size_t)od * H + H + (size_t)H * H + H + (size_t)H * NO + NO + nu);
  for (auto& w : prm) w = sym(0.3f);
  for (int u = 0; u < nu; u++) prm[prm.size() - nu + u] = 0.5f + 0.1f * u;
  // the last row ends with its last element: no pad behind it
  std::vector<float> obs((size_t)(rows - 1) * pitch + od);
  for (size_t k = 0; k < obs.size(); k++) obs[k] = (int)(k % pitch) < od ? sym(1.5f) : nanf("");
  const float fill = 7.0f;
  Dev<float> d_prm(prm), d_obs(obs), d_act(std::vector<float>((size_t)(rows + GUARD) * nu, fill)), d_logp(std::vector<float>(rows + GUARD, fill)),
      d_val(std::vector<float>(rows + GUARD, fill)), d_cval(std::vector<float>(rows + GUARD, fill));
  sag_policy_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = rows; d.hidden = H; d.activation = SAG_POLICY_RELU; d.flags = SAG_POLICY_MEAN; d.obs_pitch = pitch;
  d.logp_const = 1.5f; d.d_params = d_prm.p; d.d_obs = d_obs.p; d.d_actions = d_act.p; d.d_logp = d_logp.p; d.d_value = d_val.p; d.d_cvalue = d_cval.p;
  int rc = sag_policy_forward_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_policy_forward_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto act = d_act.get(), logp = d_logp.get(), val = d_val.get(), cval = d_cval.get();
  const float *W1 = prm.data(), *b1 = W1 + (size_t)od * H, *W2 = b1 + H, *b2 = W2 + (size_t)H * H, *W3 = b2 + H, *b3 = W3 + (size_t)H * NO;
  std::vector<float> h1(H), h2(H), o(NO);
  for (int i = 0; i < rows; i++) {
    layer(&obs[(size_t)i * pitch], od, W1, b1, H, true, h1.data());
    layer(h1.data(), H, W2, b2, H, true, h2.data());
    layer(h2.data(), H, W3, b3, NO, false, o.data());
    CHECK(memcmp(&act[(size_t)i * nu], o.data(), nu * sizeof(float)) == 0, "od %d H %d rows %d pad %d: mean of row %d differs", od, H, rows, pad, i);
    CHECK(memcmp(&val[i], &o[nu], 4) == 0 && memcmp(&cval[i], &o[nu + 1], 4) == 0, "od %d H %d rows %d pad %d: values of row %d differ", od, H, rows, pad, i);
    CHECK(logp[i] == -1.5f, "row %d: logp %g", i, (double)logp[i]);
  }
  for (int i = rows; i < rows + GUARD; i++) {
    CHECK(logp[i] == fill && val[i] == fill && cval[i] == fill, "od %d H %d rows %d: guard row %d was written", od, H, rows, i);
    for (int u = 0; u < nu; u++) CHECK(act[(size_t)i * nu + u] == fill, "od %d H %d rows %d: guard action row %d was written", od, H, rows, i);
  }
  CHECK(d_obs.get().size() == obs.size() && memcmp(d_obs.get().data(), obs.data(), obs.size() * 4) == 0, "the observations changed");
  // sampled, and with each output left out in turn: every index of the sampling path under the sanitizers
  d.flags = 0; d.draw = 9; d.row0 = 0xfffffff0u;
  for (int drop = 0; drop < 5; drop++) {
    sag_policy_desc e = d;
    if (drop == 1) e.d_actions = nullptr;
    if (drop == 2) e.d_logp = nullptr;
    if (drop == 3) e.d_value = nullptr;
    if (drop == 4) e.d_cvalue = nullptr;
    rc = sag_policy_forward_device(g_ctx, &e);
    CHECK(rc == SAG_OK, "sampled, drop %d: %d %s", drop, rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
  }
  const auto a2 = d_act.get(), v2 = d_val.get();
  int moved = 0;
  for (int i = 0; i < rows * nu; i++) moved += a2[i] != act[i] && isfinite(a2[i]);
  CHECK(moved * 10 > rows * nu * 9, "sampled actions: %d of %d differ from the mean", moved, rows * nu);
  CHECK(memcmp(v2.data(), val.data(), v2.size() * 4) == 0, "sampling changed the values");
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
    for (int H : {32, 96})
      for (int rows : {1, 33, 130}) {
        if (rb[0] != SAG_ROBOT_POINT && rows == 130 && H == 96) continue;   // the largest case once
        forward_case(rb[1], rb[2], H, rows, 0);
      }
    forward_case(rb[1], rb[2], 32, 33, 4);   // a pitched input
    sag_destroy(g_ctx);
  }
  if (g_failures) { printf("policy_main: %d failures\n", g_failures); return 1; }
  printf("policy_main: ok\n");
  return 0;
}
