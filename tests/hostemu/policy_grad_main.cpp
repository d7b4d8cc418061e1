// policy_grad_main.cpp - TEST INFRASTRUCTURE: sag_policy_backward_device and sag_adam_device of the host build of the device
// sources (tests/hostemu/build.py) driven from a program of its own, so that the whole process - this file and the library -
// runs under AddressSanitizer and UndefinedBehaviorSanitizer (test_policy_grad_hostemu.py compiles and runs it).  "Device"
// memory is malloc'ed there.  Every input is allocated at its exact size - the last plane ends with its last row, so a read of
// a pad row behind it is a heap overflow - and every output (the gradient, the parameters and both moments) has guard words
// behind it that must keep their fill.  The gradient is compared with plain loops in double precision over the forward's own
// fp32 activations (the fmaf chains of the header): 1e-4 of a tensor's largest entry, where fp32 sums of <= 390 terms stay
// below 1e-5 and a misplaced row or column costs at least 1 / 390.  Adam is compared bit for bit with the header's chain.
// Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "policy_grad_main: ok" on success.
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

void layer(const float* x, int K, const float* W, const float* b, int J, bool relu, float* y) {
  for (int j = 0; j < J; j++) {
    float acc = b[j];
    for (int k = 0; k < K; k++) acc = fmaf(x[k], W[(size_t)k * J + j], acc);
    y[j] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
  }
}

// a [planes][pitch] array of `width` floats per row, cut behind row n_rows - 1 of the last plane; pad rows are NaN
std::vector<float> planes(int n_planes, int n_rows, int pitch, int width, float scale, float offset = 0.0f) {
  std::vector<float> v(((size_t)(n_planes - 1) * pitch + n_rows) * width);
  for (size_t k = 0; k < v.size(); k++) v[k] = (int)((k / width) % pitch) < n_rows ? offset + sym(scale) : nanf("");
  return v;
}

void grad_case(int od, int nu, int H, int n_rows, int n_planes) {
  const int NO = nu + 2, pitch = n_rows + 3, total = n_rows * n_planes;
  const size_t oW1 = 0, ob1 = (size_t)od * H, oW2 = ob1 + H, ob2 = oW2 + (size_t)H * H, oW3 = ob2 + H, ob3 = oW3 + (size_t)H * NO, ostd = ob3 + NO,
               np_ = ostd + nu;
  std::vector<float> prm(np_);
  for (auto& w : prm) w = sym(0.3f);
  for (int u = 0; u < nu; u++) prm[ostd + u] = 0.6f + 0.05f * u;
  auto obs = planes(n_planes, n_rows, pitch, od, 1.5f), act = planes(n_planes, n_rows, pitch, nu, 1.0f), lpo = planes(n_planes, n_rows, pitch, 1, 0.3f),
       adv = planes(n_planes, n_rows, pitch, 1, 1.0f), ret = planes(n_planes, n_rows, pitch, 1, 1.0f), cadv = planes(n_planes, n_rows, pitch, 1, 1.0f),
       cret = planes(n_planes, n_rows, pitch, 1, 1.0f);
  sag_policy_grad_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = n_rows; d.n_planes = n_planes; d.pitch = pitch; d.obs_pitch = od; d.hidden = H; d.activation = SAG_POLICY_RELU;
  d.clip = 0.2f; d.vf_coef = 0.5f; d.cvf_coef = 0.25f; d.ent_coef = 0.01f; d.adv_mul = 1.0f; d.adv_sub = 0.1f; d.cadv_mul = 0.5f; d.cadv_sub = -0.1f;
  d.scale = 1.0f / (float)total;
  // logp_old near the new logp, so that the ratios are of order one: logp of these actions, in double, plus the draw above
  const float *W1 = &prm[oW1], *b1 = &prm[ob1], *W2 = &prm[oW2], *b2 = &prm[ob2], *W3 = &prm[oW3], *b3 = &prm[ob3], *sd = &prm[ostd];
  std::vector<float> h1((size_t)total * H), h2((size_t)total * H), o((size_t)total * NO);
  std::vector<double> logp(total);
  std::vector<size_t> src(total);
  for (int g = 0; g < total; g++) {
    src[g] = (size_t)(g / n_rows) * pitch + g % n_rows;
    layer(&obs[src[g] * od], od, W1, b1, H, true, &h1[(size_t)g * H]);
    layer(&h1[(size_t)g * H], H, W2, b2, H, true, &h2[(size_t)g * H]);
    layer(&h2[(size_t)g * H], H, W3, b3, NO, false, &o[(size_t)g * NO]);
    double lp = -0.5 * nu * log(2 * M_PI);
    for (int u = 0; u < nu; u++) {
      const double z = ((double)act[src[g] * nu + u] - o[(size_t)g * NO + u]) / sd[u];
      lp += -0.5 * z * z - log((double)sd[u]);
    }
    logp[g] = lp;
    lpo[src[g]] = (float)(lp + lpo[src[g]]);
  }
  Dev<float> d_prm(prm), d_obs(obs), d_act(act), d_lpo(lpo), d_adv(adv), d_ret(ret), d_cadv(cadv), d_cret(cret),
      d_grad(std::vector<float>(np_ + 8 + GUARD, FILL));
  d.d_params = d_prm.p; d.d_obs = d_obs.p; d.d_actions = d_act.p; d.d_logp_old = d_lpo.p; d.d_adv = d_adv.p; d.d_ret = d_ret.p;
  d.d_cadv = d_cadv.p; d.d_cret = d_cret.p; d.d_grad = d_grad.p;
  int rc = sag_policy_backward_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_policy_backward_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto got = d_grad.get();
  for (int k = 0; k < GUARD; k++) CHECK(got[np_ + 8 + k] == FILL, "od %d H %d rows %d: guard word %d behind d_grad was written", od, H, n_rows, k);

  // the header's function, in double, over the fp32 activations
  std::vector<double> ref(np_ + 8, 0.0), dO(NO), dz2(H), dz1(H);
  for (int g = 0; g < total; g++) {
    const float *x = &obs[src[g] * od], *a1 = &h1[(size_t)g * H], *a2 = &h2[(size_t)g * H], *og = &o[(size_t)g * NO];
    const double rho = exp(logp[g] - (double)lpo[src[g]]);
    const double A = (double)d.adv_mul * ((double)adv[src[g]] - d.adv_sub) - (double)d.cadv_mul * ((double)cadv[src[g]] - d.cadv_sub);
    const double lo = 1.0 - (double)d.clip, hi = 1.0 + (double)d.clip;
    const bool live = (A >= 0 && rho <= hi) || (A < 0 && rho >= lo);
    const double dlp = live ? -rho * A : 0.0;
    for (int u = 0; u < nu; u++) {
      const double z = ((double)act[src[g] * nu + u] - og[u]) / sd[u];
      dO[u] = dlp * z / sd[u];
      ref[ostd + u] += dlp * (z * z - 1.0) / sd[u] - (double)d.ent_coef / sd[u];
    }
    const double ev = (double)og[nu] - ret[src[g]], ec = (double)og[nu + 1] - cret[src[g]];
    dO[nu] = (double)d.vf_coef * ev; dO[nu + 1] = (double)d.cvf_coef * ec;
    ref[np_ + 0] += -(live ? rho : fmin(fmax(rho, lo), hi)) * A; ref[np_ + 1] += 0.5 * ev * ev; ref[np_ + 2] += 0.5 * ec * ec;
    ref[np_ + 3] += (double)lpo[src[g]] - logp[g]; ref[np_ + 4] += live ? 0.0 : 1.0; ref[np_ + 5] += 1.0;
    for (int i = 0; i < H; i++) {
      double s = 0.0;
      for (int j = 0; j < NO; j++) { s += (double)W3[(size_t)i * NO + j] * dO[j]; ref[oW3 + (size_t)i * NO + j] += (double)a2[i] * dO[j]; }
      dz2[i] = a2[i] > 0.0f ? s : 0.0;
    }
    for (int j = 0; j < NO; j++) ref[ob3 + j] += dO[j];
    for (int i = 0; i < H; i++) {
      double s = 0.0;
      for (int j = 0; j < H; j++) { s += (double)W2[(size_t)i * H + j] * dz2[j]; ref[oW2 + (size_t)i * H + j] += (double)a1[i] * dz2[j]; }
      dz1[i] = a1[i] > 0.0f ? s : 0.0;
      ref[ob2 + i] += dz2[i];
    }
    for (int j = 0; j < H; j++) {
      ref[ob1 + j] += dz1[j];
      for (int k = 0; k < od; k++) ref[oW1 + (size_t)k * H + j] += (double)x[k] * dz1[j];
    }
  }
  const size_t bounds[9] = {oW1, ob1, oW2, ob2, oW3, ob3, ostd, np_, np_ + 8};
  for (int t = 0; t < 8; t++) {
    double top = 0.0, err = 0.0;
    for (size_t k = bounds[t]; k < bounds[t + 1]; k++) {
      const double r = ref[k] * (double)d.scale;
      top = fmax(top, fabs(r));
      err = fmax(err, fabs((double)got[k] - r));
      CHECK(isfinite(got[k]), "od %d H %d rows %d x %d: word %zu is not finite", od, H, n_rows, n_planes, k);
    }
    CHECK(err <= 1e-4 * top, "od %d H %d rows %d x %d: tensor %d differs by %.3g of %.3g", od, H, n_rows, n_planes, t, err, top);
  }
  const auto obs2 = d_obs.get();
  CHECK(memcmp(obs2.data(), obs.data(), obs.size() * 4) == 0, "the observations changed");

  // Adam on that gradient, three steps, the std entries clamped; guard words behind the parameters and both moments
  std::vector<float> p0(prm), m0(np_, 0.0f), v0(np_, 0.0f);
  p0.resize(np_ + GUARD, FILL); m0.resize(np_ + GUARD, FILL); v0.resize(np_ + GUARD, FILL);
  Dev<float> d_p(p0), d_m(m0), d_v(v0);
  sag_adam_desc a;
  memset(&a, 0, sizeof(a));
  a.n = (int)np_; a.clamp_first = (int)(np_ - nu); a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f; a.clamp_lo = 0.62f;
  a.d_param = d_p.p; a.d_grad = d_grad.p; a.d_m = d_m.p; a.d_v = d_v.p;
  for (int t = 1; t <= 3; t++) {
    a.step = (float)(3e-2 * sqrt(1.0 - pow(0.999, t)) / (1.0 - pow(0.9, t)));
    rc = sag_adam_device(g_ctx, &a);
    CHECK(rc == SAG_OK, "sag_adam_device: %d %s", rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
    const float o1 = 1.0f - a.beta1, o2 = 1.0f - a.beta2;
    for (size_t k = 0; k < np_; k++) {
      const float gk = got[k];
      volatile float t0 = a.beta1 * m0[k], t1 = o1 * gk; const float m = t0 + t1;
      volatile float u0 = a.beta2 * v0[k], u1 = o2 * gk, u2 = u1 * gk; const float v = u0 + u2;
      volatile float den = sqrtf(v) + a.eps, num = a.step * m, q = num / den;
      float pn = p0[k] - q;
      if ((int)k >= a.clamp_first) pn = pn > a.clamp_lo ? pn : a.clamp_lo;
      m0[k] = m; v0[k] = v; p0[k] = pn;
    }
    const auto p1 = d_p.get(), m1 = d_m.get(), v1 = d_v.get();
    CHECK(memcmp(p1.data(), p0.data(), (np_ + GUARD) * 4) == 0 && memcmp(m1.data(), m0.data(), (np_ + GUARD) * 4) == 0 &&
              memcmp(v1.data(), v0.data(), (np_ + GUARD) * 4) == 0,
          "od %d H %d rows %d: Adam step %d differs from the chain, or a guard word was written", od, H, n_rows, t);
  }
  for (int u = 0; u < nu; u++) CHECK(p0[ostd + u] >= a.clamp_lo, "std[%d] = %g below the clamp", u, (double)p0[ostd + u]);
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
        grad_case(rb[1], rb[2], H, rows, 1);
      }
    grad_case(rb[1], rb[2], 32, 33, 3);   // three planes, tiles that straddle them, the allocation ends with the last row
    sag_destroy(g_ctx);
  }
  if (g_failures) { printf("policy_grad_main: %d failures\n", g_failures); return 1; }
  printf("policy_grad_main: ok\n");
  return 0;
}
