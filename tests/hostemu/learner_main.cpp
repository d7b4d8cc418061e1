// learner_main.cpp - TEST INFRASTRUCTURE: sag_moments_device, sag_advantage_mix_device, sag_lagrange_device and
// sag_grad_clip_device of the host build of the device sources (tests/hostemu/build.py) driven from a program of its own, so
// that the whole process - this file and the library - runs under AddressSanitizer and UndefinedBehaviorSanitizer
// (test_learner_kernels_hostemu.py compiles and runs it).  "Device" memory is malloc'ed there.  Every input is allocated at
// its exact size - three planes whose last counted row ends the allocation, so a read of a pad row or of another column
// behind it is a heap overflow - and every output has guard words behind it that must keep their fill.  The reductions are
// compared with plain loops in double precision (1e-5 relative: fp32 sums of <= 12 300 terms of one sign stay below 1e-6, a
// dropped element costs >= 1 / 12 300), the mix and the multiplier bit for bit with the header's chains.
// Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "learner_main: ok" on success.
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

bool guards_ok(const std::vector<float>& v, size_t words) {
  for (size_t k = words; k < v.size(); k++)
    if (v[k] != FILL) return false;
  return true;
}

// element (p, r) at (p * pitch + r) * stride; the array ends with the last counted element, everything else is NaN
size_t span_floats(int n_rows, int n_planes, int pitch, int stride) { return ((size_t)(n_planes - 1) * pitch + n_rows - 1) * stride + 1; }

void moments_case(int n_rows, int n_planes, int pitch, int stride, bool masked, int max_blocks) {
  std::vector<float> x(span_floats(n_rows, n_planes, pitch, stride), NAN);
  std::vector<uint8_t> mask(span_floats(n_rows, n_planes, pitch, 1), 1);   // ends with the last counted row's byte
  double sum = 0, cnt = 0;
  std::vector<double> kept;
  for (int p = 0; p < n_planes; p++)
    for (int r = 0; r < n_rows; r++) {
      const size_t o = (size_t)p * pitch + r;
      const bool keep = !masked || (rnd() % 3 == 0);
      mask[o] = keep ? (uint8_t)(1 + rnd() % 255) : 0;
      if (keep) { x[o * stride] = 2.0f + sym(3.0f); kept.push_back(x[o * stride]); sum += x[o * stride]; cnt += 1; }
    }
  const float eps = 1e-3f;
  const double mean = cnt > 0 ? sum / cnt : 0;
  double sq = 0;
  for (double v : kept) sq += (v - mean) * (v - mean);
  const double var = cnt > 0 ? sq / cnt : 0, rstd = cnt > 0 ? 1.0 / (sqrt(var) + (double)eps) : 0;
  Dev<float> d_x(x);
  Dev<uint8_t> d_m(mask);
  Dev<float> d_o(std::vector<float>(4 + GUARD, FILL));
  sag_moments_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = n_rows; d.n_planes = n_planes; d.pitch = pitch; d.stride = stride; d.max_blocks = max_blocks; d.eps = eps;
  d.d_x = d_x.p; d.d_mask = masked ? d_m.p : nullptr; d.d_out = d_o.p;
  const int rc = sag_moments_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_moments_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto o = d_o.get();
  CHECK(guards_ok(o, 4), "moments %d x %d: a guard word was written", n_rows, n_planes);
  CHECK(o[0] == (float)cnt, "moments %d x %d stride %d: count %g for %g", n_rows, n_planes, stride, (double)o[0], cnt);
  const double sd = sqrt(var) > 0 ? sqrt(var) : 1.0;
  CHECK(fabs(o[1] - mean) <= 1e-5 * sd && fabs(o[2] - var) <= 1e-5 * (var > 0 ? var : 1) && fabs(o[3] - rstd) <= 1e-5 * (rstd > 0 ? rstd : 1),
        "moments %d x %d stride %d masked %d: {%g %g %g} for {%g %g %g}", n_rows, n_planes, stride, (int)masked, (double)o[1], (double)o[2],
        (double)o[3], mean, var, rstd);
}

float norm_chain(float x, int mode, float m, float s) {
  if (mode >= 1) { volatile float t = x - m; x = t; }
  if (mode == 2) { volatile float t = x * s; x = t; }
  return x;
}

void mix_case(int n_rows, int n_planes, int pitch, int adv_mode, int cadv_mode, bool cost, bool lam_dev) {
  const size_t n = span_floats(n_rows, n_planes, pitch, 1);
  std::vector<float> adv(n, NAN), cadv(n, NAN), want(n + GUARD, FILL);
  const std::vector<float> ma = {99.0f, 0.37f, 2.0f, 0.71f}, mc = {99.0f, 4.1f, 9.0f, 0.332f}, lam = {0.613f};
  for (int p = 0; p < n_planes; p++)
    for (int r = 0; r < n_rows; r++) {
      const size_t o = (size_t)p * pitch + r;
      adv[o] = sym(3.0f); cadv[o] = 4.0f + sym(9.0f);
      const float a = norm_chain(adv[o], adv_mode, ma[1], ma[3]), c = norm_chain(cadv[o], cadv_mode, mc[1], mc[3]);
      volatile float t = lam[0] * c;
      volatile float w = a - t;
      want[o] = cost ? w : a;
    }
  Dev<float> d_a(adv), d_c(cadv), d_ma(ma), d_mc(mc), d_l(lam);
  Dev<float> d_o(std::vector<float>(n + GUARD, FILL));
  sag_advantage_mix_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = n_rows; d.n_planes = n_planes; d.pitch = pitch; d.adv_mode = adv_mode; d.cadv_mode = cadv_mode;
  d.cost_weight = lam_dev ? 55.0f : lam[0];
  d.d_adv = d_a.p; d.d_cadv = cost ? d_c.p : nullptr; d.d_adv_mom = d_ma.p; d.d_cadv_mom = d_mc.p; d.d_lambda = lam_dev ? d_l.p : nullptr;
  d.d_out = d_o.p;
  const int rc = sag_advantage_mix_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_advantage_mix_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto o = d_o.get();
  CHECK(memcmp(o.data(), want.data(), o.size() * 4) == 0, "mix %d x %d pitch %d modes %d %d cost %d: differs from the chain, or a pad row or guard was written",
        n_rows, n_planes, pitch, adv_mode, cadv_mode, (int)cost);
}

void lagrange_case() {
  const float moms[5][4] = {{12, 28.37f, 1, 1}, {7, 23.9f, 2, 0.5f}, {0, 0, 0, 0}, {3, 2.125f, 0, 1}, {40, 61.03f, 9, 0.3f}};
  std::vector<float> st(4 + GUARD, FILL);
  st[0] = 0.1f; st[1] = st[2] = st[3] = 0.0f;
  Dev<float> d_s(st);
  const float lr = 0.05f, budget = 25.0f, cap = 0.5f;
  for (const auto& m : moms) {
    Dev<float> d_m(std::vector<float>(m, m + 4));
    sag_lagrange_desc d;
    memset(&d, 0, sizeof(d));
    d.lr = lr; d.budget = budget; d.lambda_max = cap; d.d_mom = d_m.p; d.d_state = d_s.p;
    const int rc = sag_lagrange_device(g_ctx, &d);
    CHECK(rc == SAG_OK, "sag_lagrange_device: %d %s", rc, sag_last_error(g_ctx));
    sag_wait(g_ctx);
    if (m[0] > 0) {
      volatile float dd = m[1] - budget;
      volatile float step = lr * dd;
      float t = st[0] + step;
      t = t > 0.0f ? t : 0.0f;
      t = t < cap ? t : cap;
      st[0] = t; st[1] = m[1]; st[2] = m[0]; st[3] += 1.0f;
    } else {
      st[2] = 0.0f;
    }
    const auto o = d_s.get();
    CHECK(memcmp(o.data(), st.data(), o.size() * 4) == 0, "lagrange: {%g %g %g %g} for {%g %g %g %g}", (double)o[0], (double)o[1], (double)o[2],
          (double)o[3], (double)st[0], (double)st[1], (double)st[2], (double)st[3]);
  }
}

void clip_case(int n, float max_scale, int max_blocks) {
  std::vector<float> g(n + 8 + GUARD, FILL);
  double ss = 0;
  for (int k = 0; k < n; k++) { g[k] = sym(0.05f); ss += (double)g[k] * g[k]; }
  const double norm = sqrt(ss);
  Dev<float> d_g(std::vector<float>(g.begin(), g.end()));
  Dev<float> d_o(std::vector<float>(2 + GUARD, FILL));
  sag_grad_clip_desc d;
  memset(&d, 0, sizeof(d));
  d.n = n; d.max_blocks = max_blocks; d.max_norm = (float)(max_scale * norm); d.d_grad = d_g.p; d.d_out = d_o.p;
  const int rc = sag_grad_clip_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_grad_clip_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto o = d_o.get(), got = d_g.get();
  CHECK(guards_ok(o, 2), "clip %d: a guard word behind d_out was written", n);
  CHECK(fabs(o[0] - norm) <= 1e-5 * norm, "clip %d: norm %g for %g", n, (double)o[0], norm);
  if (max_scale > 1.0f) CHECK(o[1] == 1.0f, "clip %d: factor %g, expected 1", n, (double)o[1]);
  else CHECK(o[1] < 1.0f && fabs(o[1] - d.max_norm / (norm + 1e-6)) <= 1e-5 * o[1], "clip %d: factor %g for %g", n, (double)o[1], d.max_norm / (norm + 1e-6));
  for (int k = 0; k < n; k++) {
    volatile float w = g[k] * o[1];
    g[k] = o[1] == 1.0f ? g[k] : w;
  }
  CHECK(memcmp(got.data(), g.data(), got.size() * 4) == 0, "clip %d: an element is not fl(g * factor), or a word behind n was written", n);
}

}  // namespace

int main() {
  sag_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = SAG_ABI_VERSION; cfg.robot = SAG_ROBOT_POINT; cfg.n_envs = 8; cfg.device = 0;
  cfg.max_hazards = SAG_MAX_HAZARDS; cfg.max_vases = SAG_MAX_VASES; cfg.max_pillars = SAG_MAX_PILLARS; cfg.max_buttons = SAG_MAX_BUTTONS;
  cfg.has_box = 1; cfg.seed = 12345;
  int rc = sag_create(&cfg, &g_ctx);
  if (rc != SAG_OK) { printf("sag_create: %d %s (SAG_HOSTEMU=1 set?)\n", rc, sag_last_error(nullptr)); return 2; }
  for (int masked = 0; masked < 2; masked++) {
    moments_case(1, 1, 1, 1, masked, 0);
    moments_case(33, 3, 38, 1, masked, 0);
    moments_case(33, 3, 40, 4, masked, 0);       // episode rows: the cost column
    moments_case(64, 3, 64, 1, masked, 0);       // every quad one 16-byte load
    moments_case(4099, 3, 4100, 1, masked, 0);   // three chunks; planes end inside a quad
    moments_case(4099, 3, 4099, 1, masked, 2);   // two blocks, the first takes a second chunk
  }
  for (int am = 0; am < 3; am++)
    for (int cm = 0; cm < 3; cm++) {
      mix_case(33, 3, 38, am, cm, true, cm == 1);
      mix_case(64, 3, 64, am, cm, true, cm != 1);
    }
  mix_case(33, 3, 38, 2, 0, false, false);
  mix_case(64, 3, 64, 1, 0, false, true);
  lagrange_case();
  for (int n : {1, 33, 3142, 2 * 4096 + 1}) {
    clip_case(n, 2.0f, 0);
    clip_case(n, 0.5f, n > 4096 ? 2 : 0);
  }
  sag_destroy(g_ctx);
  if (g_failures) { printf("learner_main: %d failures\n", g_failures); return 1; }
  printf("learner_main: ok\n");
  return 0;
}
