// shuffle_main.cpp - TEST INFRASTRUCTURE: sag_permutation_device and sag_policy_backward_rows_device of the host build of the
// device sources (tests/hostemu/build.py) driven from a program of its own, so that the whole process - this file and the
// library - runs under AddressSanitizer and UndefinedBehaviorSanitizer (test_shuffle_hostemu.py compiles and runs it).
// "Device" memory is malloc'ed there.
//   * the permutation at n = 1, 33 and 4097 into an array of exactly n words - a store at or behind d_index + n is a heap
//     overflow -, compared with the header's definition restated here (Philox4x32-10, six Feistel rounds, cycle walking) and
//     checked to be a bijection;
//   * the rows backward with lists of 1, 33 and 97 entries, entries outside the planes among them, over planes allocated at
//     their exact size - the last plane ends with its last row, so a read of a pad row behind it, or of a row that an
//     out-of-range entry names, is a heap overflow.  The gradient is compared with plain loops in double precision over the
//     forward's own fp32 activations, on the valid entries of the list: 1e-4 of a tensor's largest entry, where fp32 sums of
//     <= 97 terms stay below 1e-5 and a misplaced row costs at least 1 / 97.  Statistic 5 is the count of the valid entries.
// Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "shuffle_main: ok" on success.
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
constexpr uint64_t SEED = 0x1234567800000abcull;
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

// ---- the permutation, from the header's text -------------------------------------------------------------------------
uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

uint32_t pi_ref(uint32_t i, uint32_t n, uint32_t draw) {
  int b = 0;
  for (uint32_t m = n - 1; m; m >>= 1) b++;
  if (b < 2) b = 2;
  uint32_t x = i;
  do {
    int wl = b / 2, wr = b - wl;
    uint32_t L = x >> wr, R = x & ((1u << wr) - 1u);
    for (uint32_t r = 0; r < 6; r++) {
      const uint32_t f = philox_word0(R, draw, r, 0x18000000u, (uint32_t)SEED, (uint32_t)(SEED >> 32)) & ((1u << wl) - 1u);
      const uint32_t t = L ^ f;
      L = R; R = t;
      const int w = wl; wl = wr; wr = w;
    }
    x = (L << wr) | R;
  } while (x >= n);
  return x;
}

void permutation_case(int n, uint32_t draw) {
  Dev<int32_t> d(std::vector<int32_t>((size_t)n, -77));   // exactly n words
  const int rc = sag_permutation_device(g_ctx, n, draw, d.p);
  CHECK(rc == SAG_OK, "sag_permutation_device(%d): %d %s", n, rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto got = d.get();
  std::vector<char> seen((size_t)n, 0);
  for (int i = 0; i < n; i++) {
    CHECK(got[i] >= 0 && got[i] < n && !seen[got[i] < 0 || got[i] >= n ? 0 : got[i]], "n %d: entry %d = %d is out of range or taken twice", n, i, got[i]);
    if (got[i] >= 0 && got[i] < n) seen[got[i]] = 1;
    CHECK((uint32_t)got[i] == pi_ref((uint32_t)i, (uint32_t)n, draw), "n %d draw %u: entry %d = %d, the definition gives %u", n, draw, i, got[i],
          pi_ref((uint32_t)i, (uint32_t)n, draw));
  }
}

// ---- the rows backward -----------------------------------------------------------------------------------------------
void layer(const float* x, int K, const float* W, const float* b, int J, bool relu, float* y) {
  for (int j = 0; j < J; j++) {
    float acc = b[j];
    for (int k = 0; k < K; k++) acc = fmaf(x[k], W[(size_t)k * J + j], acc);
    y[j] = relu ? (acc > 0.0f ? acc : 0.0f) : acc;
  }
}

// a [planes][pitch] array of `width` floats per row, cut behind row n_rows - 1 of the last plane; pad rows are NaN
std::vector<float> planes(int n_planes, int n_rows, int pitch, int width, float scale) {
  std::vector<float> v(((size_t)(n_planes - 1) * pitch + n_rows) * width);
  for (size_t k = 0; k < v.size(); k++) v[k] = (int)((k / width) % pitch) < n_rows ? sym(scale) : nanf("");
  return v;
}

// a list of `len` entries over `total` logical elements: the last element first (its row ends the allocation), draws with
// repetition, and - with `bad` - entries outside [0, total) at both ends and inside
std::vector<int32_t> row_list(int len, int total, bool bad) {
  std::vector<int32_t> r((size_t)len);
  for (int j = 0; j < len; j++) r[j] = (int32_t)(rnd() % (uint32_t)total);
  r[0] = total - 1;
  if (bad) {
    const int32_t out[6] = {-1, total, INT32_MAX, INT32_MIN, total + 1, -total};
    for (int k = 0; k < 6; k++) r[(size_t)(5 * k + 2)] = out[k];   // entries 2, 7, ..., 27: len >= 33
    r[(size_t)len - 1] = total;
  }
  return r;
}

void rows_case(int od, int nu, int H, int n_rows, int n_planes, int len, bool bad) {
  const int NO = nu + 2, pitch = n_rows + 3, total = n_rows * n_planes;
  const size_t oW1 = 0, ob1 = (size_t)od * H, oW2 = ob1 + H, ob2 = oW2 + (size_t)H * H, oW3 = ob2 + H, ob3 = oW3 + (size_t)H * NO, ostd = ob3 + NO,
               np_ = ostd + nu;
  std::vector<float> prm(np_);
  for (auto& w : prm) w = sym(0.3f);
  for (int u = 0; u < nu; u++) prm[ostd + u] = 0.6f + 0.05f * u;
  auto obs = planes(n_planes, n_rows, pitch, od, 1.5f), act = planes(n_planes, n_rows, pitch, nu, 1.0f), lpo = planes(n_planes, n_rows, pitch, 1, 0.3f),
       adv = planes(n_planes, n_rows, pitch, 1, 1.0f), ret = planes(n_planes, n_rows, pitch, 1, 1.0f), cadv = planes(n_planes, n_rows, pitch, 1, 1.0f),
       cret = planes(n_planes, n_rows, pitch, 1, 1.0f);
  const auto list = row_list(len, total, bad);
  sag_policy_grad_desc d;
  memset(&d, 0, sizeof(d));
  d.n_rows = n_rows; d.n_planes = n_planes; d.pitch = pitch; d.obs_pitch = od; d.hidden = H; d.activation = SAG_POLICY_RELU;
  d.clip = 0.2f; d.vf_coef = 0.5f; d.cvf_coef = 0.25f; d.ent_coef = 0.01f; d.adv_mul = 1.0f; d.adv_sub = 0.1f; d.cadv_mul = 0.5f; d.cadv_sub = -0.1f;
  d.scale = 1.0f / (float)len;
  const float *W1 = &prm[oW1], *b1 = &prm[ob1], *W2 = &prm[oW2], *b2 = &prm[ob2], *W3 = &prm[oW3], *b3 = &prm[ob3], *sd = &prm[ostd];
  // per logical element: the forward, and logp_old near the new logp so that the ratios are of order one
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
  Dev<int32_t> d_list(list);   // exactly `len` entries
  d.d_params = d_prm.p; d.d_obs = d_obs.p; d.d_actions = d_act.p; d.d_logp_old = d_lpo.p; d.d_adv = d_adv.p; d.d_ret = d_ret.p;
  d.d_cadv = d_cadv.p; d.d_cret = d_cret.p; d.d_grad = d_grad.p;
  const int rc = sag_policy_backward_rows_device(g_ctx, &d, d_list.p, len, nullptr, 0.0f);
  CHECK(rc == SAG_OK, "sag_policy_backward_rows_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto got = d_grad.get();
  for (int k = 0; k < GUARD; k++) CHECK(got[np_ + 8 + k] == FILL, "od %d H %d list %d: guard word %d behind d_grad was written", od, H, len, k);

  // the header's function, in double, over the fp32 activations, entry by entry of the list
  std::vector<double> ref(np_ + 8, 0.0), dO(NO), dz2(H), dz1(H);
  int valid = 0;
  for (int j = 0; j < len; j++) {
    if (list[j] < 0 || list[j] >= total) continue;
    const int g = list[j];
    valid++;
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
      for (int k = 0; k < NO; k++) { s += (double)W3[(size_t)i * NO + k] * dO[k]; ref[oW3 + (size_t)i * NO + k] += (double)a2[i] * dO[k]; }
      dz2[i] = a2[i] > 0.0f ? s : 0.0;
    }
    for (int k = 0; k < NO; k++) ref[ob3 + k] += dO[k];
    for (int i = 0; i < H; i++) {
      double s = 0.0;
      for (int k = 0; k < H; k++) { s += (double)W2[(size_t)i * H + k] * dz2[k]; ref[oW2 + (size_t)i * H + k] += (double)a1[i] * dz2[k]; }
      dz1[i] = a1[i] > 0.0f ? s : 0.0;
      ref[ob2 + i] += dz2[i];
    }
    for (int k = 0; k < H; k++) {
      ref[ob1 + k] += dz1[k];
      for (int i = 0; i < od; i++) ref[oW1 + (size_t)i * H + k] += (double)x[i] * dz1[k];
    }
  }
  CHECK(valid == (bad ? len - 7 : len), "the list of %d entries has %d valid ones", len, valid);
  const size_t bounds[9] = {oW1, ob1, oW2, ob2, oW3, ob3, ostd, np_, np_ + 8};
  for (int t = 0; t < 8; t++) {
    double top = 0.0, err = 0.0;
    for (size_t k = bounds[t]; k < bounds[t + 1]; k++) {
      const double r = ref[k] * (double)d.scale;
      top = fmax(top, fabs(r));
      err = fmax(err, fabs((double)got[k] - r));
      CHECK(isfinite(got[k]), "od %d H %d list %d: word %zu is not finite", od, H, len, k);
    }
    CHECK(err <= 1e-4 * top, "od %d H %d rows %d x %d list %d: tensor %d differs by %.3g of %.3g", od, H, n_rows, n_planes, len, t, err, top);
  }
  CHECK(fabs((double)got[np_ + 5] - valid * (double)d.scale) <= 1e-6, "statistic 5 = %g, %d valid entries of %d", (double)got[np_ + 5], valid, len);
  const auto obs2 = d_obs.get();
  const auto list2 = d_list.get();
  CHECK(memcmp(obs2.data(), obs.data(), obs.size() * 4) == 0 && memcmp(list2.data(), list.data(), list.size() * 4) == 0,
        "the observations or the list changed");
}

}  // namespace

int main() {
  static const int robots[2][3] = {{SAG_ROBOT_POINT, 60, 2}, {SAG_ROBOT_DOGGO, 104, 12}};
  for (const auto& rb : robots) {
    sag_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.abi_version = SAG_ABI_VERSION; cfg.robot = rb[0]; cfg.n_envs = 8; cfg.device = 0;
    cfg.max_hazards = SAG_MAX_HAZARDS; cfg.max_vases = SAG_MAX_VASES; cfg.max_pillars = SAG_MAX_PILLARS; cfg.max_buttons = SAG_MAX_BUTTONS;
    cfg.has_box = 1; cfg.seed = SEED;
    const int rc = sag_create(&cfg, &g_ctx);
    if (rc != SAG_OK) { printf("sag_create: %d %s (SAG_HOSTEMU=1 set?)\n", rc, sag_last_error(nullptr)); return 2; }
    if (rb[0] == SAG_ROBOT_POINT)
      for (int n : {1, 33, 4097}) {
        permutation_case(n, 0u);
        permutation_case(n, 0xffffffffu);
      }
    const int H = rb[0] == SAG_ROBOT_POINT ? 32 : 96;
    rows_case(rb[1], rb[2], H, 33, 3, 1, false);     // one entry: the row that ends the allocation
    rows_case(rb[1], rb[2], H, 33, 3, 33, true);     // a tile plus one, the lone entry of the second tile out of range
    rows_case(rb[1], rb[2], H, 130, 3, 97, true);    // three tiles and a ragged last
    rows_case(rb[1], rb[2], 32, 33, 1, 97, false);   // more entries than rows: duplicates
    sag_destroy(g_ctx);
  }
  if (g_failures) { printf("shuffle_main: %d failures\n", g_failures); return 1; }
  printf("shuffle_main: ok\n");
  return 0;
}
