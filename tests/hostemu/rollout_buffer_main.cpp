// rollout_buffer_main.cpp - TEST INFRASTRUCTURE: sag_append_rows_device and sag_gae_device of the host build of the device
// sources (tests/hostemu/build.py) driven from a program of its own, so that the whole process - this file and the library -
// runs under AddressSanitizer and UndefinedBehaviorSanitizer (test_rollout_buffer_hostemu.py compiles and runs it).  "Device"
// memory is malloc'ed there, every array below is allocated at its exact size, and the results are compared with the plain
// loops of this file.  Needs SAG_HOSTEMU=1 in the environment.  Exit status 0 and "rollout_buffer_main: ok" on success.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sag.h"

namespace {

constexpr int N = 130, PITCH = 256;   // two full wavefronts and a partial one of two lanes
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
float unit() { return (float)(rnd() & 0xffffff) / 16777216.0f; }

// a device array of exactly v.size() elements
template <class T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;
  explicit Dev(const std::vector<T>& v) : n(v.size()) {
    void* q = nullptr;
    if (sag_dev_alloc(g_ctx, n * sizeof(T), &q) != SAG_OK) { printf("sag_dev_alloc failed\n"); exit(1); }
    p = (T*)q;
    put(v);
  }
  ~Dev() { sag_dev_free(g_ctx, p); }
  void put(const std::vector<T>& v) { if (n) sag_dev_upload(g_ctx, p, v.data(), n * sizeof(T)); }
  std::vector<T> get() const {
    std::vector<T> v(n);
    if (n) sag_dev_download(g_ctx, v.data(), p, n * sizeof(T));
    return v;
  }
};

void append_case(int row_bytes, int capacity, int c0, int mask_kind) {
  std::vector<uint8_t> src((size_t)N * row_bytes), fill((size_t)capacity * row_bytes), mask(N);
  for (auto& b : src) b = (uint8_t)rnd();
  for (size_t k = 0; k < fill.size(); k++) fill[k] = (uint8_t)(k % 251 + 3);
  for (int i = 0; i < N; i++)
    mask[i] = mask_kind == 0 ? 0 : mask_kind == 1 ? 1 : mask_kind == 2 ? (rnd() % 3 == 0 ? (uint8_t)(1 + rnd() % 255) : 0) : mask_kind == 3 ? i == 0 : i == N - 1;
  Dev<uint8_t> d_src(src), d_store(fill), d_mask(mask);
  Dev<int32_t> d_count(std::vector<int32_t>{c0}), d_slot(std::vector<int32_t>(N, -7));
  int rc = sag_append_rows_device(g_ctx, d_mask.p, row_bytes, d_src.p, d_store.p, capacity, d_count.p, 0, d_slot.p);
  CHECK(rc == SAG_OK, "sag_append_rows_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  const auto store = d_store.get();
  const auto slot = d_slot.get();
  const int count = d_count.get()[0];
  int k = 0;
  for (int i = 0; i < N; i++) k += mask[i] != 0;
  const int fit = k < capacity - c0 ? k : (capacity - c0 > 0 ? capacity - c0 : 0);
  CHECK(count == c0 + k, "rows %d capacity %d c0 %d mask %d: count %d, expected %d", row_bytes, capacity, c0, mask_kind, count, c0 + k);
  std::vector<int> owner(capacity, -1);
  int kept = 0;
  for (int g0 = 0; g0 < N; g0 += 64) {
    int prev = -2;   // the slot of the previous set env of this group: -2 none yet, -1 did not fit
    for (int i = g0; i < g0 + 64 && i < N; i++) {
      if (!mask[i]) { CHECK(slot[i] == -1, "env %d outside the mask has slot %d", i, slot[i]); continue; }
      const int s = slot[i];
      CHECK(s == -1 || (s >= c0 && s < c0 + k && s < capacity), "env %d: slot %d", i, s);
      if (prev == -1) CHECK(s == -1, "env %d fits after an env of its group that did not", i);
      if (prev >= 0 && s >= 0) CHECK(s == prev + 1, "env %d: slot %d after %d", i, s, prev);
      prev = s;
      if (s >= 0 && s < capacity) {
        CHECK(owner[s] == -1, "slot %d handed out twice", s);
        owner[s] = i;
        kept++;
        CHECK(memcmp(&store[(size_t)s * row_bytes], &src[(size_t)i * row_bytes], row_bytes) == 0, "env %d: row of slot %d differs", i, s);
      }
    }
  }
  CHECK(kept == fit, "rows %d capacity %d c0 %d mask %d: %d rows kept, %d fit", row_bytes, capacity, c0, mask_kind, kept, fit);
  for (int s = 0; s < capacity; s++)
    if (owner[s] < 0)
      CHECK(memcmp(&store[(size_t)s * row_bytes], &fill[(size_t)s * row_bytes], row_bytes) == 0, "unclaimed row %d of the store was written", s);
  CHECK(d_src.get() == src, "the source changed");
}

// one channel of the header's recipe, every operation rounded on its own (this file is built with -ffp-contract=off)
void gae_loop(int T, float gamma, float lam, const float* r, int r_stride, const uint8_t* cost, const uint8_t* ended, const float* value,
              const int32_t* slot, const float* fin, int capacity, std::vector<float>& adv, std::vector<float>& ret) {
  const float gl = gamma * lam;
  for (int i = 0; i < N; i++) {
    float carry = 0.0f;
    for (int t = T - 1; t >= 0; t--) {
      const size_t at = (size_t)t * PITCH + i;
      const int e = ended[at];
      float nv;
      if (e == 0) nv = value[at + PITCH];
      else if (e == 2 && slot && fin && slot[at] >= 0 && slot[at] < capacity) { nv = fin[slot[at]]; carry = 0.0f; }
      else { nv = 0.0f; carry = 0.0f; }
      const float rr = r ? r[at * r_stride] : (cost[at] != 0 ? 1.0f : 0.0f);
      volatile float q = gamma * nv;
      volatile float s = rr + q;
      volatile float delta = s - value[at];
      volatile float p = gl * carry;
      volatile float A = delta + p;
      volatile float rt = A + value[at];
      adv[at] = A;
      ret[at] = rt;
      carry = A;
    }
  }
}

void gae_case(int T, bool with_cost, bool with_slot, float gamma, float lam, float cgamma, float clam) {
  const size_t TP = (size_t)T * PITCH;
  const int capacity = 40;
  std::vector<float> reward(TP * 2), value(TP + PITCH), cvalue(TP + PITCH), fv(capacity), fcv(capacity);
  std::vector<uint8_t> cost(TP), ended(TP);
  std::vector<int32_t> slot(TP, -1);
  const float nan = nanf("");
  for (int t = 0; t <= T; t++)
    for (int i = 0; i < PITCH; i++) {
      const size_t at = (size_t)t * PITCH + i;
      const bool pad = i >= N;
      value[at] = pad ? nan : 6.0f * unit() - 3.0f;
      cvalue[at] = pad ? nan : 4.0f * unit();
      if (t == T) continue;
      reward[2 * at] = pad ? nan : 2.0f * unit() - 1.0f;
      reward[2 * at + 1] = nan;
      cost[at] = pad ? 1 : (rnd() % 4 == 0 ? (uint8_t)(1 + rnd() % 255) : 0);
      ended[at] = pad ? 7 : (rnd() % 10 == 0 ? (uint8_t)(1 + rnd() % 2) : 0);
      if (!pad && ended[at] == 2) slot[at] = (int32_t)(rnd() % (capacity + 4)) - 2;   // -2 ... capacity + 1: some are not kept
    }
  if (T > 1) ended[(size_t)(T - 1) * PITCH + 3] = 2, slot[(size_t)(T - 1) * PITCH + 3] = 5;
  for (auto& x : fv) x = 6.0f * unit() - 3.0f;
  for (auto& x : fcv) x = 4.0f * unit();
  const uint32_t fill_bits = 0x7fc12345u;
  float fill;
  memcpy(&fill, &fill_bits, 4);
  std::vector<float> out0(TP, fill);
  Dev<float> d_reward(reward), d_value(value), d_cvalue(cvalue), d_fv(fv), d_fcv(fcv), d_adv(out0), d_ret(out0), d_cadv(out0), d_cret(out0);
  Dev<uint8_t> d_cost(cost), d_ended(ended);
  Dev<int32_t> d_slot(slot);
  sag_gae_desc d;
  memset(&d, 0, sizeof(d));
  d.T = T; d.pitch = PITCH; d.capacity = capacity;
  d.gamma = gamma; d.lam = lam; d.cost_gamma = cgamma; d.cost_lam = clam;
  d.d_reward = d_reward.p; d.d_cost = d_cost.p; d.d_ended = d_ended.p; d.d_value = d_value.p;
  d.d_adv = d_adv.p; d.d_ret = d_ret.p;
  if (with_cost) { d.d_cvalue = d_cvalue.p; d.d_cadv = d_cadv.p; d.d_cret = d_cret.p; }
  if (with_slot) { d.d_slot = d_slot.p; d.d_final_value = d_fv.p; d.d_final_cvalue = with_cost ? d_fcv.p : nullptr; }
  int rc = sag_gae_device(g_ctx, &d);
  CHECK(rc == SAG_OK, "sag_gae_device: %d %s", rc, sag_last_error(g_ctx));
  sag_wait(g_ctx);
  std::vector<float> adv(TP, fill), ret(TP, fill), cadv(TP, fill), cret(TP, fill);
  gae_loop(T, gamma, lam, reward.data(), 2, cost.data(), ended.data(), value.data(), with_slot ? slot.data() : nullptr, fv.data(), capacity, adv, ret);
  if (with_cost)
    gae_loop(T, cgamma, clam, nullptr, 0, cost.data(), ended.data(), cvalue.data(), with_slot ? slot.data() : nullptr, fcv.data(), capacity, cadv, cret);
  const std::vector<float> got[4] = {d_adv.get(), d_ret.get(), d_cadv.get(), d_cret.get()};
  const std::vector<float>* want[4] = {&adv, &ret, &cadv, &cret};
  static const char* name[4] = {"adv", "ret", "cadv", "cret"};
  for (int k = 0; k < 4; k++)
    CHECK(memcmp(got[k].data(), want[k]->data(), TP * sizeof(float)) == 0, "T %d cost %d slot %d gamma %g lam %g: %s differs (pad columns included)", T,
          (int)with_cost, (int)with_slot, (double)gamma, (double)lam, name[k]);
  CHECK(d_reward.get().size() == reward.size() && memcmp(d_reward.get().data(), reward.data(), reward.size() * 4) == 0, "the rewards changed");
  CHECK(d_ended.get() == ended && d_cost.get() == cost && d_slot.get() == slot, "an input changed");
}

}  // namespace

int main() {
  sag_config cfg;
  memset(&cfg, 0, sizeof(cfg));
  cfg.abi_version = SAG_ABI_VERSION; cfg.robot = SAG_ROBOT_POINT; cfg.n_envs = N; cfg.device = 0;
  cfg.max_hazards = SAG_MAX_HAZARDS; cfg.max_vases = SAG_MAX_VASES; cfg.max_pillars = SAG_MAX_PILLARS; cfg.max_buttons = SAG_MAX_BUTTONS;
  cfg.has_box = 1; cfg.seed = 12345;
  int rc = sag_create(&cfg, &g_ctx);
  if (rc != SAG_OK) { printf("sag_create: %d %s (SAG_HOSTEMU=1 set?)\n", rc, sag_last_error(nullptr)); return 2; }
  for (int row_bytes : {16, 240})
    for (int mask_kind = 0; mask_kind < 5; mask_kind++)
      for (int c0 : {0, 5}) {
        append_case(row_bytes, N + 8, c0, mask_kind);
        append_case(row_bytes, 50, c0, mask_kind);   // a store that overflows under the full mask
      }
  append_case(240, 1, 0, 1);
  append_case(240, 7, 9, 1);   // a counter already past the capacity
  static const float pairs[4][2] = {{0.99f, 0.95f}, {1.0f, 1.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}};
  for (int T : {1, 2, 7, 8, 9, 37})
    for (int k = 0; k < 4; k++)
      for (int cost = 0; cost < 2; cost++)
        for (int slot = 0; slot < 2; slot++) gae_case(T, cost != 0, slot != 0, pairs[k][0], pairs[k][1], pairs[(k + 1) % 4][0], pairs[(k + 1) % 4][1]);
  sag_destroy(g_ctx);
  if (g_failures) { printf("rollout_buffer_main: %d failures\n", g_failures); return 1; }
  printf("rollout_buffer_main: ok\n");
  return 0;
}
