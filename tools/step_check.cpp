// step_check.cpp -- the host side of dynamic loss scaling (pico_amd/csrc/segments.cpp:
// bine_step_state_init, bine_step_update_host, step_update_args, adamw_dyn_args;
// pico_amd/csrc/bine_internal.h: step_update_rule, the statement k_step_update
// runs too) as a stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/step_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/step_check
//   tools/bin/step_check
//
// It drives bine_step_state_init at many step counts against the products of
// as many updates, long random sequences of bine_step_update_host (finite,
// zero, infinite and NaN norms; random hyper-parameters) against the rule's
// invariants restated here and against bine_adamw_consts, states placed at the
// very end of heap blocks of exactly BINE_STEP_STATE_BYTES (so a byte written
// past the block is the address sanitizer's to report), and every refusal.
// CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 20253;
static uint32_t rnd() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}
static double uni() { return (rnd() + 0.5) / 2147483648.0; }  // (0, 1)

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

using bine::StepState;

static bine_step_hyper defaults() {
  return {1e-3, 0.9, 0.999, 1e-8, 0.01, HUGE_VAL, 1e-6, 2.0, 0.5, 1.0, 16777216.0, 2000};
}

static int ulps(float a, float b) {
  int32_t x, y;
  memcpy(&x, &a, 4), memcpy(&y, &b, 4);
  return abs(x - y);
}

// a heap block of exactly one state
struct Block {
  StepState *s = static_cast<StepState *>(malloc(BINE_STEP_STATE_BYTES));
  ~Block() { free(s); }
};

int main() {
  const double nan = std::nan(""), inf = HUGE_VAL;
  uint64_t updates = 0, skips = 0;

  // bine_step_state_init(step = t) = the products of t updates
  const double betas[3][2] = {{0.9, 0.999}, {0.0, 0.5}, {0.75, 0.999999}};
  for (const auto &b : betas) {
    Block run;
    REQUIRE(bine_step_state_init(run.s, 3.0, 0, b[0], b[1]) == BINE_SUCCESS);
    REQUIRE(run.s->d[0] == 3.0 && run.s->d[2] == 0.0 && run.s->d[3] == 1.0 && run.s->d[4] == 1.0);
    bine_step_hyper h = defaults();
    h.beta1 = b[0], h.beta2 = b[1], h.growth_interval = INT64_MAX;
    for (int64_t t = 0; t <= 5000; t++) {
      if (t < 20 || t % 499 == 0) {
        Block at;
        REQUIRE(bine_step_state_init(at.s, 3.0, t, b[0], b[1]) == BINE_SUCCESS);
        REQUIRE(at.s->d[2] == (double)t && at.s->d[3] == run.s->d[3] && at.s->d[4] == run.s->d[4]);
        for (int j : {1, 5, 6, 7}) REQUIRE(at.s->d[j] == 0.0);
        for (float c : at.s->c) REQUIRE(c == 0.0f);
      }
      REQUIRE(bine_step_update_host(run.s, 1.0, &h) == BINE_SUCCESS);
      updates++;
    }
  }
  {  // far past the underflow: the early exit
    Block at;
    REQUIRE(bine_step_state_init(at.s, 1.0, INT64_MAX, 0.75, 0.25) == BINE_SUCCESS);
    REQUIRE(at.s->d[3] > 0.0 && at.s->d[3] < 1e-320 && at.s->d[4] == 0.0 && at.s->d[2] == (double)INT64_MAX);
  }

  // long random sequences with overflows, the rule's invariants after every update
  for (int seq = 0; seq < 64; seq++) {
    bine_step_hyper h = defaults();
    h.lr = std::pow(10.0, -1 - 4 * uni()), h.beta1 = seq % 8 == 0 ? 0.0 : 1.0 - std::pow(10.0, -3 * uni());
    h.beta2 = 1.0 - std::pow(10.0, -4 * uni()), h.eps = seq % 5 == 0 ? 0.0 : 1e-8, h.weight_decay = 0.1 * uni();
    h.max_norm = seq % 3 == 0 ? inf : std::pow(10.0, 2 * uni() - 1), h.clip_eps = seq % 4 == 0 ? 0.0 : 1e-6;
    h.growth_factor = 1.0 + 2 * uni(), h.backoff_factor = seq % 7 == 0 ? 1.0 : uni();
    h.growth_interval = 1 + rnd() % 40, h.min_scale = std::pow(2.0, -(int)(rnd() % 10));
    h.max_scale = h.min_scale * std::pow(2.0, rnd() % 30);
    const double scale0 = h.min_scale * (1.0 + (h.max_scale / h.min_scale - 1.0) * uni());
    const int64_t step0 = seq % 2 ? rnd() % 3000 : 0;
    Block b;
    REQUIRE(bine_step_state_init(b.s, scale0, step0, h.beta1, h.beta2) == BINE_SUCCESS);
    for (int i = 0; i < 4000; i++) {
      const StepState a = *b.s;
      const uint32_t kind = rnd() % 16;
      const double n2 = kind == 0 ? inf : kind == 1 ? nan : kind == 2 ? 0.0 : std::pow(10.0, 24 * uni() - 6);
      REQUIRE(bine_step_update_host(b.s, n2, &h) == BINE_SUCCESS);
      updates++;
      const StepState &s = *b.s;
      REQUIRE(s.d[0] >= h.min_scale && s.d[0] <= std::fmax(h.max_scale, scale0) && s.d[1] >= 0.0);
      REQUIRE(s.d[1] < (double)h.growth_interval && s.d[1] == std::floor(s.d[1]));
      REQUIRE(s.d[2] + s.d[7] == (double)(step0 + i + 1));
      if (kind < 2) {
        skips++;
        REQUIRE(s.d[5] == 1.0 && s.d[6] == 0.0 && s.d[1] == 0.0 && s.d[7] == a.d[7] + 1.0);
        REQUIRE(s.d[2] == a.d[2] && s.d[3] == a.d[3] && s.d[4] == a.d[4] && !memcmp(s.c, a.c, sizeof s.c));
        REQUIRE(s.d[0] == std::fmax(a.d[0] * h.backoff_factor, h.min_scale));
      } else {
        REQUIRE(s.d[5] == 0.0 && s.d[2] == a.d[2] + 1.0 && s.d[7] == a.d[7]);
        REQUIRE(s.d[3] == a.d[3] * h.beta1 && s.d[4] == a.d[4] * h.beta2);
        REQUIRE(s.d[6] > 0.0 && s.d[6] <= 1.0 / a.d[0]);
        const bool grow = a.d[1] + 1.0 >= (double)h.growth_interval;
        REQUIRE(s.d[0] == (grow ? std::fmin(a.d[0] * h.growth_factor, h.max_scale) : a.d[0]));
        REQUIRE(s.d[1] == (grow ? 0.0 : a.d[1] + 1.0));
        float k[8];
        REQUIRE(bine_adamw_consts(h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, (int64_t)s.d[2], k) == BINE_SUCCESS);
        for (int j : {0, 1, 2, 3, 4, 6}) REQUIRE(s.c[j] == k[j]);
        // 1 - pw amplifies the products' t * 2^-53 by up to 1 / (1 - beta) <= 10^4 here: still far below an ulp
        REQUIRE(ulps(s.c[5], k[5]) <= 1 && ulps(s.c[7], k[7]) <= 1);
      }
    }
  }

  // refusals: bine_step_state_init
  Block b;
  alignas(8) unsigned char raw[BINE_STEP_STATE_BYTES + 8];
  REQUIRE(bine_step_state_init(nullptr, 1.0, 0, 0.9, 0.999) == BINE_ERR_ARG);
  REQUIRE(bine_step_state_init(raw + 4, 1.0, 0, 0.9, 0.999) == BINE_ERR_ARG);
  REQUIRE(bine_step_state_init(raw + 8, 1.0, 0, 0.9, 0.999) == BINE_SUCCESS);
  for (double bad : {0.0, -1.0, inf, nan}) REQUIRE(bine_step_state_init(b.s, bad, 0, 0.9, 0.999) == BINE_ERR_ARG);
  REQUIRE(bine_step_state_init(b.s, 1.0, -1, 0.9, 0.999) == BINE_ERR_ARG);
  for (double bad : {-0.1, 1.0, inf, nan}) {
    REQUIRE(bine_step_state_init(b.s, 1.0, 0, bad, 0.999) == BINE_ERR_ARG);
    REQUIRE(bine_step_state_init(b.s, 1.0, 0, 0.9, bad) == BINE_ERR_ARG);
  }
  // bine_step_update_host / step_update_args: every field in turn
  REQUIRE(bine_step_state_init(b.s, 1.0, 0, 0.9, 0.999) == BINE_SUCCESS);
  const StepState before = *b.s;
  auto bad_hyper = [&](auto set) {
    bine_step_hyper h = defaults();
    set(h);
    REQUIRE(bine_step_update_host(b.s, 1.0, &h) == BINE_ERR_ARG);
    REQUIRE(bine::step_update_args((void *)0x1000, (void *)0x2000, &h) == BINE_ERR_ARG);
    REQUIRE(!memcmp(b.s, &before, sizeof before));
  };
  for (double x : {-1.0, nan}) {
    bad_hyper([&](bine_step_hyper &h) { h.lr = x; });
    bad_hyper([&](bine_step_hyper &h) { h.eps = x; });
    bad_hyper([&](bine_step_hyper &h) { h.weight_decay = x; });
    bad_hyper([&](bine_step_hyper &h) { h.max_norm = x; });
    bad_hyper([&](bine_step_hyper &h) { h.clip_eps = x; });
    bad_hyper([&](bine_step_hyper &h) { h.min_scale = x; });
    bad_hyper([&](bine_step_hyper &h) { h.max_scale = x; });
    bad_hyper([&](bine_step_hyper &h) { h.growth_factor = x; });
    bad_hyper([&](bine_step_hyper &h) { h.backoff_factor = x; });
  }
  for (double x : {-0.1, 1.0, inf, nan}) {
    bad_hyper([&](bine_step_hyper &h) { h.beta1 = x; });
    bad_hyper([&](bine_step_hyper &h) { h.beta2 = x; });
  }
  bad_hyper([&](bine_step_hyper &h) { h.growth_factor = 0.999; });
  bad_hyper([&](bine_step_hyper &h) { h.growth_factor = inf; });
  bad_hyper([&](bine_step_hyper &h) { h.backoff_factor = 0.0; });
  bad_hyper([&](bine_step_hyper &h) { h.backoff_factor = 1.0001; });
  bad_hyper([&](bine_step_hyper &h) { h.growth_interval = 0; });
  bad_hyper([&](bine_step_hyper &h) { h.growth_interval = INT64_MIN; });
  bad_hyper([&](bine_step_hyper &h) { h.min_scale = 0.0; });
  bad_hyper([&](bine_step_hyper &h) { h.min_scale = 2.0, h.max_scale = 1.0; });
  bad_hyper([&](bine_step_hyper &h) { h.max_scale = inf; });
  bine_step_hyper h = defaults();
  REQUIRE(bine_step_update_host(nullptr, 1.0, &h) == BINE_ERR_ARG);
  REQUIRE(bine_step_update_host(raw + 4, 1.0, &h) == BINE_ERR_ARG);
  REQUIRE(bine_step_update_host(b.s, 1.0, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args(nullptr, (void *)0x2000, &h) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args((void *)0x1004, (void *)0x2000, &h) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args((void *)0x1000, nullptr, &h) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args((void *)0x1000, (void *)0x2004, &h) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args((void *)0x1000, (void *)0x2000, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::step_update_args((void *)0x1000, (void *)0x2000, &h) == BINE_SUCCESS);
  h.lr = h.beta1 = h.beta2 = h.eps = h.weight_decay = h.max_norm = h.clip_eps = 0.0;
  h.growth_factor = h.backoff_factor = 1.0, h.growth_interval = 1, h.min_scale = h.max_scale = 3.0;
  // every bound at its edge; 0 / 0 gives cc = 1; min_scale acts on a back-off only, so the scale of 1 stays
  REQUIRE(bine_step_update_host(b.s, 0.0, &h) == BINE_SUCCESS && b.s->d[0] == 1.0 && b.s->d[6] == 1.0);

  // adamw_dyn_args (what bine_adamw_segments_dyn and bine_adamw_multi_dyn check before any HIP call)
  void *pp[2] = {(void *)0x1000, (void *)0x2000};
  const void *const *gp = pp;
  const size_t c2[2] = {5, 0};
  std::vector<bine::AdamwLaunch> ls;
  auto dyn = [&](int n, void *const *p, const void *state, int gd = BINE_FLOAT) {
    return bine::adamw_dyn_args(n, p, pp, pp, gp, pp, c2, gd, BINE_FLOAT, state, &ls);
  };
  REQUIRE(dyn(2, pp, (void *)0x3008) == BINE_SUCCESS && ls.size() == 1 && ls[0].nseg == 1);
  REQUIRE(dyn(2, pp, nullptr) == BINE_ERR_ARG);
  REQUIRE(dyn(2, pp, (void *)0x3004) == BINE_ERR_ARG);
  REQUIRE(dyn(0, nullptr, nullptr) == BINE_ERR_ARG);
  REQUIRE(dyn(0, nullptr, (void *)0x3008) == BINE_SUCCESS);
  REQUIRE(dyn(-1, pp, (void *)0x3008) == BINE_ERR_ARG);
  REQUIRE(dyn(2, nullptr, (void *)0x3008) == BINE_ERR_ARG);
  REQUIRE(dyn(2, pp, (void *)0x3008, BINE_DOUBLE) == BINE_ERR_ARG);
  void *odd[2] = {(void *)0x1002, nullptr};
  REQUIRE(dyn(2, odd, (void *)0x3008) == BINE_ERR_ARG);
  printf("step_check: ok (%llu updates, %llu skipped)\n", (unsigned long long)updates, (unsigned long long)skips);
  return 0;
}
