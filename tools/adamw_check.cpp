// adamw_check.cpp -- the host side of the fused AdamW step (pico_amd/csrc/segments.cpp:
// bine_adamw_consts, plan_adamw_launches / bine_plan_adamw, adamw_args) as a
// stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/adamw_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/adamw_check
//   tools/bin/adamw_check
//
// It walks shard lists of tests/test_adamw.py's kind (the nine counts at every
// element phase of p, every operand in turn off p's phase, pout absent, list
// lengths around the per-launch 64 and the per-call 1,024, empties and NULL
// empties) through bine_plan_adamw and plan_adamw_launches, checks the launch
// tables against the tile rule, the launch cut and the body flag restated
// here, and the refusals of the three entry points.  CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 20252;
static uint32_t rnd() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(g_state >> 33);
}

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

static const int kTypes[] = {BINE_FLOAT, BINE_FLOAT16, BINE_BFLOAT16};
constexpr int S = BINE_ADAMW_SEGS_PER_LAUNCH;

struct Lists {
  std::vector<uint64_t> p, m, v, g, o;
  std::vector<size_t> cnt;
  bool has_o = true;
  const uint64_t *po() const { return has_o ? o.data() : nullptr; }
};

static uint64_t tiles_of(uint64_t addr, uint64_t count) {
  if (!count) return 0;
  uint64_t head = ((16 - addr % 16) % 16) / 4;
  if (head > count) head = count;
  const uint64_t t = ((count - head) / 4 + 2047) / 2048;
  return t ? t : 1;
}

static uint64_t body_of(const Lists &l, int k, size_t gsz, size_t osz) {
  const uint64_t h = ((16 - l.p[k] % 16) % 16) / 4;
  bool vec = (l.m[k] + 4 * h) % 16 == 0 && (l.v[k] + 4 * h) % 16 == 0 && (l.g[k] + gsz * h) % (4 * gsz) == 0;
  if (l.has_o) vec = vec && (l.o[k] + osz * h) % (4 * osz) == 0;
  return vec ? 0 : 1;
}

// the records and the launch tables of one list against the rule; returns its workgroups
static uint64_t check(const Lists &l, int gdtype, int odtype) {
  const int n = (int)l.cnt.size();
  const size_t gsz = bine::adamw_esz(gdtype), osz = bine::adamw_esz(odtype);
  const int64_t segs = bine_plan_adamw(n, l.p.data(), l.m.data(), l.v.data(), l.g.data(), l.po(), l.cnt.data(), gdtype,
                                       odtype, nullptr, 0);
  REQUIRE(segs >= 0);
  std::vector<uint64_t> rec(5 * (size_t)segs + 5, 0xDEAD);
  REQUIRE(bine_plan_adamw(n, l.p.data(), l.m.data(), l.v.data(), l.g.data(), l.po(), l.cnt.data(), gdtype, odtype,
                          rec.data(), segs) == segs);
  for (int j = 0; j < 5; j++) REQUIRE(rec[5 * (size_t)segs + j] == 0xDEAD);  // nothing past cap
  std::vector<bine::AdamwLaunch> ls;
  REQUIRE(bine::plan_adamw_launches(n, l.p.data(), l.m.data(), l.v.data(), l.g.data(), l.po(), l.cnt.data(), gdtype,
                                    odtype, ls) == BINE_SUCCESS);
  int next = 0;
  int64_t t = 0;
  uint64_t wgs = 0;
  for (size_t li = 0; li < ls.size(); li++) {
    const bine::AdamwLaunch &L = ls[li];
    REQUIRE(L.nseg >= 1 && L.nseg <= S && L.tile0[0] == 0);
    REQUIRE(li + 1 == ls.size() || L.nseg == S);  // only the last launch is short
    for (int s = 0; s < L.nseg; s++, t++, next++) {
      while (next < n && !l.cnt[next]) next++;
      REQUIRE(next < n && L.seg[s] == next && t < segs);
      const uint64_t want = tiles_of(l.p[next], l.cnt[next]), body = body_of(l, next, gsz, osz);
      REQUIRE(L.tile0[s + 1] - L.tile0[s] == want);
      REQUIRE(((L.elem >> s) & 1) == body);
      const uint64_t *e = &rec[5 * (size_t)t];
      REQUIRE(e[0] == li && e[1] == (uint64_t)next && e[2] == L.tile0[s] && e[3] == want && e[4] == body);
    }
    REQUIRE(L.nseg == S || (L.elem >> L.nseg) == 0);
    wgs += L.tile0[L.nseg];
  }
  while (next < n && !l.cnt[next]) next++;
  REQUIRE(next == n && t == segs);
  REQUIRE(ls.size() == (size_t)(segs + S - 1) / S);
  return wgs;
}

int main() {
  uint64_t wgs = 0;
  const size_t tile = 8192;
  const size_t counts[] = {0, 1, 3, 4, 5, tile - 1, tile, tile + 1, 3 * tile + 21};
  for (int gdtype : kTypes)
    for (int odtype : kTypes) {
      const size_t gsz = bine::adamw_esz(gdtype), osz = bine::adamw_esz(odtype);
      REQUIRE(gsz && osz);
      // every element phase of p; variant 0: all congruent, 1..4: m, v, g, pout one element off, 5: no pout
      for (uint64_t phase = 0; phase < 4; phase++)
        for (int variant = 0; variant < 6; variant++) {
          Lists l;
          l.cnt.assign(counts, counts + 9);
          l.has_o = variant != 5;
          for (int k = 0; k < 9; k++) {
            const uint64_t off = (phase + 1) % 4;
            l.p.push_back(0x10000000 + 0x100000ull * k + 4 * phase);
            l.m.push_back(0x20000000 + 0x100000ull * k + 4 * (variant == 1 ? off : phase));
            l.v.push_back(0x30000000 + 0x100000ull * k + 4 * (variant == 2 ? off : phase));
            l.g.push_back(0x40000000 + 0x100000ull * k + gsz * (variant == 3 ? off : phase));
            l.o.push_back(0x50000000 + 0x100000ull * k + osz * (variant == 4 ? off : phase));
          }
          for (int k = 1; k < 9; k++) REQUIRE(body_of(l, k, gsz, osz) == (variant >= 1 && variant <= 4 ? 1u : 0u));
          wgs += check(l, gdtype, odtype);
        }
      // list lengths around a launch's 64 segments and the call's 1,024
      for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
        Lists l;
        l.has_o = rnd() % 4 != 0;
        uint64_t a = 0x1000000;
        for (int k = 0; k < n; k++) {
          const size_t c = rnd() % 4 == 0 ? 0 : counts[rnd() % (n > S + 1 ? 7 : 9)];
          const bool null = c == 0 && rnd() % 2;  // an empty shard may be NULL
          const uint64_t ph = rnd() % 4;
          auto at = [&](uint64_t base, size_t esz, bool off) {
            return null ? 0 : base + a + esz * (off ? (ph + 1 + rnd() % 3) % 4 : ph);
          };
          l.cnt.push_back(c);
          l.p.push_back(at(0x100000000ull, 4, false));
          l.m.push_back(at(0x200000000ull, 4, rnd() % 8 == 0));
          l.v.push_back(at(0x300000000ull, 4, rnd() % 8 == 0));
          l.g.push_back(at(0x400000000ull, gsz, rnd() % 8 == 0));
          l.o.push_back(at(0x500000000ull, osz, rnd() % 8 == 0));
          a += (c * 4 + 64) & ~(uint64_t)15;
        }
        wgs += check(l, gdtype, odtype);
      }
    }

  // the refusals of bine_plan_adamw
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 4);
  auto plan = [&](int n, const uint64_t *p, const uint64_t *m, const uint64_t *v, const uint64_t *g, const uint64_t *o,
                  const size_t *cnt, int gd = BINE_FLOAT, int od = BINE_FLOAT) {
    return bine_plan_adamw(n, p, m, v, g, o, cnt, gd, od, nullptr, 0);
  };
  const uint64_t *A = a.data();
  REQUIRE(plan(BINE_MULTI_MAX + 1, A, A, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(BINE_MULTI_MAX, A, A, A, A, A, c.data()) == BINE_MULTI_MAX);
  REQUIRE(plan(-1, A, A, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, nullptr, A, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, nullptr, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, nullptr, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, A, nullptr, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, A, A, nullptr, c.data()) == 1);  // pout may be NULL as a whole
  REQUIRE(plan(1, A, A, A, A, A, nullptr) == -BINE_ERR_ARG);
  REQUIRE(plan(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((plan(1, A, A, A, A, A, c.data(), dtype, BINE_FLOAT) == 1) == ok);
    REQUIRE((plan(1, A, A, A, A, nullptr, c.data(), BINE_FLOAT, dtype) == 1) == ok);
    REQUIRE(ok || plan(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, dtype, BINE_FLOAT) == -BINE_ERR_ARG);
  }
  const uint64_t zero = 0, odd = 0x1002, ok4 = 0x1004;
  const size_t one = 1, none = 0, huge = (size_t)1 << 57;
  for (int which = 0; which < 5; which++) {  // each of the five arrays in turn
    auto with = [&](const uint64_t *bad, const size_t *cnt, int gd, int od) {
      const uint64_t *q[5] = {&ok4, &ok4, &ok4, &ok4, &ok4};
      q[which] = bad;
      return plan(1, q[0], q[1], q[2], q[3], q[4], cnt, gd, od);
    };
    REQUIRE(with(&zero, &one, BINE_FLOAT, BINE_FLOAT) == -BINE_ERR_ARG);  // NULL with a non-zero count
    REQUIRE(with(&zero, &none, BINE_FLOAT, BINE_FLOAT) == 0);             // empty: may be NULL
    REQUIRE(with(&odd, &one, BINE_FLOAT, BINE_FLOAT) == -BINE_ERR_ARG);   // 2 mod 4: not a float's alignment
    REQUIRE(with(&odd, &none, BINE_FLOAT, BINE_FLOAT) == 0);
    // ... but a 16-bit element's
    REQUIRE((with(&odd, &one, BINE_FLOAT16, BINE_BFLOAT16) == 1) == (which >= 3));
  }
  REQUIRE(plan(1, A, A, A, A, A, &huge) == -BINE_ERR_ARG);

  // bine_adamw_consts: the values at step 1 (pow is exact there) and the refusals
  float k[8];
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, 0.01, 1, k) == BINE_SUCCESS);
  REQUIRE(k[0] == (float)(1.0 - 1e-3 * 0.01) && k[1] == (float)0.9 && k[2] == (float)(1.0 - 0.9));
  REQUIRE(k[3] == (float)0.999 && k[4] == (float)(1.0 - 0.999) && k[6] == (float)1e-8);
  REQUIRE(k[5] == (float)(1.0 / std::sqrt(1.0 - 0.999)) && k[7] == (float)(1e-3 / (1.0 - 0.9)));
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, 0.01, 1000000, k) == BINE_SUCCESS);
  REQUIRE(k[5] == 1.0f && k[7] == (float)1e-3);  // both powers are far below 2^-53
  const double nan = std::nan(""), inf = HUGE_VAL;
  REQUIRE(bine_adamw_consts(-1e-3, 0.9, 0.999, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(nan, 0.9, 0.999, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 1.0, 0.999, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, -0.1, 0.999, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, nan, 0.999, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 1.0, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, inf, 1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, -1e-8, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, nan, 0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, -0.01, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, nan, 1, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, 0.01, 0, k) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(1e-3, 0.9, 0.999, 1e-8, 0.01, 1, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine_adamw_consts(0.0, 0.0, 0.0, 0.0, 0.0, 1, k) == BINE_SUCCESS);

  // adamw_args (what bine_adamw_segments and bine_adamw_multi check before any HIP call)
  void *pp[2] = {(void *)0x1000, (void *)0x2000};
  const void *const *gp = pp;
  const size_t c2[2] = {5, 0};
  std::vector<bine::AdamwLaunch> ls;
  auto args = [&](const double *gcoef, double grad_mul, double lr, int64_t step, void *const *pout) {
    return bine::adamw_args(2, pp, pp, pp, gp, pout, c2, BINE_FLOAT, BINE_FLOAT, lr, 0.9, 0.999, 1e-8, 0.01, step,
                            gcoef, grad_mul, k, &ls);
  };
  REQUIRE(args(nullptr, 1.0, 1e-3, 1, pp) == BINE_SUCCESS && ls.size() == 1 && ls[0].nseg == 1);
  REQUIRE(args(nullptr, 0.0, 1e-3, 1, nullptr) == BINE_SUCCESS);
  REQUIRE(args((const double *)0x3008, 1.0, 1e-3, 1, pp) == BINE_SUCCESS);
  REQUIRE(args((const double *)0x3004, 1.0, 1e-3, 1, pp) == BINE_ERR_ARG);
  REQUIRE(args(nullptr, nan, 1e-3, 1, pp) == BINE_ERR_ARG);
  REQUIRE(args(nullptr, inf, 1e-3, 1, pp) == BINE_ERR_ARG);
  REQUIRE(args(nullptr, -1.0, 1e-3, 1, pp) == BINE_ERR_ARG);
  REQUIRE(args(nullptr, 1.0, -1e-3, 1, pp) == BINE_ERR_ARG);
  REQUIRE(args(nullptr, 1.0, 1e-3, 0, pp) == BINE_ERR_ARG);
  REQUIRE(bine::adamw_args(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, BINE_FLOAT, BINE_FLOAT16, 1e-3,
                           0.9, 0.999, 1e-8, 0.01, 1, nullptr, 1.0, nullptr, nullptr) == BINE_SUCCESS);
  REQUIRE(bine::adamw_args(-1, pp, pp, pp, gp, pp, c2, BINE_FLOAT, BINE_FLOAT, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1,
                           nullptr, 1.0, nullptr, nullptr) == BINE_ERR_ARG);
  printf("adamw_check: ok (%llu workgroups)\n", (unsigned long long)wgs);
  return 0;
}
