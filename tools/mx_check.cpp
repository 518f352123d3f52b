// mx_check.cpp -- the host side of the MX block-scaled quantization
// (pico_amd/csrc/segments.cpp: plan_mx_launches / bine_plan_mx, mx_args,
// mx_multi_args, bine_mx_scale_host) as a stand-alone program, for the host
// sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/mx_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/mx_check
//   tools/bin/mx_check
//
// It walks tensor lists of tests/test_mx.py's kind (counts around 32 and around
// one tile at every element phase of the wide side and every byte phase of the
// data side, list lengths around the per-launch 112 and the per-call 1,024,
// empties and NULL empties) through bine_plan_mx and plan_mx_launches, checks
// the launch tables against the tile rule, the launch cut and the body flag
// restated here, the scale rule against frexp on every boundary pattern, and
// the refusals.  CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 950;
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
static const int kFmts[] = {BINE_MX_E4M3, BINE_MX_E5M2, BINE_MX_E2M1};
constexpr int S = BINE_MX_SEGS_PER_LAUNCH;

static uint64_t tiles_of(uint64_t count, uint64_t esz) { return (count * esz + 32767) / 32768; }
static uint64_t body_of(uint64_t wide, uint64_t d8, uint64_t esz, int fmt) {
  const uint64_t per = fmt == BINE_MX_E2M1 ? 8 / esz : 16 / esz;
  return wide % 16 || d8 % per ? 1 : 0;
}

static uint64_t check(const std::vector<uint64_t> &wide, const std::vector<uint64_t> &d8,
                      const std::vector<uint64_t> &sc, const std::vector<size_t> &cnt, int dtype, int fmt) {
  const int n = (int)cnt.size();
  const uint64_t esz = bine::adamw_esz(dtype);
  const int64_t segs = bine_plan_mx(n, wide.data(), d8.data(), sc.data(), cnt.data(), dtype, fmt, nullptr, 0);
  REQUIRE(segs >= 0);
  std::vector<uint64_t> rec(5 * (size_t)segs + 5, 0xDEAD);
  REQUIRE(bine_plan_mx(n, wide.data(), d8.data(), sc.data(), cnt.data(), dtype, fmt, rec.data(), segs) == segs);
  for (int j = 0; j < 5; j++) REQUIRE(rec[5 * (size_t)segs + j] == 0xDEAD);  // nothing past cap
  std::vector<bine::MxLaunch> ls;
  REQUIRE(bine::plan_mx_launches(n, wide.data(), d8.data(), sc.data(), cnt.data(), dtype, fmt, ls) == BINE_SUCCESS);
  int next = 0;
  int64_t t = 0;
  uint64_t wgs = 0;
  for (size_t li = 0; li < ls.size(); li++) {
    const bine::MxLaunch &L = ls[li];
    REQUIRE(L.nseg >= 1 && L.nseg <= S && L.tile0[0] == 0);
    REQUIRE(li + 1 == ls.size() || L.nseg == S);  // only the last launch is short
    for (int s = 0; s < L.nseg; s++, t++, next++) {
      while (next < n && !cnt[next]) next++;
      REQUIRE(next < n && L.seg[s] == next && t < segs);
      const uint64_t want = tiles_of(cnt[next], esz), body = body_of(wide[next], d8[next], esz, fmt);
      REQUIRE(want >= 1 && L.tile0[s + 1] - L.tile0[s] == want);
      REQUIRE(((L.elem[s >> 6] >> (s & 63)) & 1) == body);
      const uint64_t *e = &rec[5 * (size_t)t];
      REQUIRE(e[0] == li && e[1] == (uint64_t)next && e[2] == L.tile0[s] && e[3] == want && e[4] == body);
    }
    for (int s = L.nseg; s < S; s++) REQUIRE(((L.elem[s >> 6] >> (s & 63)) & 1) == 0);
    wgs += L.tile0[L.nseg];
  }
  while (next < n && !cnt[next]) next++;
  REQUIRE(next == n && t == segs);
  REQUIRE(ls.size() == (size_t)(segs + S - 1) / S);
  // the body flags set again for other addresses of the same counts
  std::vector<const void *> w2, d2;
  for (int k = 0; k < n; k++) {
    w2.push_back((const void *)(uintptr_t)(wide[k] ? wide[k] + 16 : 0));
    d2.push_back((const void *)(uintptr_t)(d8[k] ? d8[k] + 1 : 0));
  }
  bine::mx_set_bodies(ls, w2.data(), d2.data(), dtype, fmt);
  for (const bine::MxLaunch &L : ls)
    for (int s = 0; s < L.nseg; s++)
      REQUIRE(((L.elem[s >> 6] >> (s & 63)) & 1) == body_of(wide[L.seg[s]] + 16, d8[L.seg[s]] + 1, esz, fmt));
  return wgs;
}

// the rule with frexp, as bine_amd.h states it
static uint8_t rule(uint32_t A, int fmt) {
  if (A >= 0x7f800000u) return 0xff;
  if (A == 0) return 0;
  float a;
  memcpy(&a, &A, 4);
  int x;
  (void)frexp((double)a, &x);  // a = f * 2^x, f in [0.5, 1): floor(log2 a) = x - 1
  const int emax = fmt == BINE_MX_E4M3 ? 8 : fmt == BINE_MX_E5M2 ? 15 : 2;
  const int s = x - 1 - emax + 127;
  return (uint8_t)(s < 0 ? 0 : s);
}

int main() {
  uint64_t wgs = 0;
  for (int dtype : kTypes)
    for (int fmt : kFmts) {
      const uint64_t esz = bine::adamw_esz(dtype), V = 16 / esz, tile = 32768 / esz;
      REQUIRE(esz);
      const size_t counts[] = {0, 1, 31, 32, 33, (size_t)tile - 1, (size_t)tile, (size_t)tile + 1, 3 * (size_t)tile + 21};
      for (uint64_t sp = 0; sp < V; sp++)
        for (uint64_t dp = 0; dp < 2 * V; dp++) {
          std::vector<uint64_t> w, d, s;
          std::vector<size_t> c(counts, counts + 9);
          for (int k = 0; k < 9; k++) {
            w.push_back(0x10000000 + 0x100000ull * k + esz * sp);
            d.push_back(0x50000000 + 0x100000ull * k + dp);
            s.push_back(0x70000000 + 0x100000ull * k + (dp * 7 + sp) % 5);
          }
          wgs += check(w, d, s, c, dtype, fmt);
        }
      for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
        std::vector<uint64_t> w, d, s;
        std::vector<size_t> c;
        uint64_t a = 0x1000000;
        for (int k = 0; k < n; k++) {
          const size_t cnt = rnd() % 4 == 0 ? 0 : counts[rnd() % (n > S + 1 ? 7 : 9)];
          const bool null = cnt == 0 && rnd() % 2;  // an empty tensor may be NULL
          c.push_back(cnt);
          w.push_back(null ? 0 : 0x100000000ull + a + esz * (rnd() % 2) * (rnd() % V));
          d.push_back(null ? 0 : 0x500000000ull + a + (rnd() % 2) * (rnd() % 16));
          s.push_back(null ? 0 : 0x700000000ull + a + rnd() % 16);
          a += (cnt * 4 + 64) & ~(uint64_t)15;
        }
        wgs += check(w, d, s, c, dtype, fmt);
      }
    }

  // the refusals of bine_plan_mx
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 4);
  auto plan = [&](int n, const uint64_t *w, const uint64_t *d, const uint64_t *s, const size_t *cnt,
                  int dt = BINE_FLOAT, int fmt = BINE_MX_E4M3) { return bine_plan_mx(n, w, d, s, cnt, dt, fmt, nullptr, 0); };
  const uint64_t *A = a.data();
  REQUIRE(plan(BINE_MULTI_MAX + 1, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(BINE_MULTI_MAX, A, A, A, c.data()) == BINE_MULTI_MAX);
  REQUIRE(plan(-1, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, nullptr, A, A, c.data()) == -BINE_ERR_ARG && plan(1, A, nullptr, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, nullptr, c.data()) == -BINE_ERR_ARG && plan(1, A, A, A, nullptr) == -BINE_ERR_ARG);
  REQUIRE(plan(0, nullptr, nullptr, nullptr, nullptr) == 0);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((plan(1, A, A, A, c.data(), dtype) == 1) == ok);
  }
  for (int fmt = -2; fmt < 6; fmt++) REQUIRE((plan(1, A, A, A, c.data(), BINE_FLOAT, fmt) == 1) == (fmt >= 0 && fmt <= 2));
  const uint64_t zero = 0, odd = 0x1002, ok4 = 0x1004;
  const size_t one = 1, none = 0, huge = (size_t)1 << 57;
  REQUIRE(plan(1, &zero, &ok4, &ok4, &one) == -BINE_ERR_ARG && plan(1, &ok4, &zero, &ok4, &one) == -BINE_ERR_ARG);
  REQUIRE(plan(1, &ok4, &ok4, &zero, &one) == -BINE_ERR_ARG && plan(1, &zero, &zero, &zero, &none) == 0);
  REQUIRE(plan(1, &odd, &ok4, &ok4, &one) == -BINE_ERR_ARG && plan(1, &odd, &ok4, &ok4, &one, BINE_FLOAT16) == 1);
  REQUIRE(plan(1, &ok4, &odd, &odd, &one) == 1 && plan(1, &ok4, &ok4, &ok4, &huge) == -BINE_ERR_ARG);

  // the scale rule: bine_mx_scale_host against frexp
  uint64_t pats = 0;
  for (int fmt : kFmts) {
    auto same = [&](uint32_t A32) {
      uint8_t s = 0x55;
      REQUIRE(bine_mx_scale_host(A32, fmt, &s) == BINE_SUCCESS);
      REQUIRE(s == rule(A32, fmt) && (s <= 252 || s == 0xff));
      pats++;
    };
    for (uint32_t ex = 0; ex < 256; ex++)
      for (uint32_t m : {0u, 1u, 0x400000u, 0x7fffffu}) same(ex << 23 | m);
    for (int p = 0; p < 23; p++)
      for (uint32_t m : {1u << p, (1u << p) | 1u, (2u << p) - 1}) same(m);
    for (int j = 0; j < 200000; j++) same((rnd() << 1 ^ rnd()) & 0x7fffffffu);
    uint8_t s;
    REQUIRE(bine_mx_scale_host(1, 3, &s) == BINE_ERR_ARG && bine_mx_scale_host(1, -1, &s) == BINE_ERR_ARG);
    REQUIRE(bine_mx_scale_host(1, fmt, nullptr) == BINE_ERR_ARG);
  }

  // mx_args and mx_multi_args (what the entry points check before any HIP call)
  void *pp[2] = {(void *)0x1000, (void *)0x2003};
  const void *const *cp = pp;
  const size_t c2[2] = {5, 0}, c32[2] = {64, 0}, c33[2] = {33, 0}, cbig[2] = {(size_t)1 << 31, 0};
  const char *why = nullptr;
  std::vector<bine::MxLaunch> ml;
  REQUIRE(bine::mx_args(2, cp, cp, cp, c2, BINE_FLOAT, 0, &why, &ml) == BINE_SUCCESS && ml.size() == 1);
  REQUIRE(ml[0].nseg == 1 && ml[0].elem[0] == 0 && ml[0].tile0[1] == 1);
  REQUIRE(bine::mx_args(2, cp, cp, cp, c2, BINE_FLOAT, 3, &why, nullptr) == BINE_ERR_ARG && why);
  REQUIRE(bine::mx_args(2, cp, cp, cp, c2, BINE_INT32, 0, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::mx_args(1, cp + 1, cp, cp, c2, BINE_FLOAT, 0, nullptr, nullptr) == BINE_ERR_ARG);  // 0x2003
  REQUIRE(bine::mx_args(1, cp, cp + 1, cp, c2, BINE_FLOAT, 0, &why, &ml) == BINE_SUCCESS && ml[0].elem[0] == 1);
  REQUIRE(bine::mx_args(1, cp, cp, nullptr, c2, BINE_FLOAT, 0, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::mx_args(0, nullptr, nullptr, nullptr, nullptr, BINE_BFLOAT16, 2, &why, &ml) == BINE_SUCCESS && ml.empty());
  REQUIRE(bine::mx_multi_args(2, pp, pp, cp, c32, BINE_FLOAT, 2, &why, &ml) == BINE_SUCCESS && ml.size() == 1);
  REQUIRE(bine::mx_multi_args(2, pp, pp, cp, c33, BINE_FLOAT, 2, &why, nullptr) == BINE_ERR_ARG && strstr(why, "32"));
  REQUIRE(bine::mx_multi_args(2, pp, pp, cp, cbig, BINE_FLOAT, 0, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::mx_multi_args(BINE_MULTI_MAX / 2 + 1, pp, pp, cp, c32, BINE_FLOAT, 0, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::mx_multi_args(2, pp, pp, cp, c33, BINE_DOUBLE, 0, &why, nullptr) == BINE_ERR_ARG && strstr(why, "sdtype"));
  printf("mx_check: ok (%llu workgroups, %llu scale patterns)\n", (unsigned long long)wgs, (unsigned long long)pats);
  return 0;
}
