// quant_check.cpp -- the host side of the FP8 quantization (pico_amd/csrc/segments.cpp:
// plan_quant_launches / bine_plan_quant, amax_args, fp8_scales_args, quant_args,
// bine_fp8_scale_host) as a stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/quant_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/quant_check
//   tools/bin/quant_check
//
// It walks tensor lists of tests/test_quant.py's kind (the nine counts at every
// element phase of the wide side and every byte phase of the FP8 side, list
// lengths around the per-launch 128 and the per-call 1,024, empties and NULL
// empties) through bine_plan_quant and plan_quant_launches, checks the launch
// tables against the tile rule, the launch cut and the body flag restated
// here, the scale rule against frexp / ldexp on every boundary pattern, and
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
constexpr int S = BINE_COPY_SEGS_PER_LAUNCH;

static uint64_t tiles_of(uint64_t addr, uint64_t count, uint64_t esz) {
  if (!count) return 0;
  uint64_t head = ((16 - addr % 16) % 16) / esz;
  if (head > count) head = count;
  const uint64_t t = ((count - head) * esz / 16 + 2047) / 2048;
  return t ? t : 1;
}
static uint64_t body_of(uint64_t wide, uint64_t b8, uint64_t esz) {
  const uint64_t h = ((16 - wide % 16) % 16) / esz;
  return (b8 + h) % (16 / esz) ? 1 : 0;
}

static uint64_t check(const std::vector<uint64_t> &wide, const std::vector<uint64_t> &b8,
                      const std::vector<size_t> &cnt, int dtype) {
  const int n = (int)cnt.size();
  const uint64_t esz = bine::adamw_esz(dtype);
  const int64_t segs = bine_plan_quant(n, wide.data(), b8.data(), cnt.data(), dtype, nullptr, 0);
  REQUIRE(segs >= 0);
  std::vector<uint64_t> rec(5 * (size_t)segs + 5, 0xDEAD);
  REQUIRE(bine_plan_quant(n, wide.data(), b8.data(), cnt.data(), dtype, rec.data(), segs) == segs);
  for (int j = 0; j < 5; j++) REQUIRE(rec[5 * (size_t)segs + j] == 0xDEAD);  // nothing past cap
  std::vector<bine::QuantLaunch> ls;
  REQUIRE(bine::plan_quant_launches(n, wide.data(), b8.data(), cnt.data(), dtype, ls) == BINE_SUCCESS);
  int next = 0;
  int64_t t = 0;
  uint64_t wgs = 0;
  for (size_t li = 0; li < ls.size(); li++) {
    const bine::QuantLaunch &L = ls[li];
    REQUIRE(L.nseg >= 1 && L.nseg <= S && L.tile0[0] == 0);
    REQUIRE(li + 1 == ls.size() || L.nseg == S);  // only the last launch is short
    for (int s = 0; s < L.nseg; s++, t++, next++) {
      while (next < n && !cnt[next]) next++;
      REQUIRE(next < n && L.seg[s] == next && t < segs);
      const uint64_t want = tiles_of(wide[next], cnt[next], esz), body = body_of(wide[next], b8[next], esz);
      REQUIRE(L.tile0[s + 1] - L.tile0[s] == want);
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
  return wgs;
}

// the rule with frexp / ldexp, as bine_amd.h states it
static void rule(uint32_t bits, int fmt, float *scale, float *inv) {
  int e = 0;
  if (bits != 0 && bits < 0x7f800000u) {
    float a;
    memcpy(&a, &bits, 4);
    int x;
    const double f = frexp((double)a, &x);
    e = (fmt == BINE_FP8_E4M3 ? 9 : 16) - x - (f > 0.875 ? 1 : 0);
    e = e < -126 ? -126 : e > 126 ? 126 : e;
  }
  *scale = (float)ldexp(1.0, e);
  *inv = (float)ldexp(1.0, -e);
}

int main() {
  uint64_t wgs = 0;
  for (int dtype : kTypes) {
    const uint64_t esz = bine::adamw_esz(dtype), V = 16 / esz, tile = 2048 * V;
    REQUIRE(esz);
    const size_t counts[] = {0, 1, (size_t)V - 1, (size_t)V, (size_t)V + 1, (size_t)tile - 1, (size_t)tile,
                             (size_t)tile + 1, 3 * (size_t)tile + 21};
    for (uint64_t sp = 0; sp < V; sp++)
      for (uint64_t dp = 0; dp < 2 * V; dp++) {
        std::vector<uint64_t> w, b;
        std::vector<size_t> c(counts, counts + 9);
        for (int k = 0; k < 9; k++) {
          w.push_back(0x10000000 + 0x100000ull * k + esz * sp);
          b.push_back(0x50000000 + 0x100000ull * k + dp);
        }
        REQUIRE(body_of(w[1], b[1], esz) == ((dp + (V - sp) % V) % V ? 1u : 0u));
        wgs += check(w, b, c, dtype);
      }
    for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
      std::vector<uint64_t> w, b;
      std::vector<size_t> c;
      uint64_t a = 0x1000000;
      for (int k = 0; k < n; k++) {
        const size_t cnt = rnd() % 4 == 0 ? 0 : counts[rnd() % (n > S + 1 ? 7 : 9)];
        const bool null = cnt == 0 && rnd() % 2;  // an empty tensor may be NULL
        c.push_back(cnt);
        w.push_back(null ? 0 : 0x100000000ull + a + esz * (rnd() % V));
        b.push_back(null ? 0 : 0x500000000ull + a + rnd() % 16);
        a += (cnt * 4 + 64) & ~(uint64_t)15;
      }
      wgs += check(w, b, c, dtype);
    }
  }

  // the refusals of bine_plan_quant
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 4);
  auto plan = [&](int n, const uint64_t *w, const uint64_t *b, const size_t *cnt, int dt = BINE_FLOAT) {
    return bine_plan_quant(n, w, b, cnt, dt, nullptr, 0);
  };
  const uint64_t *A = a.data();
  REQUIRE(plan(BINE_MULTI_MAX + 1, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(BINE_MULTI_MAX, A, A, c.data()) == BINE_MULTI_MAX);
  REQUIRE(plan(-1, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, nullptr, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, nullptr, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, nullptr) == -BINE_ERR_ARG);
  REQUIRE(plan(0, nullptr, nullptr, nullptr) == 0);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((plan(1, A, A, c.data(), dtype) == 1) == ok);
    REQUIRE(ok || plan(-1, nullptr, nullptr, nullptr, dtype) == -BINE_ERR_ARG);
  }
  const uint64_t zero = 0, odd = 0x1002, ok4 = 0x1004;
  const size_t one = 1, none = 0, huge = (size_t)1 << 57;
  REQUIRE(plan(1, &zero, &ok4, &one) == -BINE_ERR_ARG && plan(1, &ok4, &zero, &one) == -BINE_ERR_ARG);
  REQUIRE(plan(1, &zero, &zero, &none) == 0);
  REQUIRE(plan(1, &odd, &ok4, &one) == -BINE_ERR_ARG && plan(1, &odd, &ok4, &one, BINE_FLOAT16) == 1);
  REQUIRE(plan(1, &ok4, &odd, &one) == 1 && plan(1, &ok4, &ok4, &huge) == -BINE_ERR_ARG);

  // the scale rule: bine_fp8_scale_host against frexp / ldexp
  uint64_t pats = 0;
  for (int fmt : {BINE_FP8_E4M3, BINE_FP8_E5M2}) {
    auto same = [&](uint32_t bits) {
      float s, i, ws, wi;
      REQUIRE(bine_fp8_scale_host(bits, fmt, &s, &i) == BINE_SUCCESS);
      rule(bits, fmt, &ws, &wi);
      REQUIRE(memcmp(&s, &ws, 4) == 0 && memcmp(&i, &wi, 4) == 0 && s * i == 1.0f);
      pats++;
    };
    for (uint32_t ex = 0; ex < 256; ex++)
      for (uint32_t m : {0u, 1u, 0x5fffffu, 0x600000u, 0x600001u, 0x7fffffu}) same(ex << 23 | m);
    for (int p = 0; p < 23; p++)
      for (uint32_t m : {1u << p, (1u << p) - 1, (7u << p) >> 2, ((7u << p) >> 2) + 1}) same(m);
    for (int j = 0; j < 200000; j++) same(rnd() << 1 ^ rnd());
    float s, i;
    REQUIRE(bine_fp8_scale_host(1, 2, &s, &i) == BINE_ERR_ARG && bine_fp8_scale_host(1, -1, &s, &i) == BINE_ERR_ARG);
    REQUIRE(bine_fp8_scale_host(1, fmt, nullptr, &i) == BINE_ERR_ARG);
    REQUIRE(bine_fp8_scale_host(1, fmt, &s, nullptr) == BINE_ERR_ARG);
  }

  // amax_args, fp8_scales_args, quant_args (what the entry points check before any HIP call)
  void *pp[2] = {(void *)0x1000, (void *)0x2003};
  const void *const *cp = pp;
  const size_t c2[2] = {5, 0};
  const char *why = nullptr;
  std::vector<bine::AmaxLaunch> sl;
  std::vector<bine::QuantLaunch> ql;
  REQUIRE(bine::amax_args(2, cp, c2, BINE_FLOAT, (void *)0x7000, &why, &sl) == BINE_SUCCESS && sl.size() == 1);
  // k_amax_segs' workgroups: BINE_AMAX_TILES_PER_WG consecutive tiles each, at least one per non-empty tensor
  {
    void *bp[4] = {(void *)0x10000, (void *)0x2000000, nullptr, (void *)0x4000004};
    const void *const *bq = bp;
    const size_t G = BINE_AMAX_TILES_PER_WG, tile = 8192;
    const size_t bc[4] = {1, G * tile, 0, (2 * G + 1) * tile + 3};
    REQUIRE(bine::amax_args(4, bq, bc, BINE_FLOAT, (void *)0x7000, &why, &sl) == BINE_SUCCESS && sl.size() == 1);
    REQUIRE(sl[0].nseg == 3 && sl[0].seg[0] == 0 && sl[0].seg[1] == 1 && sl[0].seg[2] == 3);
    REQUIRE(sl[0].tile0[0] == 0 && sl[0].tile0[1] == 1 && sl[0].tile0[2] == 2 && sl[0].tile0[3] == 5);
    bine::LaunchTable<BINE_COPY_SEGS_PER_LAUNCH> t;
    t.nseg = 3;
    const uint32_t tiles[4] = {0, G - 1, 2 * G - 1, 3 * G};  // G - 1, G and G + 1 tiles
    for (int s = 0; s < 3; s++) t.seg[s] = s;
    for (int s = 0; s <= 3; s++) t.tile0[s] = tiles[s];
    const bine::AmaxLaunch g = bine::amax_launch_of(t);
    REQUIRE(g.nseg == 3 && g.tile0[0] == 0 && g.tile0[1] == 1 && g.tile0[2] == 2 && g.tile0[3] == 4);
  }
  REQUIRE(bine::amax_args(2, cp, c2, BINE_DOUBLE, (void *)0x7000, &why, nullptr) == BINE_ERR_ARG && why);
  REQUIRE(bine::amax_args(2, cp, c2, BINE_FLOAT, nullptr, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::amax_args(2, cp, c2, BINE_FLOAT, (void *)0x7002, nullptr, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::amax_args(0, nullptr, nullptr, BINE_BFLOAT16, (void *)0x7000, &why, &sl) == BINE_SUCCESS && sl.empty());
  REQUIRE(bine::fp8_scales_args(3, (void *)0x7000, BINE_FP8_E5M2, (void *)0x8000, &why) == BINE_SUCCESS);
  REQUIRE(bine::fp8_scales_args(3, (void *)0x7000, 2, (void *)0x8000, &why) == BINE_ERR_ARG);
  REQUIRE(bine::fp8_scales_args(3, nullptr, 0, (void *)0x8000, &why) == BINE_ERR_ARG);
  REQUIRE(bine::fp8_scales_args(3, (void *)0x7000, 0, (void *)0x8001, &why) == BINE_ERR_ARG);
  REQUIRE(bine::fp8_scales_args(BINE_MULTI_MAX + 1, (void *)0x7000, 0, (void *)0x8000, &why) == BINE_ERR_ARG);
  REQUIRE(bine::quant_args(2, cp, cp, c2, BINE_FLOAT, 0, nullptr, &why, &ql) == BINE_SUCCESS && ql.size() == 1);
  REQUIRE(ql[0].nseg == 1 && ql[0].elem[0] == 0);
  REQUIRE(bine::quant_args(2, cp, cp, c2, BINE_FLOAT, 0, (void *)0x9002, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::quant_args(2, cp, cp, c2, BINE_FLOAT, 2, nullptr, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::quant_args(2, cp, cp, c2, BINE_INT32, 0, nullptr, &why, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine::quant_args(1, cp + 1, cp, c2, BINE_FLOAT, 0, nullptr, nullptr, nullptr) == BINE_ERR_ARG);  // 0x2003
  REQUIRE(bine::quant_args(1, cp, cp + 1, c2, BINE_FLOAT, 0, nullptr, &why, &ql) == BINE_SUCCESS && ql[0].elem[0] == 1);
  printf("quant_check: ok (%llu workgroups, %llu scale patterns)\n", (unsigned long long)wgs,
         (unsigned long long)pats);
  return 0;
}
