// mxef_check.cpp -- the host side of MX quantization with an error-feedback
// residual (pico_amd/csrc/segments.cpp: plan_mx_ef_launches / bine_plan_mx_ef,
// mx_ef_args, mx_ef_rs_args) as a stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/mxef_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/mxef_check
//   tools/bin/mxef_check
//
// It walks buckets of tests/test_mxef.py's kind (counts around one tile of the
// source, each of source, residual and data at phases of their own, list
// lengths around the per-launch 92 and the per-call 1,024, empties and NULL
// empties) through the planner, checks the launch tables against the tile
// rule, the launch cut and the body flag restated here, and makes every
// refusal of the three checkers in the header's order.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 612;
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
constexpr int S = BINE_MX_EF_SEGS_PER_LAUNCH;

struct Lists {
  std::vector<uint64_t> src, res, d8, sc;
  std::vector<size_t> cnt;
};

static uint64_t check_plan(const Lists &l, int dtype, int fmt) {
  const int n = (int)l.cnt.size();
  const uint64_t esz = bine::adamw_esz(dtype), per = (fmt == BINE_MX_E2M1 ? 8 : 16) / esz;
  auto plan = [&](uint64_t *out, int64_t cap) {
    return bine_plan_mx_ef(n, l.src.data(), l.res.data(), l.d8.data(), l.sc.data(), l.cnt.data(), dtype, fmt, out, cap);
  };
  const int64_t segs = plan(nullptr, 0);
  REQUIRE(segs >= 0);
  std::vector<uint64_t> rec(5 * (size_t)segs + 5, 0xDEAD);
  REQUIRE(plan(rec.data(), segs) == segs);
  for (int j = 0; j < 5; j++) REQUIRE(rec[5 * (size_t)segs + j] == 0xDEAD);  // nothing past cap
  std::vector<bine::MxEfLaunch> ls;
  REQUIRE(bine::plan_mx_ef_launches(n, l.src.data(), l.res.data(), l.d8.data(), l.sc.data(), l.cnt.data(), dtype, fmt,
                                    ls) == BINE_SUCCESS);
  int next = 0;
  int64_t t = 0;
  uint64_t wgs = 0;
  for (size_t li = 0; li < ls.size(); li++) {
    const bine::MxEfLaunch &L = ls[li];
    REQUIRE(L.nseg >= 1 && L.nseg <= S && L.tile0[0] == 0);
    REQUIRE(li + 1 == ls.size() || L.nseg == S);  // only the last launch is short
    for (int s = 0; s < L.nseg; s++, t++, next++) {
      while (next < n && !l.cnt[next]) next++;
      REQUIRE(next < n && L.seg[s] == next && t < segs);
      const uint64_t want = (l.cnt[next] * esz + 32767) / 32768;
      const uint64_t body = l.src[next] % 16 || l.res[next] % 16 || l.d8[next] % per ? 1 : 0;
      REQUIRE(want >= 1 && L.tile0[s + 1] - L.tile0[s] == want);
      REQUIRE(((L.elem[s >> 6] >> (s & 63)) & 1) == body);
      const uint64_t *e = &rec[5 * (size_t)t];
      REQUIRE(e[0] == li && e[1] == (uint64_t)next && e[2] == L.tile0[s] && e[3] == want && e[4] == body);
    }
    wgs += L.tile0[L.nseg];
  }
  while (next < n && !l.cnt[next]) next++;
  REQUIRE(next == n && t == segs && ls.size() == (size_t)(segs + S - 1) / S);
  return wgs;
}

int main() {
  uint64_t wgs = 0, lists = 0;
  for (int dtype : kTypes)
    for (int fmt : kFmts) {
      const uint64_t esz = bine::adamw_esz(dtype), V = 16 / esz, tile = 32768 / esz;
      const size_t counts[] = {0, 1, 31, 32, 33, (size_t)tile - 32, (size_t)tile, (size_t)tile + 37, 2 * (size_t)tile + 32};
      // each of the three addresses at every phase of its own, the others aligned
      for (int which = 0; which < 3; which++)
        for (uint64_t ph = 0; ph < (which == 0 ? V : which == 1 ? 4 : 8); ph++) {
          Lists l;
          for (int k = 0; k < 9; k++) {
            l.cnt.push_back(counts[k]);
            l.src.push_back(0x10000000 + 0x100000ull * k + (which == 0 ? esz * ph : 0));
            l.res.push_back(0x30000000 + 0x100000ull * k + (which == 1 ? 4 * ph : 0));
            l.d8.push_back(0x50000000 + 0x100000ull * k + (which == 2 ? ph : 0));
            l.sc.push_back(0x70000001 + 0x100000ull * k);
          }
          wgs += check_plan(l, dtype, fmt);
          lists++;
        }
      for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
        Lists l;
        uint64_t a = 0x1000000;
        for (int k = 0; k < n; k++) {
          const size_t cnt = rnd() % 4 == 0 ? 0 : counts[1 + rnd() % (n > S + 1 ? 6 : 8)];
          const bool null = cnt == 0 && rnd() % 2;  // an empty tensor may be NULL
          l.cnt.push_back(cnt);
          l.src.push_back(null ? 0 : 0x100000000ull + a + esz * (rnd() % 2) * (rnd() % V));
          l.res.push_back(null ? 0 : 0x300000000ull + a + 4 * (rnd() % 2) * (rnd() % 4));
          l.d8.push_back(null ? 0 : 0x500000000ull + a + (rnd() % 2) * (rnd() % 8));
          l.sc.push_back(null ? 0 : 0x700000000ull + a + rnd() % 3);
          a += (cnt * 4 + 64) & ~(uint64_t)15;
        }
        wgs += check_plan(l, dtype, fmt);
        lists++;
      }
    }

  // bine_plan_mx_ef: the refusals
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 32);
  auto plan = [&](int n, const uint64_t *s, const uint64_t *r, const uint64_t *d, const uint64_t *sc, const size_t *cnt,
                  int dt = BINE_FLOAT, int fmt = BINE_MX_E4M3) {
    return bine_plan_mx_ef(n, s, r, d, sc, cnt, dt, fmt, nullptr, 0);
  };
  const uint64_t *A = a.data();
  REQUIRE(plan(BINE_MULTI_MAX + 1, A, A, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(BINE_MULTI_MAX, A, A, A, A, c.data()) == BINE_MULTI_MAX);
  REQUIRE(plan(-1, A, A, A, A, c.data()) == -BINE_ERR_ARG && plan(0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
  REQUIRE(plan(1, nullptr, A, A, A, c.data()) == -BINE_ERR_ARG && plan(1, A, nullptr, A, A, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, nullptr, A, c.data()) == -BINE_ERR_ARG && plan(1, A, A, A, nullptr, c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, A, A, nullptr) == -BINE_ERR_ARG);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((plan(1, A, A, A, A, c.data(), dtype) == 1) == ok);
  }
  for (int fmt = -2; fmt < 6; fmt++) REQUIRE((plan(1, A, A, A, A, c.data(), BINE_FLOAT, fmt) == 1) == (fmt >= 0 && fmt <= 2));
  const uint64_t zero = 0, odd = 0x1002, r1 = 0x2001, r2 = 0x2002, r4 = 0x2004;
  const size_t c33 = 33, c0 = 0, huge = (size_t)1 << 57;
  REQUIRE(plan(1, &zero, A, A, A, &c33) == -BINE_ERR_ARG && plan(1, A, &zero, A, A, &c33) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, A, &zero, A, &c33) == -BINE_ERR_ARG && plan(1, A, A, A, &zero, &c33) == -BINE_ERR_ARG);
  REQUIRE(plan(1, &zero, &zero, &zero, &zero, &c0) == 0);
  REQUIRE(plan(1, &odd, A, A, A, &c33) == -BINE_ERR_ARG && plan(1, &odd, A, A, A, &c33, BINE_FLOAT16) == 1);
  REQUIRE(plan(1, A, &r1, A, A, &c33) == -BINE_ERR_ARG && plan(1, A, &r2, A, A, &c33, BINE_BFLOAT16) == -BINE_ERR_ARG);
  REQUIRE(plan(1, A, &r4, A, A, &c33) == 1 && plan(1, A, A, A, A, &huge) == -BINE_ERR_ARG);

  // mx_ef_args, in the header's order
  void *sp[2] = {(void *)0x10000, (void *)0x11000}, *rp[2] = {(void *)0x20000, (void *)0x21004};
  void *dp[2] = {(void *)0x30000, (void *)0x31001}, *cp[2] = {(void *)0x40001, (void *)0x41002};
  void *nul[2] = {(void *)0x10000, nullptr}, *sodd[2] = {(void *)0x10002, (void *)0x11000};
  void *rodd[2] = {(void *)0x20000, (void *)0x21002};
  const size_t s2[2] = {33, 64}, z2[2] = {0, 0};
  const char *why = nullptr;
  std::vector<bine::MxEfLaunch> ml;
  auto ef = [&](int n, void *const *s, void *const *r, void *const *d, void *const *sc, const size_t *cnt, int dt,
                int fmt) {
    why = nullptr;
    return bine::mx_ef_args(n, s, r, d, sc, cnt, dt, fmt, &why, &ml);
  };
  REQUIRE(ef(2, sp, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_SUCCESS && ml.size() == 1 && ml[0].nseg == 2);
  REQUIRE(ml[0].elem[0] == 2);  // tensor 1: the residual 4 bytes off, the data one byte off
  REQUIRE(ef(2, sp, rp, dp, cp, s2, BINE_DOUBLE, 3) == BINE_ERR_ARG && strstr(why, "sdtype"));
  REQUIRE(ef(-1, nullptr, nullptr, nullptr, nullptr, nullptr, BINE_FLOAT, 3) == BINE_ERR_ARG && strstr(why, "fmt"));
  REQUIRE(ef(-1, sp, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG);
  REQUIRE(ef(BINE_MULTI_MAX + 1, sp, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG);
  REQUIRE(ef(2, nullptr, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(ef(2, sp, nullptr, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(ef(2, sp, rp, nullptr, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(ef(2, sp, rp, dp, nullptr, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(ef(2, sp, rp, dp, cp, nullptr, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(ef(2, nul, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(ef(2, sodd, nul, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(ef(2, sp, rp, nul, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && ef(2, sp, rp, dp, nul, s2, BINE_FLOAT, 0) == BINE_ERR_ARG);
  REQUIRE(ef(2, sodd, rp, dp, cp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && ef(2, sodd, rp, dp, cp, s2, BINE_FLOAT16, 0) == BINE_SUCCESS);
  REQUIRE(ef(2, sp, rodd, dp, cp, s2, BINE_BFLOAT16, 0) == BINE_ERR_ARG && strstr(why, "residual"));
  REQUIRE(ef(2, nul, nul, nul, nul, z2, BINE_FLOAT, 0) == BINE_SUCCESS && ml.empty());
  REQUIRE(ef(0, nullptr, nullptr, nullptr, nullptr, nullptr, BINE_FLOAT16, 2) == BINE_SUCCESS && ml.empty());

  // mx_ef_rs_args: mx_rs_args' order with res beside sbufs
  const size_t m2[2] = {32, 64}, m33[2] = {32, 33};
  const void *sw = (const void *)0x50000, *rw = (const void *)0x60000;
  uint64_t blk = 9;
  std::vector<uint64_t> off;
  auto rs = [&](int P, int n, void *const *s, void *const *r, void *const *d, const size_t *cnt, int sdt, int rdt,
                int fmt, const void *x, const void *y, size_t wsb) {
    why = nullptr;
    return bine::mx_ef_rs_args(P, n, s, r, d, cnt, sdt, rdt, fmt, x, y, wsb, &why, &blk, &off);
  };
  REQUIRE(rs(4, 2, sp, rp, dp, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 448) == BINE_ERR_ARG && strstr(why, "aligned"));
  void *dq[2] = {(void *)0x30000, (void *)0x31010};
  REQUIRE(rs(4, 2, sp, rp, dq, m2, BINE_FLOAT, BINE_BFLOAT16, 0, sw, rw, 448) == BINE_SUCCESS && blk == 112 && off[3] == 97);
  REQUIRE(rs(4, 2, sp, rp, dq, m2, BINE_FLOAT, BINE_BFLOAT16, 0, sw, rw, 447) == BINE_ERR_ARG && strstr(why, "ws_bytes"));
  REQUIRE(rs(1, 2, sp, rp, dq, m2, BINE_INT32, BINE_FLOAT, 3, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "sdtype"));
  REQUIRE(rs(1, -1, sp, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 3, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "fmt"));
  REQUIRE(rs(1, -1, sp, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, 2, nullptr, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(rs(1, 2, sp, nullptr, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(rs(1, 2, sp, rp, nullptr, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(rs(1, 2, sp, nul, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(rs(1, 2, sodd, nul, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(rs(1, 2, sodd, rodd, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "aligned") &&
          !strstr(why, "residual"));  // the source's alignment first
  REQUIRE(rs(1, 2, sp, rodd, dq, m33, BINE_FLOAT, BINE_FLOAT, 0, nullptr, rw, 112) == BINE_ERR_ARG && strstr(why, "residual"));
  REQUIRE(rs(1, 2, sp, rp, dq, m33, BINE_FLOAT, BINE_FLOAT, 0, nullptr, rw, 112) == BINE_ERR_ARG && strstr(why, "32"));
  REQUIRE(rs(1, 2, sp, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, nullptr, rw, 112) == BINE_ERR_ARG && strstr(why, "send_ws"));
  REQUIRE(rs(1, 2, sp, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, sw, 16) == BINE_ERR_ARG && strstr(why, "overlap"));
  REQUIRE(rs(16, 2, sp, rp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 16 * 112 - 1) == BINE_ERR_ARG && strstr(why, "ws_bytes"));
  REQUIRE(rs(16, 2, nul, nul, nul, z2, BINE_FLOAT, BINE_FLOAT, 0, nullptr, nullptr, 0) == BINE_SUCCESS && blk == 0);
  REQUIRE(rs(16, 0, nullptr, nullptr, nullptr, nullptr, BINE_FLOAT16, BINE_FLOAT16, 2, nullptr, nullptr, 0) == BINE_SUCCESS);
  // the plain call's checks are what they were: no residual list is looked at
  const void *const *csp = sp;
  REQUIRE(bine::mx_rs_args(1, 2, csp, dq, m2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112, &why, &blk, &off) == BINE_SUCCESS);
  printf("mxef_check: ok (%llu lists, %llu workgroups)\n", (unsigned long long)lists, (unsigned long long)wgs);
  return 0;
}
