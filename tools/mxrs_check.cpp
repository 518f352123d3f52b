// mxrs_check.cpp -- the host side of the MX-quantized gradient reduce-scatter
// (pico_amd/csrc/segments.cpp: mx_wire_layout / bine_mx_wire_bytes,
// plan_mx_sum_launches / bine_plan_mx_sum, mx_sum_args, mx_rs_args) as a
// stand-alone program, for the host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/mxrs_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/mxrs_check
//   tools/bin/mxrs_check
//
// It walks buckets of tests/test_mxrs.py's kind (counts around one tile of the
// destination at every element phase, list lengths around the per-launch 112
// and the per-call 1,024, empties and NULL empties) through the wire layout
// and the planner, checks offsets, D and B against the layout restated here
// and the launch tables against the tile rule, the launch cut and the body
// flag, and makes every refusal, the overflowing sums included.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 611;
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

static uint64_t dbytes(uint64_t c, int fmt) { return fmt == BINE_MX_E2M1 ? c / 2 : c; }

// the layout against its statement in bine_amd.h; returns B
static uint64_t check_layout(const std::vector<size_t> &cnt, int fmt) {
  const int n = (int)cnt.size();
  size_t D = 1, B = 1;
  REQUIRE(bine_mx_wire_bytes(n, cnt.data(), fmt, &D, &B) == BINE_SUCCESS);
  std::vector<uint64_t> off;
  uint64_t d2 = 1, b2 = 1;
  REQUIRE(bine::mx_wire_layout(n, cnt.data(), fmt, &off, &d2, &b2) == BINE_SUCCESS && d2 == D && b2 == B);
  REQUIRE(off.size() == 2 * (size_t)n);
  uint64_t d = 0, s = 0;
  for (int k = 0; k < n; k++) {
    REQUIRE(off[k] == d && off[k] % 16 == 0);
    d += dbytes(cnt[k], fmt);
    s += cnt[k] / 32;
  }
  REQUIRE(D == d && B % 16 == 0 && B >= d + s && B - (d + s) < 16);
  s = 0;
  for (int k = 0; k < n; k++) {
    REQUIRE(off[(size_t)n + k] == d + s);
    s += cnt[k] / 32;
  }
  return B;
}

static uint64_t check_plan(const std::vector<uint64_t> &dst, const std::vector<size_t> &cnt, int dtype, int fmt) {
  const int n = (int)cnt.size();
  const uint64_t esz = bine::adamw_esz(dtype);
  const int64_t segs = bine_plan_mx_sum(n, dst.data(), cnt.data(), dtype, fmt, nullptr, 0);
  REQUIRE(segs >= 0);
  std::vector<uint64_t> rec(5 * (size_t)segs + 5, 0xDEAD);
  REQUIRE(bine_plan_mx_sum(n, dst.data(), cnt.data(), dtype, fmt, rec.data(), segs) == segs);
  for (int j = 0; j < 5; j++) REQUIRE(rec[5 * (size_t)segs + j] == 0xDEAD);  // nothing past cap
  std::vector<bine::MxLaunch> ls;
  REQUIRE(bine::plan_mx_sum_launches(n, dst.data(), cnt.data(), dtype, fmt, ls) == BINE_SUCCESS);
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
      const uint64_t want = (cnt[next] * esz + 32767) / 32768, body = dst[next] % 16 ? 1 : 0;
      REQUIRE(want >= 1 && L.tile0[s + 1] - L.tile0[s] == want);
      REQUIRE(((L.elem[s >> 6] >> (s & 63)) & 1) == body);
      const uint64_t *e = &rec[5 * (size_t)t];
      REQUIRE(e[0] == li && e[1] == (uint64_t)next && e[2] == L.tile0[s] && e[3] == want && e[4] == body);
    }
    wgs += L.tile0[L.nseg];
  }
  while (next < n && !cnt[next]) next++;
  REQUIRE(next == n && t == segs && ls.size() == (size_t)(segs + S - 1) / S);
  return wgs;
}

int main() {
  uint64_t wgs = 0, bytes = 0;
  for (int dtype : kTypes)
    for (int fmt : kFmts) {
      const uint64_t esz = bine::adamw_esz(dtype), V = 16 / esz, tile = 32768 / esz;
      const size_t counts[] = {0, 32, 64, (size_t)tile - 32, (size_t)tile, (size_t)tile + 32, 2 * (size_t)tile + 32};
      for (uint64_t ph = 0; ph < V; ph++) {
        std::vector<uint64_t> d;
        std::vector<size_t> c(counts, counts + 7);
        for (int k = 0; k < 7; k++) d.push_back(0x10000000 + 0x100000ull * k + esz * ph);
        wgs += check_plan(d, c, dtype, fmt);
        bytes += check_layout(c, fmt);
      }
      for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
        std::vector<uint64_t> d;
        std::vector<size_t> c;
        uint64_t a = 0x1000000;
        for (int k = 0; k < n; k++) {
          const size_t cnt = rnd() % 4 == 0 ? 0 : counts[rnd() % (n > S + 1 ? 5 : 7)];
          const bool null = cnt == 0 && rnd() % 2;  // an empty tensor may be NULL
          c.push_back(cnt);
          d.push_back(null ? 0 : 0x100000000ull + a + esz * (rnd() % 2) * (rnd() % V));
          a += (cnt * 4 + 64) & ~(uint64_t)15;
        }
        wgs += check_plan(d, c, dtype, fmt);
        bytes += check_layout(c, fmt);
      }
    }

  // bine_mx_wire_bytes: the refusals, the sums that wrap
  size_t D = 7, B = 7;
  const size_t ok2[2] = {32, 64}, bad2[2] = {32, 33};
  const size_t top = (size_t)0 - 32;
  const size_t wrap2[2] = {top, 32}, top1[1] = {top}, top2[2] = {top, top};
  REQUIRE(bine_mx_wire_bytes(2, ok2, 0, &D, &B) == BINE_SUCCESS && D == 96 && B == 112);
  REQUIRE(bine_mx_wire_bytes(2, ok2, 2, &D, &B) == BINE_SUCCESS && D == 48 && B == 64);
  REQUIRE(bine_mx_wire_bytes(0, nullptr, 1, &D, &B) == BINE_SUCCESS && D == 0 && B == 0);
  REQUIRE(bine_mx_wire_bytes(2, ok2, 3, &D, &B) == BINE_ERR_ARG && bine_mx_wire_bytes(2, ok2, -1, &D, &B) == BINE_ERR_ARG);
  REQUIRE(bine_mx_wire_bytes(2, ok2, 0, nullptr, &B) == BINE_ERR_ARG && bine_mx_wire_bytes(2, ok2, 0, &D, nullptr) == BINE_ERR_ARG);
  REQUIRE(bine_mx_wire_bytes(-1, ok2, 0, &D, &B) == BINE_ERR_ARG && bine_mx_wire_bytes(2, nullptr, 0, &D, &B) == BINE_ERR_ARG);
  REQUIRE(bine_mx_wire_bytes(2, bad2, 0, &D, &B) == BINE_ERR_ARG);
  REQUIRE(bine_mx_wire_bytes(2, wrap2, 0, &D, &B) == BINE_ERR_ARG && bine_mx_wire_bytes(1, top1, 0, &D, &B) == BINE_ERR_ARG);
  REQUIRE(bine_mx_wire_bytes(1, top1, 2, &D, &B) == BINE_SUCCESS && D == top / 2);
  REQUIRE(bine_mx_wire_bytes(2, top2, 2, &D, &B) == BINE_ERR_ARG);

  // bine_plan_mx_sum: the refusals
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 32);
  auto plan = [&](int n, const uint64_t *d, const size_t *cnt, int dt = BINE_FLOAT, int fmt = BINE_MX_E4M3) {
    return bine_plan_mx_sum(n, d, cnt, dt, fmt, nullptr, 0);
  };
  REQUIRE(plan(BINE_MULTI_MAX + 1, a.data(), c.data()) == -BINE_ERR_ARG);
  REQUIRE(plan(BINE_MULTI_MAX, a.data(), c.data()) == BINE_MULTI_MAX);
  REQUIRE(plan(-1, a.data(), c.data()) == -BINE_ERR_ARG && plan(0, nullptr, nullptr) == 0);
  REQUIRE(plan(1, nullptr, c.data()) == -BINE_ERR_ARG && plan(1, a.data(), nullptr) == -BINE_ERR_ARG);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((plan(1, a.data(), c.data(), dtype) == 1) == ok);
  }
  for (int fmt = -2; fmt < 6; fmt++) REQUIRE((plan(1, a.data(), c.data(), BINE_FLOAT, fmt) == 1) == (fmt >= 0 && fmt <= 2));
  const uint64_t zero = 0, odd = 0x1002;
  const size_t c32 = 32, c0 = 0, c33 = 33, huge = (size_t)1 << 57;
  REQUIRE(plan(1, &zero, &c32) == -BINE_ERR_ARG && plan(1, &zero, &c0) == 0);
  REQUIRE(plan(1, &odd, &c32) == -BINE_ERR_ARG && plan(1, &odd, &c32, BINE_FLOAT16) == 1);
  REQUIRE(plan(1, a.data(), &c33) == -BINE_ERR_ARG && plan(1, a.data(), &huge) == -BINE_ERR_ARG);

  // mx_sum_args, in the header's order
  void *dp[2] = {(void *)0x1000, (void *)0x2010};
  const size_t s2[2] = {32, 64}, s33[2] = {32, 33}, z2[2] = {0, 0};
  const void *pk = (const void *)0x9000;
  const char *why = nullptr;
  std::vector<bine::MxLaunch> ml;
  std::vector<uint64_t> off;
  auto sum = [&](int n, int ns, const void *p, size_t blk, void *const *d, const size_t *cnt, int dt, int fmt) {
    why = nullptr;
    return bine::mx_sum_args(n, ns, p, blk, d, cnt, dt, fmt, &why, &ml, &off);
  };
  REQUIRE(sum(2, 16, pk, 112, dp, s2, BINE_FLOAT, 0) == BINE_SUCCESS && ml.size() == 1 && ml[0].nseg == 2);
  REQUIRE(off.size() == 4 && off[0] == 0 && off[1] == 32 && off[2] == 96 && off[3] == 97 && ml[0].elem[0] == 0);
  REQUIRE(sum(2, 1, pk, 112, dp, s2, BINE_DOUBLE, 3) == BINE_ERR_ARG && strstr(why, "ddtype"));
  REQUIRE(sum(-1, 0, nullptr, 0, nullptr, nullptr, BINE_FLOAT, 3) == BINE_ERR_ARG && strstr(why, "fmt"));
  REQUIRE(sum(-1, 1, pk, 112, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG);
  REQUIRE(sum(BINE_MULTI_MAX + 1, 1, pk, 112, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG);
  REQUIRE(sum(2, 1, pk, 112, nullptr, s33, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(sum(2, 1, pk, 112, dp, nullptr, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL array"));
  void *dnull[2] = {(void *)0x1000, nullptr}, *dodd[2] = {(void *)0x1002, (void *)0x2000};
  REQUIRE(sum(2, 1, pk, 112, dnull, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(sum(2, 0, pk, 112, dodd, s33, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "aligned"));
  REQUIRE(sum(2, 0, pk, 112, dodd, s2, BINE_BFLOAT16, 0) == BINE_ERR_ARG && strstr(why, "nstreams") && ml[0].elem[0] == 1);
  REQUIRE(sum(2, 0, nullptr, 0, dp, s33, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "32") && ml.empty());
  REQUIRE(sum(2, 0, nullptr, 0, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "nstreams"));
  REQUIRE(sum(2, 17, nullptr, 0, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "nstreams"));
  REQUIRE(sum(2, 1, nullptr, 0, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "packed"));
  REQUIRE(sum(2, 1, (const void *)0x9008, 0, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "packed"));
  REQUIRE(sum(2, 1, pk, 96, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "block_bytes"));
  REQUIRE(sum(2, 1, pk, 120, dp, s2, BINE_FLOAT, 0) == BINE_ERR_ARG && strstr(why, "block_bytes"));
  REQUIRE(sum(2, 1, pk, 128, dp, s2, BINE_FLOAT, 0) == BINE_SUCCESS);
  REQUIRE(sum(2, 1, nullptr, 0, dnull, z2, BINE_FLOAT, 0) == BINE_SUCCESS && ml.empty());
  REQUIRE(sum(0, 1, nullptr, 0, nullptr, nullptr, BINE_FLOAT16, 2) == BINE_SUCCESS && ml.empty());

  // mx_rs_args, in the header's order
  void *sp[2] = {(void *)0x10000, (void *)0x11000};
  const void *const *csp = sp;
  const void *sw = (const void *)0x40000, *rw = (const void *)0x50000;
  uint64_t blk = 9;
  auto rs = [&](int P, int n, const void *const *s, void *const *r, const size_t *cnt, int sdt, int rdt, int fmt,
                const void *a, const void *b, size_t wsb) {
    why = nullptr;
    return bine::mx_rs_args(P, n, s, r, cnt, sdt, rdt, fmt, a, b, wsb, &why, &blk, &off);
  };
  REQUIRE(rs(4, 2, csp, dp, s2, BINE_FLOAT, BINE_BFLOAT16, 0, sw, rw, 448) == BINE_SUCCESS && blk == 112 && off[3] == 97);
  REQUIRE(rs(4, 2, csp, dp, s2, BINE_FLOAT, BINE_BFLOAT16, 0, sw, rw, 447) == BINE_ERR_ARG && strstr(why, "ws_bytes"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_SUCCESS);
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_INT32, BINE_FLOAT, 3, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "sdtype"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_DOUBLE, 3, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "rdtype"));
  REQUIRE(rs(1, -1, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 3, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "fmt"));
  REQUIRE(rs(1, -1, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, BINE_MULTI_MAX + 1, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, 2, nullptr, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL array"));
  REQUIRE(rs(1, 2, csp, nullptr, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, 2, csp, dp, nullptr, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, 2, csp, dnull, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "NULL buffer"));
  REQUIRE(rs(1, 2, csp, dodd, s33, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "aligned"));
  REQUIRE(rs(1, 2, csp, dodd, s2, BINE_FLOAT, BINE_FLOAT16, 0, nullptr, rw, 112) == BINE_ERR_ARG && strstr(why, "send_ws"));
  REQUIRE(rs(1, 2, csp, dp, s33, BINE_FLOAT, BINE_FLOAT, 0, nullptr, rw, 112) == BINE_ERR_ARG && strstr(why, "32"));
  const size_t big2[2] = {(size_t)1 << 31, 32};
  REQUIRE(rs(1, 2, csp, dp, big2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 112) == BINE_ERR_ARG && strstr(why, "INT_MAX"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, nullptr, 112) == BINE_ERR_ARG && strstr(why, "recv_ws"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, (const void *)0x40004, rw, 112) == BINE_ERR_ARG);
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, sw, 16) == BINE_ERR_ARG && strstr(why, "overlap"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, (const void *)0x40070, 128) == BINE_ERR_ARG && strstr(why, "overlap"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, (const void *)0x50070, rw, 128) == BINE_ERR_ARG && strstr(why, "overlap"));
  REQUIRE(rs(1, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, (const void *)0x40070, 112) == BINE_SUCCESS);  // adjacent
  REQUIRE(rs(16, 2, csp, dp, s2, BINE_FLOAT, BINE_FLOAT, 0, sw, rw, 16 * 112 - 1) == BINE_ERR_ARG && strstr(why, "ws_bytes"));
  REQUIRE(rs(16, 2, csp, dnull, z2, BINE_FLOAT, BINE_FLOAT, 0, nullptr, nullptr, 0) == BINE_SUCCESS && blk == 0);
  REQUIRE(rs(16, 0, nullptr, nullptr, nullptr, BINE_FLOAT16, BINE_FLOAT16, 2, nullptr, nullptr, 0) == BINE_SUCCESS && blk == 0);
  printf("mxrs_check: ok (%llu workgroups, %llu block bytes)\n", (unsigned long long)wgs, (unsigned long long)bytes);
  return 0;
}
