// sumsq_check.cpp -- the planner of the segmented sum of squares and the segmented
// scale (pico_amd/csrc/segments.cpp, host only) as a stand-alone program, for the
// host sanitizers:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ipico_amd/csrc tools/sumsq_check.cpp pico_amd/csrc/segments.cpp -o tools/bin/sumsq_check
//   tools/bin/sumsq_check
//
// It walks tensor lists of tests/test_norm.py's kind (the nine counts per type,
// all 16 phases -- those that are no multiple of the element size must be
// refused -- list lengths around the per-launch 128 and the per-call 1,024,
// empties and NULL empties) through bine_plan_sumsq and plan_norm_launches,
// checks the launch tables against the tile rule restated here (every vector of
// every tensor in exactly one workgroup, the launches' grids summing to the
// scratch size), and the refusals.  CPU only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "bine_internal.h"

static uint64_t g_state = 20251;
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

static const int kTypes[] = {BINE_FLOAT, BINE_DOUBLE, BINE_FLOAT16, BINE_BFLOAT16};

static uint64_t tiles_of(uint64_t addr, uint64_t bytes) {
  if (!bytes) return 0;
  uint64_t head = (16 - addr % 16) % 16;
  if (head > bytes) head = bytes;
  const uint64_t nvec = (bytes - head) / 16, t = (nvec + 2047) / 2048;
  return t ? t : 1;
}

// the table of one list against the rule; returns its workgroups
static int64_t check(int dtype, const std::vector<uint64_t> &addr, const std::vector<size_t> &cnt) {
  const int n = (int)cnt.size();
  const size_t esz = bine::norm_esz(dtype);
  const int64_t need = bine_plan_sumsq(n, addr.data(), cnt.data(), dtype);
  REQUIRE(need >= 0);
  std::vector<bine::SegLaunch> ls;
  uint64_t tiles = 0;
  REQUIRE(bine::plan_norm_launches(n, addr.data(), cnt.data(), dtype, ls, &tiles) == BINE_SUCCESS);
  REQUIRE((int64_t)tiles == need);
  int next = 0, nonempty = 0;  // the segments appear in list order, the empty ones left out
  uint64_t sum = 0;
  for (const bine::SegLaunch &L : ls) {
    REQUIRE(L.nseg >= 1 && L.nseg <= BINE_COPY_SEGS_PER_LAUNCH && L.tile0[0] == 0);
    for (int s = 0; s < L.nseg; s++) {
      while (next < n && !cnt[next]) next++;
      REQUIRE(next < n && L.seg[s] == next);
      const uint64_t bytes = cnt[next] * esz, want = tiles_of(addr[next], bytes);
      REQUIRE(L.tile0[s + 1] - L.tile0[s] == want);
      REQUIRE(L.head[s] + 16 * L.nvec[s] <= bytes && bytes - L.head[s] - 16 * L.nvec[s] < 16);
      REQUIRE((addr[next] + L.head[s]) % 16 == 0 || L.nvec[s] == 0);
      REQUIRE(L.head[s] % esz == 0);  // whole elements before the first vector
      next++, nonempty++;
    }
    sum += L.tile0[L.nseg];
  }
  while (next < n && !cnt[next]) next++;
  REQUIRE(next == n && sum == tiles);
  REQUIRE(ls.size() == (size_t)(nonempty + BINE_COPY_SEGS_PER_LAUNCH - 1) / BINE_COPY_SEGS_PER_LAUNCH);
  return need;
}

int main() {
  const int S = BINE_COPY_SEGS_PER_LAUNCH;
  int64_t tiles = 0;
  for (int dtype : kTypes) {
    const size_t esz = bine::norm_esz(dtype), vec = 16 / esz, tile = 2048 * vec;
    REQUIRE(esz);
    const size_t counts[] = {0, 1, vec - 1, vec, vec + 1, tile - 1, tile, tile + 1, 3 * tile + 21};
    // all 16 phases: the misaligned ones are refused, the others follow the rule
    for (uint64_t phase = 0; phase < 16; phase++) {
      std::vector<uint64_t> addr;
      std::vector<size_t> cnt(counts, counts + 9);
      for (int k = 0; k < 9; k++) addr.push_back(0x7000000 + 0x100000ull * k + phase);
      if (phase % esz) {
        REQUIRE(bine_plan_sumsq(9, addr.data(), cnt.data(), dtype) == -BINE_ERR_ARG);
        std::vector<bine::SegLaunch> ls;
        REQUIRE(bine::plan_norm_launches(9, addr.data(), cnt.data(), dtype, ls, nullptr) == BINE_ERR_ARG);
        continue;
      }
      tiles += check(dtype, addr, cnt);
    }
    // list lengths around a launch's 128 segments and the call's 1,024
    for (int n : {0, 1, S - 1, S, S + 1, 2 * S + 37, BINE_MULTI_MAX - 1, BINE_MULTI_MAX}) {
      std::vector<uint64_t> addr(n);
      std::vector<size_t> cnt(n);
      uint64_t a = 0x10000000;
      for (int k = 0; k < n; k++) {
        cnt[k] = rnd() % 4 == 0 ? 0 : counts[rnd() % (n > S + 1 ? 7 : 9)];
        addr[k] = cnt[k] == 0 && rnd() % 2 ? 0 : a + (rnd() % vec) * esz;  // an empty tensor may be NULL
        a += (cnt[k] * esz + 64) & ~(uint64_t)15;
      }
      tiles += check(dtype, addr, cnt);
    }
  }
  // the refusals
  std::vector<uint64_t> a(BINE_MULTI_MAX + 1, 0x1000);
  std::vector<size_t> c(BINE_MULTI_MAX + 1, 4);
  REQUIRE(bine_plan_sumsq(BINE_MULTI_MAX + 1, a.data(), c.data(), BINE_FLOAT) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_sumsq(BINE_MULTI_MAX, a.data(), c.data(), BINE_FLOAT) == BINE_MULTI_MAX);
  REQUIRE(bine_plan_sumsq(-1, a.data(), c.data(), BINE_FLOAT) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_sumsq(1, nullptr, c.data(), BINE_FLOAT) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_sumsq(1, a.data(), nullptr, BINE_FLOAT) == -BINE_ERR_ARG);
  for (int dtype = -1; dtype < 48; dtype++) {
    const bool ok = dtype == BINE_FLOAT || dtype == BINE_DOUBLE || dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16;
    REQUIRE((bine_plan_sumsq(1, a.data(), c.data(), dtype) == 1) == ok);
    REQUIRE(ok || bine_plan_sumsq(-1, nullptr, nullptr, dtype) == -BINE_ERR_ARG);
  }
  const uint64_t zero = 0, odd = 0x1002;
  const size_t one = 1, none = 0, huge = (size_t)1 << 57;
  REQUIRE(bine_plan_sumsq(1, &zero, &one, BINE_FLOAT) == -BINE_ERR_ARG);  // NULL with a non-zero count
  REQUIRE(bine_plan_sumsq(1, &zero, &none, BINE_FLOAT) == 0);             // empty: may be NULL
  REQUIRE(bine_plan_sumsq(1, &odd, &one, BINE_FLOAT) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_sumsq(1, &odd, &one, BINE_BFLOAT16) == 1);
  REQUIRE(bine_plan_sumsq(1, &odd, &none, BINE_FLOAT) == 0);
  REQUIRE(bine_plan_sumsq(1, a.data(), &huge, BINE_FLOAT) == -BINE_ERR_ARG);
  REQUIRE(bine_plan_sumsq(0, nullptr, nullptr, BINE_DOUBLE) == 0);
  printf("sumsq_check: ok (%lld workgroups)\n", (long long)tiles);
  return 0;
}
