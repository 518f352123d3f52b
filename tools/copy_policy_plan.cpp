// copy_policy_plan.cpp -- the arithmetic launch_copy hands to k_copy as keep_vecs
// (bine_internal.h: copy_keep_policy, copy_keep_vecs), swept on the host; no HIP.
// tests/test_copy_policy_plan.py builds it with g++ and the host sanitizers.
//   g++ -std=c++17 -fsanitize=address,undefined -I include -I pico_amd/csrc \
//       tools/copy_policy_plan.cpp -o copy_policy_plan
#include <cstdio>
#include <cstring>

#include "bine_internal.h"

using namespace bine;

static int bad = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) bad++, printf("FAILED line %d: %s\n", __LINE__, #c); \
  } while (0)

int main() {
  const uint64_t MiB = 1ull << 20, defKeep = 192 * MiB, defMin = 128 * MiB;
  // the environment: unset, empty and junk give the defaults; a number replaces
  // the kept bytes and drops the size threshold
  for (const char *e : {(const char *)nullptr, "", "x", "1x", "-1", "nan", " "}) {
    const CopyKeep p = copy_keep_policy(e, defKeep, defMin);
    EXPECT(p.keep_bytes == defKeep && p.min_bytes == defMin);
  }
  struct {
    const char *env;
    uint64_t bytes;
  } set[] = {{"0", 0},         {"0.0", 0},           {"1", MiB},       {"0.015625", 16384}, {"0.03125", 32768},
             {"192", defKeep}, {"0.03814697265625", 40000}, {"1e30", 1ull << 60}, {"inf", 1ull << 60}};
  for (const auto &c : set) {
    const CopyKeep p = copy_keep_policy(c.env, defKeep, defMin);
    EXPECT(p.keep_bytes == c.bytes && p.min_bytes == 0);
  }
  // keep_vecs: 0 below the threshold, never above nvec, keep_bytes / 16 otherwise
  const uint64_t sizes[] = {0,       1,        15,        16,           17,           32752,          32768,         32784,
                            98309,   defMin - 1, defMin,  defMin + 1,   defKeep - 16, defKeep,        defKeep + 16,  256 * MiB,
                            (1ull << 32) + 5, 1ull << 40};
  const CopyKeep pols[] = {{defKeep, defMin}, {0, 0},     {16384, 0},       {32768, 0},       {40000, 0},
                           {MiB, 0},          {15, 0},    {1ull << 60, 0},  {defKeep, 0},     {0, defMin}};
  long checked = 0;
  for (const CopyKeep &p : pols)
    for (uint64_t bytes : sizes)
      for (uint64_t head = 0; head < 16; head++) {  // every destination phase
        const uint64_t h = head < bytes ? head : bytes, nvec = (bytes - h) / 16;
        const uint64_t k = copy_keep_vecs(bytes, nvec, p);
        EXPECT(k <= nvec);
        if (bytes < p.min_bytes) EXPECT(k == 0);
        if (bytes >= p.min_bytes) EXPECT(k == (p.keep_bytes / 16 < nvec ? p.keep_bytes / 16 : nvec));
        if (p.keep_bytes < 16) EXPECT(k == 0);
        checked++;
      }
  // the shipped policy at the benchmark's copy and just under the threshold
  const CopyKeep d = copy_keep_policy(nullptr, defKeep, defMin);
  EXPECT(copy_keep_vecs(256 * MiB, 256 * MiB / 16, d) == defKeep / 16);
  EXPECT(copy_keep_vecs(defMin, defMin / 16, d) == defMin / 16);
  EXPECT(copy_keep_vecs(defMin - 16, defMin / 16 - 1, d) == 0);
  printf("RESULT checked=%ld bad=%d\n", checked, bad);
  return bad != 0;
}
