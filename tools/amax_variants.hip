// amax_variants.hip -- on-box isolation of what k_amax_segs (pico_amd/csrc/kernels.hip)
// costs beyond its loads.  Standalone program, not part of the library: one
// 64 Mi-element float32 tensor (256 MiB, 16-B aligned), the library kernel's
// body -- a tile of 256 x 8 16-B vectors per workgroup, all loads issued before
// the first use, the wave butterfly and the LDS step -- with the END of the
// workgroup varied, each with and without the zeroing launch ahead of it:
//   store        thread 0 stores the workgroup's winner to scratch[t] and is done (the end
//                k_sumsq_segs has; the results are folded by nobody: a ceiling, not a candidate)
//   atomic       one atomic maximum per workgroup on out[0], no value returned
//   late         an agent-scope load of out[0] AFTER the barrier, the atomic only above it
//   early        that load issued BEFORE the tile's loads, compared after the barrier
//   early+late   the early value as a filter; only a winner above it loads again and may go atomic
// and `late` with 2 and 4 consecutive tiles per workgroup (fewer workgroups ending).
// The body here is a COPY of the library kernel's, without TileTable, head or
// tail: the figures are this program's, not bine_amax_segments'.  Without the
// zeroing launch out[0] keeps the previous call's maximum, so every workgroup
// of the load variants skips its atomic: those rows price the load, not the
// zeroing launch (the two `store` rows do that).
// hipEvents around each call, 20 timed calls after 5, 3 interleaved rounds, medians.
//   hipcc -O3 --offload-arch=gfx950 -o tools/bin/amax_variants tools/amax_variants.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#define CK(x)                                                                   \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

typedef unsigned int u4 __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256, kU = 8;
enum { STORE, ATOMIC, LATE, EARLY, EARLY_LATE };

__global__ void k_fill(uint32_t *x, size_t n) {  // positive floats below 8, hashed from the index
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint64_t h = (i + 1) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    x[i] = 0x3f800000u + (uint32_t)(h % 0x01800000u);
  }
}
__global__ void k_zero(uint32_t *out) { out[0] = 0; }

template <int END, int TPW>
__global__ __launch_bounds__(kBlock) void k_var(const u4 *vs, size_t nvec, uint32_t *out, uint32_t *scratch) {
  __shared__ uint32_t part[kBlock / 64];
  uint32_t seen = 0;
  if (END == EARLY || END == EARLY_LATE) seen = __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t acc = 0;
#pragma unroll 1
  for (int t = 0; t < TPW; t++) {
    const size_t base = ((size_t)blockIdx.x * TPW + t) * kBlock * kU + threadIdx.x;
    if (base + (kU - 1) * (size_t)kBlock >= nvec) break;  // the tensor is whole tiles
    u4 x[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) x[u] = vs[base + (size_t)u * kBlock];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const u4 v = x[u] & 0x7fffffffu;
      const uint32_t a = v.x > v.y ? v.x : v.y, b = v.z > v.w ? v.z : v.w, m = a > b ? a : b;
      acc = m > acc ? m : acc;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(acc, off, 64);
    acc = o > acc ? o : acc;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x) return;
  uint32_t w = part[0];
  for (int i = 1; i < kBlock / 64; i++) w = part[i] > w ? part[i] : w;
  if (END == STORE) scratch[blockIdx.x] = w;
  else if (END == ATOMIC) atomicMax(out, w);
  else if (END == LATE) {
    if (w > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, w);
  } else if (END == EARLY) {
    if (w > seen) atomicMax(out, w);
  } else {
    if (w > seen && w > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, w);
  }
}

int main() {
  const size_t n = (size_t)64 << 20, nvec = n / 4, tiles = nvec / (kBlock * kU);
  uint32_t *x, *out, *scratch;
  CK(hipMalloc(&x, n * 4));
  CK(hipMalloc(&out, 256));
  CK(hipMalloc(&scratch, tiles * 4));
  hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, x, n);
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  struct Var {
    std::string name;
    std::function<void()> run;
    std::vector<double> med;
  };
  std::vector<Var> vars;
  const u4 *vs = (const u4 *)x;
  auto add = [&](const char *name, auto kern, int tpw) {
    for (int zero = 1; zero >= 0; zero--)
      vars.push_back({std::string(name) + (zero ? ", zeroing launch ahead" : ", no zeroing launch"), [=] {
                        if (zero) hipLaunchKernelGGL(k_zero, dim3(1), dim3(1), 0, 0, out);
                        hipLaunchKernelGGL(kern, dim3((unsigned)(tiles / tpw)), dim3(kBlock), 0, 0, vs, nvec, out,
                                           scratch);
                      }, {}});
  };
  add("store", k_var<STORE, 1>, 1);
  add("atomic", k_var<ATOMIC, 1>, 1);
  add("late", k_var<LATE, 1>, 1);
  add("early", k_var<EARLY, 1>, 1);
  add("early+late", k_var<EARLY_LATE, 1>, 1);
  add("late, 2 tiles per workgroup", k_var<LATE, 2>, 2);
  add("late, 4 tiles per workgroup", k_var<LATE, 4>, 4);
  add("early+late, 4 tiles per workgroup", k_var<EARLY_LATE, 4>, 4);
  // every variant that ends in out[0] gives the same maximum
  uint32_t want = 0;
  for (Var &v : vars) {
    if (v.name.rfind("store", 0) == 0) continue;
    hipLaunchKernelGGL(k_zero, dim3(1), dim3(1), 0, 0, out);
    v.run();
    uint32_t got;
    CK(hipMemcpy(&got, out, 4, hipMemcpyDeviceToHost));
    if (!want) want = got;
    if (got != want || !got) {
      fprintf(stderr, "%s: maximum %08x, expected %08x\n", v.name.c_str(), got, want);
      return 1;
    }
  }
  printf("64 Mi float32 (256 MiB), %zu tiles; maximum pattern %08x in every variant; us per call "
         "(zeroing launch included where there is one), median of 20 after 5 warm-up, 3 interleaved rounds\n",
         tiles, want);
  for (int rnd = 0; rnd < 3; rnd++)
    for (Var &v : vars) {
      std::vector<float> t;
      for (int i = 0; i < 25; i++) {
        CK(hipEventRecord(e0, 0));
        v.run();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (i >= 5) t.push_back(ms * 1000.0f);
      }
      std::sort(t.begin(), t.end());
      v.med.push_back((t[9] + t[10]) / 2);
    }
  for (Var &v : vars) {
    std::sort(v.med.begin(), v.med.end());
    printf("  %-52s %7.2f us  (rounds %.2f .. %.2f)\n", v.name.c_str(), v.med[1], v.med[0], v.med[2]);
  }
  return 0;
}
