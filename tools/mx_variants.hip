// mx_variants.hip -- what gfx950's scaled conversions do, against the forms
// k_mx_segs keeps (pico_amd/csrc/kernels.hip).  Stand-alone:
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/mx_variants.hip -o tools/bin/mx_variants
//   tools/bin/mx_variants > profiles/mx_variants.txt
//
// One thread per (x, S) pair computes
//   A  FP8: y = x * 2^(127 - S), clamp to +-FMAX, v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32   (kept: quant4)
//   B  FP8: v_cvt_scalef32_pk_fp8_f32 / _bf8_f32 of x with the scale 2^(S - 127) fed directly
//   C  FP4: y by the same product, the thresholds counted in plain comparisons              (kept: fp4_enc1)
//   D  FP4: v_cvt_scalef32_pk_fp4_f32 of the clamped y with scale 1
//   E  FP4: v_cvt_scalef32_pk_fp4_f32 of x with the scale 2^(S - 127) fed directly
// x runs over every bfloat16 pattern with three fills of the low half; S over
// a handful of scale bytes.  Only LEGAL pairs count -- those a block with this
// S can hold: |y| < 2^(emax + 1), x finite -- split by whether y is a normal
// binary32 number, since below 2^-126 the product is not exact and the contract
// asks for a zero.  The second operand of every packed conversion is the
// first's negation, so the high byte / nibble and the sign are covered too.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(e)                                                                \
  do {                                                                          \
    hipError_t err_ = (e);                                                      \
    if (err_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(err_)); \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

typedef short s16x2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ uint32_t lo16(V v) {
  uint32_t w;
  __builtin_memcpy(&w, &v, 4);
  return w & 0xffffu;
}

__device__ __forceinline__ float pow2(uint32_t biased) {
  const uint32_t b = biased ? biased << 23 : 0x00400000u;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

__device__ __forceinline__ uint32_t fp4_enc1(float y) {
  uint32_t b;
  __builtin_memcpy(&b, &y, 4);
  const float a = __builtin_fabsf(y);
  const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                     (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return c | ((b >> 28) & 8u);
}

// out[5 * i + v]: variant v's two codes (x in the low byte / nibble, -x above it)
__global__ void k_variants(const float *x, const uint32_t *S, size_t n, uint32_t *out) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = x[i], f = pow2(254u - S[i]), sc = pow2(S[i]);
  const float y = a * f;
  const s16x2 z = {0, 0};
  // e4m3 in out[0..1], e5m2 in the upper halves
  const float c8 = fminf(fmaxf(y, -448.0f), 448.0f), c5 = fminf(fmaxf(y, -57344.0f), 57344.0f);
  const uint32_t A8 = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c8, -c8, 0, false) & 0xffffu;
  const uint32_t A5 = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(c5, -c5, 0, false) & 0xffffu;
  const uint32_t B8 = lo16(__builtin_amdgcn_cvt_scalef32_pk_fp8_f32(z, a, -a, sc, false));
  const uint32_t B5 = lo16(__builtin_amdgcn_cvt_scalef32_pk_bf8_f32(z, a, -a, sc, false));
  const float c4 = fminf(fmaxf(y, -6.0f), 6.0f);
  const uint32_t C = fp4_enc1(y) | (fp4_enc1(-y) << 4);
  const uint32_t D = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, c4, -c4, 1.0f, 0) & 0xffu;
  const uint32_t E = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(0u, a, -a, sc, 0) & 0xffu;
  out[5 * i + 0] = A8 | (A5 << 16);
  out[5 * i + 1] = B8 | (B5 << 16);
  out[5 * i + 2] = C;
  out[5 * i + 3] = D;
  out[5 * i + 4] = E;
}

int main() {
  const uint32_t scales[] = {0, 1, 2, 60, 126, 127, 128, 200, 251, 252};
  const uint32_t fills[] = {0x0000u, 0x8000u, 0xffffu};
  std::vector<float> x;
  std::vector<uint32_t> S;
  for (uint32_t s : scales)
    for (uint32_t fill : fills)
      for (uint32_t p = 0; p < 65536; p++) {
        const uint32_t b = p << 16 | fill;
        float v;
        memcpy(&v, &b, 4);
        x.push_back(v);
        S.push_back(s);
      }
  const size_t n = x.size();
  float *dx;
  uint32_t *dS, *dout;
  CHECK(hipMalloc(&dx, n * 4));
  CHECK(hipMalloc(&dS, n * 4));
  CHECK(hipMalloc(&dout, n * 20));
  CHECK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dS, S.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_variants, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dS, n, dout);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  std::vector<uint32_t> out(5 * n);
  CHECK(hipMemcpy(out.data(), dout, n * 20, hipMemcpyDeviceToHost));

  struct Row {
    const char *name;
    int emax, ref, var, shift;
    uint32_t mask;
  };
  const Row rows[] = {
      {"B e4m3: scalef32_pk_fp8, S direct   vs clamp + cvt_pk_fp8", 8, 0, 1, 0, 0xffffu},
      {"B e5m2: scalef32_pk_bf8, S direct   vs clamp + cvt_pk_bf8", 15, 0, 1, 16, 0xffffu},
      {"D e2m1: scalef32_pk_fp4, scale 1    vs comparisons", 2, 2, 3, 0, 0xffu},
      {"E e2m1: scalef32_pk_fp4, S direct   vs comparisons", 2, 2, 4, 0, 0xffu},
  };
  for (const Row &r : rows) {
    uint64_t legal_n = 0, bad_n = 0, legal_t = 0, bad_t = 0;
    int shown = 0;
    for (size_t i = 0; i < n; i++) {
      if (!std::isfinite(x[i])) continue;
      const double y = std::ldexp((double)x[i], 127 - (int)S[i]);
      if (!(std::fabs(y) < std::ldexp(1.0, r.emax + 1))) continue;
      const bool tiny = y != 0.0 && std::fabs(y) < std::ldexp(1.0, -126);
      const uint32_t want = (out[5 * i + r.ref] >> r.shift) & r.mask, got = (out[5 * i + r.var] >> r.shift) & r.mask;
      (tiny ? legal_t : legal_n)++;
      if (want != got) {
        (tiny ? bad_t : bad_n)++;
        if (shown++ < 4) {
          uint32_t b;
          memcpy(&b, &x[i], 4);
          printf("    x = 0x%08x  S = %3u  y = %-14.8g kept 0x%04x  variant 0x%04x\n", b, S[i], y, want, got);
        }
      }
    }
    printf("%s: %llu of %llu legal pairs differ; below 2^-126: %llu of %llu\n", r.name, (unsigned long long)bad_n,
           (unsigned long long)legal_n, (unsigned long long)bad_t, (unsigned long long)legal_t);
  }
  CHECK(hipFree(dx));
  CHECK(hipFree(dS));
  CHECK(hipFree(dout));
  return 0;
}
