// kernels.hip -- CDNA4 (gfx950) kernels of libbine_amd.so.
//
//  * k_reduce: the element-wise reduction that replaces MPI_Reduce_local at all
//    32 call sites of libbine's reduce family (e.g. libbine_allreduce.c:888):
//    out[i] = b[i] (op) a[i], out may alias b.  HBM-bound streaming kernel:
//    16 B per lane per access (global_load_dwordx4), U independent 16-B vectors
//    per lane in flight, one tile of 256 x U vectors per workgroup (no grid
//    cap below 16,384 workgroups, no grid-stride loop: measured faster on
//    MI355X, profiles/r1_explore.txt).  No LDS: every byte is touched once, so
//    staging through LDS would only add instructions.  Arithmetic follows
//    MPICH 3.3.2 exactly (inout (op) in, no FMA contraction, no denormal
//    flushing, integer wrap).
//  * k_copy: the device form of libbine's copy_buffer (libbine_utils.h:176-190,
//    e.g. the sbuf -> rbuf copy of allreduce_bine_bdw_remap at
//    libbine_allreduce.c:849-852 -- the whole P = 1 allreduce).  16-B vectors,
//    8 per lane in flight, non-temporal loads AND stores: 83 us for 256 MiB
//    (6.44 TB/s of read + write) vs 98.6 us for hipMemcpyAsync D2D
//    (tools/copy_variants.hip, profiles/r2_copy_variants.txt).  Copies of
//    128 MiB and more load their first 192 MiB with the default policy, so a
//    source copied again is partly found in the Infinity Cache: 79.4 us for
//    the same 256 MiB back to back (profiles/copy_mall_split.txt).
//  * k_fill_pico: pico_core's rand_r() input distributions
//    (pico_core_utils.c:902-923) generated in parallel by LCG jump-ahead,
//    bit-identical to the sequential host generator.
//  * k_checksum: order-independent 64-bit digest for size-independent parity
//    checks at full sizes; per-lane partial sums reduced with wave64 shuffles,
//    then through LDS, then one 64-bit atomic per workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <map>
#include <mutex>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "bine_internal.h"

// This file is compiled three times (Makefile): BINE_OPSET 0 -> kernels.o, the
// arithmetic ops SUM / PROD / MAX / MIN and every other kernel; BINE_OPSET 1
// -> kernels_logic.o, the reduction kernels' instantiations for the logical
// and bitwise ops only (launch_*_logic, reached from the opset-0 entry
// points); BINE_OPSET 2 -> kernels_h16.o, the reduction kernels'
// instantiations for the 16-bit floating types (launch_*_h16, reached the
// same way) and, for those types alone, the wide kernels k_widen / k_narrow /
// k_reduce_tree_wide (launch_*_h16, called directly: no other compilation
// holds a wide kernel), k_adamw_segs, the FP8 kernels k_amax_segs /
// k_fp8_scales / k_quant_segs and the MX kernel k_mx_segs, which need the same
// widen1 / narrow1.  Three translation units compile in parallel.
//
// Adding an element type: (1) a case in with_dtype, under the BINE_OPSET of
// the compilation that is to hold it -- every reduce-family entry point, the
// fill and the scale dispatch through that one list (with_op says which ops a
// type gets; kScaleT / kDmT whether the scaled kernels / the direct
// transport's in-launch reductions take it); (2) if another compilation than
// opset 0 holds it, owner_opset, so that the opset-0 entry points forward it.
// Outside this file: bine_op_valid / bine_dtype_size (executor.cpp).
#ifndef BINE_OPSET
#define BINE_OPSET 0
#endif
#if BINE_OPSET == 0
#define BINE_FN(name) name
#elif BINE_OPSET == 1
#define BINE_FN(name) name##_logic
#else
#define BINE_FN(name) name##_h16
#endif

namespace bine {

// ----------------------------------------------------------------------------
// element-wise reduction
// ----------------------------------------------------------------------------

template <typename T>
using uint_of = std::conditional_t<sizeof(T) == 1, uint8_t,
                std::conditional_t<sizeof(T) == 2, uint16_t,
                std::conditional_t<sizeof(T) == 4, uint32_t, uint64_t>>>;

// MPI's (value, index) pair types, C layout.  The padding of the C structs is
// spelled out as members, so that a pair passed and returned by value keeps
// the inout operand's padding bytes (implicit padding is unspecified after a
// copy -- measured: garbage in the padding of returned {double; int} pairs).
template <typename V>
struct Pair {
  V v;
  int i;
};
template <>
struct Pair<double> {
  double v;
  int i, pad_;
};
template <>
struct Pair<long> {
  long v;
  int i, pad_;
};
template <>
struct Pair<short> {
  short v, pad_;
  int i;
};
static_assert(sizeof(Pair<double>) == 16 && sizeof(Pair<long>) == 16 && sizeof(Pair<short>) == 8 &&
                  sizeof(Pair<float>) == 8 && sizeof(Pair<int>) == 8 && offsetof(Pair<short>, i) == 4,
              "MPI pair layouts");
template <typename T>
struct is_pair : std::false_type {};
template <typename V>
struct is_pair<Pair<V>> : std::true_type {};

// C99 complex {re; im} (MPI_C_FLOAT_COMPLEX / MPI_C_DOUBLE_COMPLEX)
template <typename V>
struct Cplx {
  V re, im;
};
template <typename T>
struct is_cplx : std::false_type {};
template <typename V>
struct is_cplx<Cplx<V>> : std::true_type {};

// The 16-bit floating types of the extension range (BINE_FLOAT16 /
// BINE_BFLOAT16, bine_amd.h): SUM / PROD / MAX / MIN only.  A sum or product
// is the IEEE result rounded once to the 16-bit format (nearest even,
// subnormals kept): binary16 by the native f16 instructions; bfloat16 widened
// to binary32 (a shift), one fp32 operation -- exact or far more precise than
// needed: 24 >= 2 * 8 + 2 bits, so the single rounding that follows gives the
// correctly rounded bfloat16 result -- and the hardware's round-to-nearest-
// even conversion back.  Every call rounds: the levels of a reduction tree
// never keep an fp32 intermediate, so the tree kernels give the bits of the
// literal schedule, which stores every intermediate as a 16-bit value.
// MAX / MIN compare and select (never v_pk_max / v_pk_min, whose NaN and
// signed-zero results differ from `io > in ? io : in`).
using F16 = _Float16;
using BF16 = __bf16;
static_assert(sizeof(F16) == 2 && sizeof(BF16) == 2, "16-bit floating types");

// MPICH's MPIR_OP_TYPE_REDUCE_CASE: a = inout, b = in, a = OP(a, b)
template <typename T, int OP>
__device__ __forceinline__ T apply(T io, T in) {
  if constexpr (std::is_same_v<T, BF16> && (OP == BINE_SUM || OP == BINE_PROD)) {
    const float x = (float)io, y = (float)in;
    return (BF16)(OP == BINE_SUM ? x + y : x * y);
  } else if constexpr (is_cplx<T>::value) {
    // MPICH's MPIR_LSUM / MPIR_LPROD on float/double _Complex: component-wise
    // sum; for finite operands the product is (a.re b.re - a.im b.im) +
    // (a.re b.im + a.im b.re) i (a = inout; no FMA: -ffp-contract=off)
    if constexpr (OP == BINE_SUM) {
      io.re = io.re + in.re;
      io.im = io.im + in.im;
    } else {
      static_assert(OP == BINE_PROD, "complex types: SUM / PROD only");
      const auto re = io.re * in.re - io.im * in.im;
      const auto im = io.re * in.im + io.im * in.re;
      io.re = re;
      io.im = im;
    }
    return io;
  } else if constexpr (OP == BINE_SUM) {
    if constexpr (std::is_integral_v<T>) return (T)((uint_of<T>)io + (uint_of<T>)in);
    else return io + in;
  } else if constexpr (OP == BINE_PROD) {
    if constexpr (std::is_integral_v<T>) return (T)((uint_of<T>)io * (uint_of<T>)in);
    else return io * in;
  } else if constexpr (OP == BINE_MAX) {
    return io > in ? io : in;
  } else if constexpr (OP == BINE_MIN) {
    return io < in ? io : in;
  } else if constexpr (OP == BINE_LAND) {  // MPIR_LLAND: C truthiness (-0.0 false, NaN true), 0 / 1
    return (T)(io != (T)0 && in != (T)0);
  } else if constexpr (OP == BINE_LOR) {
    return (T)(io != (T)0 || in != (T)0);
  } else if constexpr (OP == BINE_LXOR) {
    return (T)((io != (T)0) != (in != (T)0));
  } else if constexpr (OP == BINE_BAND) {
    return (T)(io & in);
  } else if constexpr (OP == BINE_BOR) {
    return (T)(io | in);
  } else if constexpr (OP == BINE_MAXLOC || OP == BINE_MINLOC) {
    // MPICH opmaxloc.c / opminloc.c (a = inout, b = in): equal values keep
    // the smaller index; otherwise a strictly larger (smaller) value of `in`
    // replaces the pair -- field by field, so io's padding bytes stay
    if (io.v == in.v) io.i = io.i < in.i ? io.i : in.i;
    else if (OP == BINE_MAXLOC ? io.v < in.v : io.v > in.v) {
      io.v = in.v;
      io.i = in.i;
    }
    return io;
  } else {
    static_assert(OP == BINE_BXOR, "unknown op");
    return (T)(io ^ in);
  }
}

// Which element types each op is instantiated for.  The bitwise ops act on
// bits alone, so every integer type runs them as bytes (canon_dtype below);
// the logical ops depend only on whether an element is zero, so signed
// integers run them as the unsigned type of their width.  The four
// arithmetic ops exist for every type.
template <typename T>
constexpr bool kLogicT = std::is_unsigned_v<T> || std::is_floating_point_v<T>;
template <typename T>
constexpr bool kBitsT = std::is_same_v<T, uint8_t>;
template <typename T>
constexpr bool kPairT = is_pair<T>::value;
template <typename T>
constexpr bool kCplxT = is_cplx<T>::value;

// ---- host dispatch: run-time (dtype, op, nl) -> template arguments ---------
// Each dispatcher calls a generic lambda with a tag whose type carries the
// compile-time value, only for the values this compilation instantiates.

template <typename T, int DT>
struct dtype_tag {
  using type = T;
  static constexpr int id = DT;
};
template <int V>
using int_c = std::integral_constant<int, V>;

static int status(hipError_t e) { return e == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP; }

// with_dtype(dtype, f): f(dtype_tag<T, dtype>{}), a BINE_* status, for the
// element type T of `dtype`; BINE_ERR_UNSUPPORTED for a dtype this
// compilation does not hold
template <typename F>
static int with_dtype(int dtype, F &&f) {
  switch (dtype) {
#if BINE_OPSET == 2
    case BINE_FLOAT16: return f(dtype_tag<F16, BINE_FLOAT16>{});
    case BINE_BFLOAT16: return f(dtype_tag<BF16, BINE_BFLOAT16>{});
#else
    case BINE_INT8: return f(dtype_tag<int8_t, BINE_INT8>{});
    case BINE_UINT8: return f(dtype_tag<uint8_t, BINE_UINT8>{});
    case BINE_INT16: return f(dtype_tag<int16_t, BINE_INT16>{});
    case BINE_UINT16: return f(dtype_tag<uint16_t, BINE_UINT16>{});
    case BINE_INT32: return f(dtype_tag<int32_t, BINE_INT32>{});
    case BINE_UINT32: return f(dtype_tag<uint32_t, BINE_UINT32>{});
    case BINE_INT64: return f(dtype_tag<int64_t, BINE_INT64>{});
    case BINE_UINT64: return f(dtype_tag<uint64_t, BINE_UINT64>{});
    case BINE_FLOAT: return f(dtype_tag<float, BINE_FLOAT>{});
    case BINE_DOUBLE: return f(dtype_tag<double, BINE_DOUBLE>{});
#endif
#if BINE_OPSET == 1
    case BINE_FLOAT_INT: return f(dtype_tag<Pair<float>, BINE_FLOAT_INT>{});
    case BINE_DOUBLE_INT: return f(dtype_tag<Pair<double>, BINE_DOUBLE_INT>{});
    case BINE_LONG_INT: return f(dtype_tag<Pair<long>, BINE_LONG_INT>{});
    case BINE_2INT: return f(dtype_tag<Pair<int>, BINE_2INT>{});
    case BINE_SHORT_INT: return f(dtype_tag<Pair<short>, BINE_SHORT_INT>{});
    case BINE_C_FLOAT_COMPLEX: return f(dtype_tag<Cplx<float>, BINE_C_FLOAT_COMPLEX>{});
    case BINE_C_DOUBLE_COMPLEX: return f(dtype_tag<Cplx<double>, BINE_C_DOUBLE_COMPLEX>{});
#endif
    default: return BINE_ERR_UNSUPPORTED;
  }
}

// with_op<T>(op, f, none): f(int_c<OP>{}) for the (T, OP) pairs this
// compilation instantiates; `none` for every other op
template <typename T, typename F, typename R = hipError_t>
static R with_op(int op, F &&f, R none = hipErrorInvalidValue) {
  switch (op) {
#if BINE_OPSET != 1
    case BINE_SUM: return f(int_c<BINE_SUM>{});
    case BINE_PROD: return f(int_c<BINE_PROD>{});
    case BINE_MAX: return f(int_c<BINE_MAX>{});
    case BINE_MIN: return f(int_c<BINE_MIN>{});
#else
    case BINE_SUM: if constexpr (kCplxT<T>) return f(int_c<BINE_SUM>{}); break;
    case BINE_PROD: if constexpr (kCplxT<T>) return f(int_c<BINE_PROD>{}); break;
    case BINE_LAND: if constexpr (kLogicT<T>) return f(int_c<BINE_LAND>{}); break;
    case BINE_LOR: if constexpr (kLogicT<T>) return f(int_c<BINE_LOR>{}); break;
    case BINE_LXOR: if constexpr (kLogicT<T>) return f(int_c<BINE_LXOR>{}); break;
    case BINE_BAND: if constexpr (kBitsT<T>) return f(int_c<BINE_BAND>{}); break;
    case BINE_BOR: if constexpr (kBitsT<T>) return f(int_c<BINE_BOR>{}); break;
    case BINE_BXOR: if constexpr (kBitsT<T>) return f(int_c<BINE_BXOR>{}); break;
    case BINE_MAXLOC: if constexpr (kPairT<T>) return f(int_c<BINE_MAXLOC>{}); break;
    case BINE_MINLOC: if constexpr (kPairT<T>) return f(int_c<BINE_MINLOC>{}); break;
#endif
    default: break;
  }
  return none;
}

// with_nl(nl, f, none): f(int_c<NL>{}) for the leaf counts the tree kernels
// are instantiated for
template <typename F, typename R = hipError_t>
static R with_nl(int nl, F &&f, R none = hipErrorInvalidValue) {
  switch (nl) {
    case 2: return f(int_c<2>{});
    case 4: return f(int_c<4>{});
    case 8: return f(int_c<8>{});
    case 16: return f(int_c<16>{});
    default: return none;
  }
}

#if BINE_OPSET == 0
// the (type, op) pairs the opset-1 compilation holds: the logical / bitwise /
// loc ops, and the pair and complex types
static bool ext_op(int dtype, int op) {
  return (op >= BINE_LAND && op < BINE_NUM_OPS) || (dtype >= BINE_FLOAT_INT && dtype < BINE_NUM_DTYPES);
}
// the types the opset-2 compilation holds (every op: the ones not defined on
// them are refused there, by canon_dtype)
static bool h16_dtype(int dtype) { return dtype == BINE_FLOAT16 || dtype == BINE_BFLOAT16; }
// the BINE_OPSET of the compilation that holds the kernels of (dtype, op);
// the entry points below forward to launch_*_h16 (2) / launch_*_logic (1)
static int owner_opset(int dtype, int op) { return h16_dtype(dtype) ? 2 : ext_op(dtype, op) ? 1 : 0; }
#endif

// the element type an op runs on (see kLogicT / kBitsT); *scale = elements
// of the run type per element of `dtype`; -1: the op is not defined on the
// type (bitwise ops on float / double: MPICH's MPI_ERR_OP; anything but the
// arithmetic four on float16 / bfloat16, which otherwise pass through)
static int canon_dtype(int dtype, int op, size_t *scale) {
  *scale = 1;
  if (!bine_op_valid(dtype, op)) return -1;
  if (op == BINE_BAND || op == BINE_BOR || op == BINE_BXOR) {
    *scale = bine_dtype_size(dtype);
    return BINE_UINT8;
  }
  if (op == BINE_LAND || op == BINE_LOR || op == BINE_LXOR) {
    switch (dtype) {
      case BINE_INT8: return BINE_UINT8;
      case BINE_INT16: return BINE_UINT16;
      case BINE_INT32: return BINE_UINT32;
      case BINE_INT64: return BINE_UINT64;
      default: return dtype;
    }
  }
  return dtype;
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <typename T, int OP>
__device__ __forceinline__ u32x4_t apply16(u32x4_t vb, u32x4_t va) {
  constexpr int N = 16 / (int)sizeof(T);
  if constexpr (std::is_same_v<T, F16> && (OP == BINE_SUM || OP == BINE_PROD)) {
    // 8 binary16 lanes: packed f16 add / mul (v_pk_add_f16 / v_pk_mul_f16)
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    f16x8 b, a;
    __builtin_memcpy(&b, &vb, 16);
    __builtin_memcpy(&a, &va, 16);
    b = OP == BINE_SUM ? b + a : b * a;
    u32x4_t r;
    __builtin_memcpy(&r, &b, 16);
    return r;
  } else if constexpr (std::is_same_v<T, BF16> && (OP == BINE_SUM || OP == BINE_PROD)) {
    // 8 bfloat16 lanes: the even elements (low halves) widened by a shift,
    // the odd ones by a mask, into two float4s; packed fp32 add / mul; one
    // round-to-nearest-even conversion per pair (v_cvt_pk_bf16_f32: element
    // 2k from the low-half result, 2k + 1 from the high-half result)
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    const u32x4_t blo = vb << 16, bhi = vb & 0xffff0000u, alo = va << 16, ahi = va & 0xffff0000u;
    f32x4 xl, xh, yl, yh;
    __builtin_memcpy(&xl, &blo, 16);
    __builtin_memcpy(&xh, &bhi, 16);
    __builtin_memcpy(&yl, &alo, 16);
    __builtin_memcpy(&yh, &ahi, 16);
    const f32x4 lo = OP == BINE_SUM ? xl + yl : xl * yl, hi = OP == BINE_SUM ? xh + yh : xh * yh;
    const bf16x8 h = __builtin_convertvector(__builtin_shufflevector(lo, hi, 0, 4, 1, 5, 2, 6, 3, 7), bf16x8);
    u32x4_t r;
    __builtin_memcpy(&r, &h, 16);
    return r;
  }
  T b[N], a[N];
  __builtin_memcpy(b, &vb, 16);
  __builtin_memcpy(a, &va, 16);
#pragma unroll
  for (int i = 0; i < N; i++) b[i] = apply<T, OP>(b[i], a[i]);
  u32x4_t r;
  __builtin_memcpy(&r, b, 16);
  return r;
}

constexpr int kBlock = 256;
using u32x4 = u32x4_t;  // one global_load/store_dwordx4 per lane

// launch geometry shared by the kernels below ----------------------------------
// Operands co-aligned mod 16 B: `head` elements of `esz` bytes up to the
// first 16-B boundary of `out` (at most n), then `nvec` whole 16-B vectors;
// the rest is the scalar tail.
struct VecSplit {
  size_t head, nvec;
};
static VecSplit vec_split(uintptr_t out, size_t n, size_t esz) {
  const size_t head = std::min<size_t>(((16 - (out & 15)) & 15) / esz, n);
  return {head, (n - head) / (16 / esz)};
}
// workgroups of a scalar grid-stride kernel over n elements: four elements
// per lane, at most 2048 workgroups
static unsigned scalar_blocks(size_t n) {
  return (unsigned)std::min<size_t>((n + kBlock * 4 - 1) / (kBlock * 4), 2048);
}

// Elements [0, head) and [head + 16/sizeof(T) * nvec, n) are done scalar by
// block 0; the 16-B aligned middle is vectorized.  NT is a cache-policy mask:
// bit 0 = non-temporal loads of `a` (the received operand, read exactly once),
// bit 1 = of `b`, bit 2 = non-temporal stores of `out`.
template <int NTBIT>
__device__ __forceinline__ u32x4 ld(const u32x4 *p) {
  if constexpr (NTBIT) return __builtin_nontemporal_load(p);
  else return *p;
}

template <typename T, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduce(const T *__restrict__ a, const T *b, T *out,
                                                   size_t head, size_t nvec, size_t n) {
  constexpr size_t V = 16 / sizeof(T);
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += kBlock) out[i] = apply<T, OP>(b[i], a[i]);
    for (size_t i = head + nvec * V + threadIdx.x; i < n; i += kBlock) out[i] = apply<T, OP>(b[i], a[i]);
  }
  const u32x4 *va = reinterpret_cast<const u32x4 *>(a + head);
  const u32x4 *vb = reinterpret_cast<const u32x4 *>(b + head);
  u32x4 *vo = reinterpret_cast<u32x4 *>(out + head);
  const size_t tile = (size_t)kBlock * U;
  const size_t stride = (size_t)gridDim.x * tile;
  size_t base = (size_t)blockIdx.x * tile + threadIdx.x;
  // full tiles: no bounds checks, U loads of each operand in flight per lane
  for (; base + (U - 1) * (size_t)kBlock < nvec; base += stride) {
    u32x4 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      x[u] = ld<NT & 1>(va + base + (size_t)u * kBlock);
      y[u] = ld<NT & 2>(vb + base + (size_t)u * kBlock);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const u32x4 r = apply16<T, OP>(y[u], x[u]);
      if constexpr (NT & 4) __builtin_nontemporal_store(r, vo + base + (size_t)u * kBlock);
      else vo[base + (size_t)u * kBlock] = r;
    }
  }
  // last partial tile
#pragma unroll
  for (int u = 0; u < U; u++) {
    const size_t i = base + (size_t)u * kBlock;
    if (i < nvec) vo[i] = apply16<T, OP>(vb[i], va[i]);
  }
}

// dispatch -----------------------------------------------------------------

// Defaults measured on MI355X (profiles/r1_explore.txt, C2 fp32 SUM 64 MiB):
// 4 vectors per lane, one tile per workgroup (no grid cap below 16384
// workgroups), non-temporal loads of the once-read operand.
constexpr int kDefaultUnroll = 4, kDefaultMaxBlocks = 16384, kDefaultNT = 1;
static int g_unroll = 0, g_maxblocks = 0, g_nt = kDefaultNT;

[[maybe_unused]] static void read_tuning() {
  if (g_unroll) return;
  const char *u = getenv("BINE_REDUCE_UNROLL");
  const char *m = getenv("BINE_REDUCE_MAXBLOCKS");
  const char *t = getenv("BINE_REDUCE_NT");
  int uu = u ? atoi(u) : 4;
  g_unroll = (uu == 1 || uu == 2 || uu == 4 || uu == 8) ? uu : 4;
  g_maxblocks = m ? atoi(m) : 0;
  g_nt = t ? atoi(t) : kDefaultNT;
}

template <typename T, int OP, int U, int NT>
static hipError_t run_reduce(const T *a, const T *b, T *out, size_t n, hipStream_t st) {
  const uintptr_t ao = (uintptr_t)a, bo = (uintptr_t)b, oo = (uintptr_t)out;
  // operands not co-aligned mod 16 B (small runs only, see reduce_t): all scalar
  const bool co = ((ao ^ oo) & 15) == 0 && ((bo ^ oo) & 15) == 0 && (oo % sizeof(T)) == 0;
  const auto [head, nvec] = co ? vec_split(oo, n, sizeof(T)) : VecSplit{n, 0};
  int blocks;
  if (nvec == 0) blocks = 1;
  else {
    const size_t tiles = (nvec + (size_t)kBlock * U - 1) / ((size_t)kBlock * U);
    const int maxb = g_maxblocks > 0 ? g_maxblocks : kDefaultMaxBlocks;
    blocks = (int)(tiles < (size_t)maxb ? tiles : (size_t)maxb);
  }
  hipLaunchKernelGGL((k_reduce<T, OP, U, NT>), dim3(blocks), dim3(kBlock), 0, st, a, b, out, head, nvec, n);
  return hipGetLastError();
}

// scalar grid-stride kernel for operands that are not co-aligned mod 16 bytes
template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void k_reduce_scalar(const T *__restrict__ a, const T *b, T *out,
                                                          size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    out[i] = apply<T, OP>(b[i], a[i]);
}

template <typename T, int OP>
static hipError_t reduce_t(const void *a, const void *b, void *out, size_t n, hipStream_t st) {
  const T *pa = (const T *)a, *pb = (const T *)b;
  T *po = (T *)out;
  const uintptr_t ao = (uintptr_t)a, bo = (uintptr_t)b, oo = (uintptr_t)out;
  if ((((ao ^ oo) & 15) != 0 || ((bo ^ oo) & 15) != 0) && n > 4096) {
    hipLaunchKernelGGL((k_reduce_scalar<T, OP>), dim3(scalar_blocks(n)), dim3(kBlock), 0, st, pa, pb, po, n);
    return hipGetLastError();
  }
  if constexpr (std::is_same_v<T, float> && OP == BINE_SUM) {
    // tuning variants (bine_set_reduce_tuning / BINE_REDUCE_*) for the headline dtype
#define NTSW(U)                                                               \
    switch (g_nt) {                                                           \
      case 0: return run_reduce<T, OP, U, 0>(pa, pb, po, n, st);              \
      case 2: return run_reduce<T, OP, U, 2>(pa, pb, po, n, st);              \
      case 3: return run_reduce<T, OP, U, 3>(pa, pb, po, n, st);              \
      case 4: return run_reduce<T, OP, U, 4>(pa, pb, po, n, st);              \
      case 5: return run_reduce<T, OP, U, 5>(pa, pb, po, n, st);              \
      case 7: return run_reduce<T, OP, U, 7>(pa, pb, po, n, st);              \
      default: return run_reduce<T, OP, U, 1>(pa, pb, po, n, st);             \
    }
    switch (g_unroll) {
      case 1: NTSW(1)
      case 2: NTSW(2)
      case 8: NTSW(8)
      default: NTSW(4)
    }
#undef NTSW
  }
  return run_reduce<T, OP, kDefaultUnroll, kDefaultNT>(pa, pb, po, n, st);
}

int BINE_FN(launch_reduce)(const void *a, const void *b, void *out, size_t count, int dtype, int op, void *stream) {
  if (count == 0) return BINE_SUCCESS;
#if BINE_OPSET == 0
  if (const int o = owner_opset(dtype, op))
    return o == 2 ? launch_reduce_h16(a, b, out, count, dtype, op, stream)
                  : launch_reduce_logic(a, b, out, count, dtype, op, stream);
#endif
  size_t scale;
  dtype = canon_dtype(dtype, op, &scale);
  if (dtype < 0) return BINE_ERR_ARG;
  count *= scale;
  read_tuning();
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return status(with_op<T>(op, [&](auto opc) { return reduce_t<T, decltype(opc)::value>(a, b, out, count, st); }));
  });
}

// ----------------------------------------------------------------------------
// The segment family's dispatch (k_copy_segs, k_copy_shards, k_sumsq_segs,
// k_scale_segs, k_adamw_segs), stated once.  A launch takes up to N descriptors
// BY VALUE in its kernel arguments: no device table to upload, nothing a later
// call could overwrite while this launch still reads it.  Its grid is the
// concatenation of the segments' tiles (tile0[k] = slot k's first tile,
// tile0[nseg] = their number; a tile is kCopyTileVecs 16-B vectors, at least
// one per segment).  A workgroup finds its slot by a binary search over that
// prefix (log2 N steps of scalar loads: every value is workgroup-uniform),
// splits the segment with the planners' own seg_head / seg_nvec into head
// bytes, 16-B ALIGNED vectors and tail bytes, and runs the kernel's body on its
// tile; a segment's first workgroup also takes head and tail.  A member is an
// argument struct {TileTable tab; ...; D s[N]} within 4 KiB, a body, and a
// planner (segments.cpp) whose LaunchTables fill_segs turns into launches.
template <int N>
struct TileTable {
  uint32_t nseg;
  uint32_t tile0[N + 1];
  struct Slot {
    uint32_t k, wt;
  };
  // tile t's slot k and its place wt among the slot's tiles: tile0[k] <= t < tile0[k + 1], nseg >= 1
  __device__ __forceinline__ Slot find(uint32_t t) const {
    uint32_t k = 0, hi = nseg;
    while (hi - k > 1) {
      const uint32_t mid = (k + hi) >> 1;
      if (t >= tile0[mid]) k = mid;
      else hi = mid;
    }
    return {k, t - tile0[k]};
  }
};

// The host side: tile0 (unused entries = the number of tiles) and slot[s] =
// desc(s) for the launch's slots, a value-initialised descriptor for the others
template <int N, typename D, typename F>
static void fill_slots(const LaunchTable<N> &L, uint32_t (&tile0)[N + 1], D (&slot)[N], F &&desc) {
  for (int s = 0; s <= N; s++) tile0[s] = L.tile0[s < L.nseg ? s : L.nseg];
  for (int s = 0; s < N; s++) slot[s] = s < L.nseg ? desc(s) : D{};
}
template <typename A, int N, typename F>
static void fill_segs(A &a, const LaunchTable<N> &L, F &&desc) {
  a.tab.nseg = (uint32_t)L.nseg;
  fill_slots(L, a.tab.tile0, a.s, desc);
}

#if BINE_OPSET == 0
// ----------------------------------------------------------------------------
// device copy (copy_buffer): one tile of kBlock * kCopyU 16-B vectors per
// workgroup, loads issued before stores, both non-temporal (the copied bytes
// are not re-read by this launch).  Bytes before the first 16-B boundary of
// `dst` and after the last full vector go byte-wise through workgroup 0.
//
// Cache policy: the tiles whose first vector lies below `keep_vecs` load with
// the default policy, so a large copy's first bytes may stay in the 256 MiB
// Infinity Cache for the next copy of the same source; everything else is
// non-temporal as before.  keep_vecs = 0 is the kernel as it was.  The choice
// depends on blockIdx alone: one branch ahead of the eight loads.
constexpr int kCopyU = 8;
// The bytes of a large copy's source that are loaded with the default policy,
// and the smallest copy that gets them.  Measured on one MI355X
// (tools/copy_variants.hip mall, profiles/copy_mall_split.txt; medians of three
// sweeps): a 256 MiB source copied back to back takes 84.88 us
// with every load non-temporal (spread of the three medians 0.20 us) and
// 85.40 / 88.52 / 86.48 / 84.20 / 81.28 / 79.44 us with the first 32 / 64 / 96 /
// 128 / 160 / 192 MiB kept: 192 MiB is 6.4 % faster, less than 128 MiB gains
// nothing.  With the source rewritten before every copy all of them take 79.1 -
// 79.8 us (no loss); a 128 MiB copy gains 7.3 %, a 64 MiB one 8.7 %.  Copies
// below 128 MiB keep today's loads all the same: they would load everything
// with the default policy, which costs 6 % where the source is not found in
// the cache (profiles/r2_copy_variants.txt), and that case was not measured.
constexpr uint64_t kCopyKeepBytes = 192ull << 20;
constexpr uint64_t kCopyKeepMinBytes = 128ull << 20;

template <bool KEEP>
__device__ __forceinline__ void copy_tile(const u32x4 *vs, u32x4 *vd, size_t base) {
  u32x4 x[kCopyU];
#pragma unroll
  for (int u = 0; u < kCopyU; u++)
    x[u] = KEEP ? vs[base + (size_t)u * kBlock] : __builtin_nontemporal_load(vs + base + (size_t)u * kBlock);
#pragma unroll
  for (int u = 0; u < kCopyU; u++) __builtin_nontemporal_store(x[u], vd + base + (size_t)u * kBlock);
}

__global__ __launch_bounds__(kBlock) void k_copy(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                 size_t head, size_t nvec, size_t n, size_t keep_vecs) {
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += kBlock) dst[i] = src[i];
    for (size_t i = head + nvec * 16 + threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
  }
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(src + head);
  u32x4 *vd = reinterpret_cast<u32x4 *>(dst + head);
  const size_t tile0 = (size_t)blockIdx.x * kBlock * kCopyU, base = tile0 + threadIdx.x;
  if (base + (kCopyU - 1) * (size_t)kBlock < nvec) {
    if (tile0 < keep_vecs) {
      // The whole tile on either side, this side between two empty asm
      // statements (no operands, no code).  Without them the compiler merges
      // the two sides' loads, identical but for the hint, into one set without
      // it; with the stores shared behind the branch it reorders the loads and
      // holds the first store back until seven of them have landed, 9 % slower.
      asm volatile("");
      copy_tile<true>(vs, vd, base);
      asm volatile("");
    } else {
      copy_tile<false>(vs, vd, base);
    }
  } else {
#pragma unroll
    for (int u = 0; u < kCopyU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) vd[i] = vs[i];
    }
  }
}

int launch_copy(void *dst, const void *src, size_t bytes, void *stream) {
  if (bytes == 0 || dst == src) return BINE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const uintptr_t so = (uintptr_t)src, dO = (uintptr_t)dst;
  if ((so ^ dO) & 15) {
    // not co-aligned mod 16 B (never the case for the plans' element offsets of
    // 16-B aligned buffers): the runtime's device copy
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP;
  }
  const auto [head, nvec] = vec_split(dO, bytes, 1);
  const size_t tiles = (nvec + (size_t)kBlock * kCopyU - 1) / ((size_t)kBlock * kCopyU);
  const unsigned blocks = (unsigned)(tiles ? tiles : 1);
  // BINE_COPY_KEEP_MIB in the environment, read once
  static const CopyKeep keep = copy_keep_policy(getenv("BINE_COPY_KEEP_MIB"), kCopyKeepBytes, kCopyKeepMinBytes);
  hipLaunchKernelGGL(k_copy, dim3(blocks), dim3(kBlock), 0, st, (const uint8_t *)src, (uint8_t *)dst, head, nvec,
                     bytes, (size_t)copy_keep_vecs(bytes, nvec, keep));
  return hipGetLastError() == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP;
}

// ----------------------------------------------------------------------------
// segmented copy (bine_copy_segments): up to kSegsPerLaunch independent copies
// in one launch (TileTable's dispatch); a workgroup is k_copy on its segment.
// Where the source is not co-aligned with the destination mod 16 B the
// workgroup loads the two 16-B ALIGNED source vectors that hold a destination vector's bytes and shifts them together in
// registers: no unaligned vector access is issued, the stores stay 16-B
// aligned, and the extra bytes read lie in 16-B lines that also hold bytes of
// the segment, so never in another page.
static_assert(kCopyTileVecs == (uint64_t)kBlock * kCopyU, "the planner's tile is k_copy's");

struct CopySeg {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t bytes;
};
struct CopySegs {
  TileTable<kSegsPerLaunch> tab;
  CopySeg s[kSegsPerLaunch];
};
static_assert(sizeof(CopySegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

// bytes [sh, sh + 16) of the 32 bytes lo : hi, 0 < sh < 16; W = sh / 4
template <int W>
__device__ __forceinline__ u32x4 shift_join(u32x4 lo, u32x4 hi, unsigned bits) {
  const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  u32x4 r;
  r.x = (uint32_t)((((uint64_t)c[W + 1] << 32) | c[W]) >> bits);
  r.y = (uint32_t)((((uint64_t)c[W + 2] << 32) | c[W + 1]) >> bits);
  r.z = (uint32_t)((((uint64_t)c[W + 3] << 32) | c[W + 2]) >> bits);
  r.w = (uint32_t)((((uint64_t)c[W + 4] << 32) | c[W + 3]) >> bits);
  return r;
}

constexpr int kCopyShiftU = 4;  // destination vectors per lane in flight on the shifted path

template <int W>
__device__ __forceinline__ void copy_shifted(const u32x4 *va, u32x4 *vd, size_t base, size_t nvec, unsigned bits) {
#pragma unroll 1  // keeps the kernel at k_copy's occupancy: the co-aligned path is the fast one
  for (int u0 = 0; u0 < kCopyU; u0 += kCopyShiftU) {
    u32x4 lo[kCopyShiftU], hi[kCopyShiftU];
#pragma unroll
    for (int u = 0; u < kCopyShiftU; u++) {
      const size_t i = base + (size_t)(u0 + u) * kBlock;
      if (i < nvec) {
        lo[u] = __builtin_nontemporal_load(va + i);
        hi[u] = __builtin_nontemporal_load(va + i + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < kCopyShiftU; u++) {
      const size_t i = base + (size_t)(u0 + u) * kBlock;
      if (i < nvec) __builtin_nontemporal_store(shift_join<W>(lo[u], hi[u], bits), vd + i);
    }
  }
}

// tile `wt` of the copy dst[0:n) = src[0:n): k_copy where the two are co-aligned
// mod 16 B, the aligned-load-and-shift path otherwise; tile 0 also copies the
// head / tail bytes.  A tile past the range's last vector writes nothing.
__device__ __forceinline__ void copy_range(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, size_t n,
                                           uint32_t wt) {
  const size_t head = seg_head((uintptr_t)dst, n), nvec = seg_nvec(n, head);
  if (wt == 0) {  // head and tail of this range
    for (size_t i = threadIdx.x; i < head; i += kBlock) dst[i] = src[i];
    for (size_t i = head + nvec * 16 + threadIdx.x; i < n; i += kBlock) dst[i] = src[i];
  }
  u32x4 *vd = reinterpret_cast<u32x4 *>(dst + head);
  const size_t base = (size_t)wt * kBlock * kCopyU + threadIdx.x;
  const unsigned sh = (unsigned)((uintptr_t)(src + head) & 15);
  if (sh == 0) {  // co-aligned: k_copy
    const u32x4 *vs = reinterpret_cast<const u32x4 *>(src + head);
    if (base + (kCopyU - 1) * (size_t)kBlock < nvec) {
      u32x4 x[kCopyU];
#pragma unroll
      for (int u = 0; u < kCopyU; u++) x[u] = __builtin_nontemporal_load(vs + base + (size_t)u * kBlock);
#pragma unroll
      for (int u = 0; u < kCopyU; u++) __builtin_nontemporal_store(x[u], vd + base + (size_t)u * kBlock);
    } else {
#pragma unroll
      for (int u = 0; u < kCopyU; u++) {
        const size_t i = base + (size_t)u * kBlock;
        if (i < nvec) vd[i] = vs[i];
      }
    }
    return;
  }
  if (nvec == 0) return;  // nothing but head / tail bytes: no vector of the source is touched
  // destination vector i = bytes [sh, sh + 16) of the aligned source vectors i, i + 1
  const u32x4 *va = reinterpret_cast<const u32x4 *>(src + head - sh);
  const unsigned bits = 8 * (sh & 3);
  switch (sh >> 2) {
    case 0: copy_shifted<0>(va, vd, base, nvec, bits); break;
    case 1: copy_shifted<1>(va, vd, base, nvec, bits); break;
    case 2: copy_shifted<2>(va, vd, base, nvec, bits); break;
    default: copy_shifted<3>(va, vd, base, nvec, bits); break;
  }
}

__global__ __launch_bounds__(kBlock) void k_copy_segs(CopySegs a) {
  const auto [k, wt] = a.tab.find(blockIdx.x);
  copy_range(a.s[k].src, a.s[k].dst, a.s[k].bytes, wt);
}

int launch_copy_segments(int n, void *const *dsts, const void *const *srcs, const size_t *bytes, void *stream) {
  std::vector<uint64_t> addr;
  if (const int rc = seg_list_addrs(n, bytes, {dsts, srcs}, addr)) return rc;
  std::vector<SegLaunch> ls;
  if (const int rc = plan_seg_launches(n, addr.data(), addr.data() + n, bytes, ls)) return rc;
  hipStream_t st = (hipStream_t)stream;
  for (const SegLaunch &L : ls) {
    CopySegs a;
    fill_segs(a, L, [&](int s) {
      const int k = L.seg[s];
      return CopySeg{(const uint8_t *)srcs[k], (uint8_t *)dsts[k], (uint64_t)bytes[k]};
    });
    hipLaunchKernelGGL(k_copy_segs, dim3(L.tile0[L.nseg]), dim3(kBlock), 0, st, a);
    if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
  }
  return BINE_SUCCESS;
}

// ----------------------------------------------------------------------------
// sharded copy (bine_copy_shards): all P shards of up to kSegsPerLaunch tensors
// in one launch, between the flat layout (shard j of tensor k at flat[k] +
// j * bytes[k]) and the packed one (packed + j * block + poff[k]) -- the
// strided layout change of a sharded bucket, one descriptor per TENSOR
// (TileTable's dispatch over the tiles of ONE shard).  With T = the tensors'
// tiles per shard summed, the grid is P x T workgroups, shard major: one
// division of workgroup-uniform values gives a workgroup its shard (t / T) and
// its place among one shard's tiles (t % T), the table's search its tensor and
// its tile, and then it is k_copy_segs on that shard's (source, destination,
// bytes): copy_range.  Neighbouring workgroups so copy
// neighbouring tiles, as they do in k_copy_segs (tile major and shard minor --
// P streams 4 MiB apart -- measured 6 % slower on 8 x 8 x 4 MiB).  The
// destination's phase may differ from shard to shard, so a tensor's tiles per
// shard is what the shard with the most vectors needs (plan_shard_launches); a
// workgroup whose tile lies past its own shard's last vector writes nothing.
struct CopyShard {
  uint8_t *flat;
  uint64_t poff;   // the shards' offset in a packed block
  uint64_t bytes;  // of one shard
};
struct CopyShards {
  TileTable<kSegsPerLaunch> tab;  // of one shard's tiles: tile0[nseg] = T
  uint32_t nranks, dir;           // dir 0: flat -> packed, 1: packed -> flat
  uint8_t *packed;
  uint64_t block;  // bytes of a packed block: the sum of every tensor's shard bytes
  CopyShard s[kSegsPerLaunch];
};
static_assert(sizeof(CopyShards) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

__global__ __launch_bounds__(kBlock) void k_copy_shards(CopyShards a) {
  const uint32_t T = a.tab.tile0[a.tab.nseg], j = blockIdx.x / T;
  const auto [k, wt] = a.tab.find(blockIdx.x - j * T);
  const size_t n = a.s[k].bytes;
  uint8_t *fl = a.s[k].flat + (size_t)j * n;
  uint8_t *pk = a.packed + (size_t)j * a.block + a.s[k].poff;
  copy_range(a.dir ? pk : fl, a.dir ? fl : pk, n, wt);
}

int launch_copy_shards(int n, int nranks, int dir, void *packed, void *const *flat, const size_t *bytes,
                       void *stream) {
  std::vector<uint64_t> addr;
  if (const int rc = seg_list_addrs(n, bytes, {flat}, addr)) return rc;
  std::vector<ShardLaunch> ls;
  uint64_t block = 0;
  if (const int rc =
          plan_shard_launches(n, nranks, dir, (uint64_t)(uintptr_t)packed, addr.data(), bytes, ls, &block))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  for (const ShardLaunch &L : ls) {
    CopyShards a;
    a.nranks = (uint32_t)nranks, a.dir = (uint32_t)dir;
    a.packed = (uint8_t *)packed, a.block = block;
    fill_segs(a, L, [&](int s) { return CopyShard{(uint8_t *)flat[L.seg[s]], L.poff[s], (uint64_t)bytes[L.seg[s]]}; });
    hipLaunchKernelGGL(k_copy_shards, dim3(L.tile0[L.nseg] * (uint32_t)nranks), dim3(kBlock), 0, st, a);
    if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
  }
  return BINE_SUCCESS;
}

#endif  // BINE_OPSET == 0

// ----------------------------------------------------------------------------
// batched reduction: up to kMaxBatch independent windows in one launch (the
// P-1 per-instance chunk reductions of a multi-tree round).  The grid is the
// concatenation of every window's tiles; a workgroup finds its window by a
// scan over at most 8 tile offsets.  Windows must be co-aligned mod 16 B
// (the caller falls back to one launch per window otherwise).

struct BatchWin {
  const void *a, *b;
  void *out;
  uint64_t head, nvec, n, tile0;
};
struct Batch {
  int nwin;
  BatchWin w[kMaxBatch];
};

template <typename T, int OP, int U, int NT>
__global__ __launch_bounds__(kBlock) void k_reduce_batch(Batch bt) {
  constexpr size_t V = 16 / sizeof(T);
  const uint64_t t = blockIdx.x;
  int k = 0;
  while (k + 1 < bt.nwin && t >= bt.w[k + 1].tile0) k++;
  const BatchWin &w = bt.w[k];
  const T *a = (const T *)w.a, *b = (const T *)w.b;
  T *out = (T *)w.out;
  if (t == w.tile0) {  // head and tail of this window
    for (size_t i = threadIdx.x; i < w.head; i += kBlock) out[i] = apply<T, OP>(b[i], a[i]);
    for (size_t i = w.head + w.nvec * V + threadIdx.x; i < w.n; i += kBlock) out[i] = apply<T, OP>(b[i], a[i]);
  }
  const u32x4 *va = reinterpret_cast<const u32x4 *>(a + w.head);
  const u32x4 *vb = reinterpret_cast<const u32x4 *>(b + w.head);
  u32x4 *vo = reinterpret_cast<u32x4 *>(out + w.head);
  const size_t base = (size_t)(t - w.tile0) * kBlock * U + threadIdx.x;
  if (base + (U - 1) * (size_t)kBlock < w.nvec) {
    u32x4 x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      x[u] = ld<NT & 1>(va + base + (size_t)u * kBlock);
      y[u] = ld<NT & 2>(vb + base + (size_t)u * kBlock);
    }
#pragma unroll
    for (int u = 0; u < U; u++) vo[base + (size_t)u * kBlock] = apply16<T, OP>(y[u], x[u]);
  } else {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < w.nvec) vo[i] = apply16<T, OP>(vb[i], va[i]);
    }
  }
}

template <typename T, int OP>
static hipError_t batch_t(int n, const void *const *a, const void *const *b, void *const *out,
                          const size_t *count, hipStream_t st) {
  constexpr int U = kDefaultUnroll;
  Batch bt;
  bt.nwin = n;
  uint64_t tiles = 0;
  for (int k = 0; k < n; k++) {
    const uintptr_t ao = (uintptr_t)a[k], bo = (uintptr_t)b[k], oo = (uintptr_t)out[k];
    if (((ao ^ oo) & 15) || ((bo ^ oo) & 15) || (oo % sizeof(T))) return hipErrorInvalidValue;
    BatchWin &w = bt.w[k];
    w.a = a[k];
    w.b = b[k];
    w.out = out[k];
    w.n = count[k];
    const VecSplit vs = vec_split(oo, count[k], sizeof(T));
    w.head = vs.head;
    w.nvec = vs.nvec;
    w.tile0 = tiles;
    tiles += std::max<uint64_t>(1, (w.nvec + (uint64_t)kBlock * U - 1) / ((uint64_t)kBlock * U));
  }
  hipLaunchKernelGGL((k_reduce_batch<T, OP, U, kDefaultNT>), dim3((unsigned)tiles), dim3(kBlock), 0, st, bt);
  return hipGetLastError();
}

int BINE_FN(launch_reduce_batch)(int n, const void *const *a, const void *const *b, void *const *out,
                                 const size_t *count_in, int dtype, int op, void *stream) {
  if (n < 1 || n > kMaxBatch) return BINE_ERR_ARG;
#if BINE_OPSET == 0
  if (const int o = owner_opset(dtype, op))
    return o == 2 ? launch_reduce_batch_h16(n, a, b, out, count_in, dtype, op, stream)
                  : launch_reduce_batch_logic(n, a, b, out, count_in, dtype, op, stream);
#endif
  size_t scale;
  dtype = canon_dtype(dtype, op, &scale);
  if (dtype < 0) return BINE_ERR_ARG;
  size_t count[kMaxBatch];
  for (int k = 0; k < n; k++) count[k] = count_in[k] * scale;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    const hipError_t e =
        with_op<T>(op, [&](auto opc) { return batch_t<T, decltype(opc)::value>(n, a, b, out, count, st); });
    if (e == hipErrorInvalidValue) return BINE_ERR_ARG;  // not co-aligned: caller falls back
    return status(e);
  });
}

// system-coherent 16-B accesses of the direct transport (protocol notes at
// k_dm_move below); here because the tree body uses them too
// A 16-B store written through to memory (system coherent: sc0 sc1, and
// non-temporal) -- the stores into a peer's inbox slot.  Through a buffer
// resource (the compiler schedules it and tracks its counters; raw stride-0
// addressing, 2 GiB range, gfx9 untyped dword3 0x00020000) with the cache
// policy sc0 | sc1 | nt = 1 | 16 | 2; `base` is wave-uniform.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(void *base) {
  // the base is the same in every lane; readfirstlane says so to the compiler
  // (otherwise it wraps each store in a waterfall loop)
  const uint64_t b = (uint64_t)(uintptr_t)base;
  const uint64_t u = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32 |
                     (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)u, (short)0, 0x7fffffff, 0x00020000);
}
__device__ __forceinline__ void st_wt(__amdgpu_buffer_rsrc_t r, uint64_t vec, u32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)(vec * 16), 0, 19);
}
__device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ----------------------------------------------------------------------------
// tree reduction: the owner's side of the flat reduce-scatter phase.  One
// launch evaluates the reference's whole reduction tree of a block from its P
// contributions (leaf 0 = the rank's own input, leaves 1..P-1 = the received
// blocks in tree order): HBM traffic (P + 1) * count * sizeof(T) instead of the
// 3 (P - 1) * count * sizeof(T) of P - 1 pairwise passes.  Per lane U 16-B
// vectors of every leaf in flight (NL * U loads), the tree evaluated in
// registers level by level -- v[i] = v[i] (op) v[i + w], left = inout -- so
// every element sees the reference's association and operand order.  Received
// leaves are read once: non-temporal loads.

// ----------------------------------------------------------------------------
// S(x), the scaled collectives' one multiplication (bine_amd.h): float and
// double multiply in their own format by (float)scale resp. scale; the 16-bit
// types are widened exactly to binary32, multiplied there by (float)scale and
// rounded to nearest even into the 16-bit format -- two roundings, by
// definition.  mul_of<T> is the multiplier's type (converted on the host).
template <typename T>
using mul_of = std::conditional_t<std::is_same_v<T, double>, double, float>;
template <typename T>
constexpr bool kScaleT =
    std::is_same_v<T, float> || std::is_same_v<T, double> || std::is_same_v<T, F16> || std::is_same_v<T, BF16>;

template <typename T>
__device__ __forceinline__ T scale1(T x, mul_of<T> m) {
  if constexpr (std::is_same_v<T, F16> || std::is_same_v<T, BF16>) {
    // The binary32 product must exist as such before it is converted: left to
    // itself the compiler folds widen + multiply + convert into one
    // v_fma_mixlo_f16 (m * x + 0), and the +0 addend turns a product of -0
    // into +0 (measured on the special-value grid: -0 * 0 gave +0).  The empty
    // asm pins the product in a VGPR (no instruction is emitted), so the
    // sequence is v_cvt_f32_f16, v_mul_f32, v_cvt_f16_f32.
    float p = (float)x * m;
    asm volatile("" : "+v"(p));
    return (T)p;
  } else return x * m;
}
// one 16-B vector.  binary16: v_cvt_f32_f16 up, packed fp32 multiply,
// v_cvt_f16_f32 (round to nearest even -- never the packed round-toward-zero
// conversion) down; bfloat16: widened by shift / mask as in apply16, packed
// fp32 multiply, the hardware's nearest-even v_cvt_pk_bf16_f32 down.
template <typename T>
__device__ __forceinline__ u32x4_t scale16(u32x4_t v, mul_of<T> m) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  if constexpr (std::is_same_v<T, F16>) {
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    typedef float f32x8 __attribute__((ext_vector_type(8)));
    f16x8 h;
    __builtin_memcpy(&h, &v, 16);
    h = __builtin_convertvector(__builtin_convertvector(h, f32x8) * m, f16x8);
    u32x4_t r;
    __builtin_memcpy(&r, &h, 16);
    return r;
  } else if constexpr (std::is_same_v<T, BF16>) {
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    const u32x4_t vlo = v << 16, vhi = v & 0xffff0000u;
    f32x4 lo, hi;
    __builtin_memcpy(&lo, &vlo, 16);
    __builtin_memcpy(&hi, &vhi, 16);
    lo = lo * m;
    hi = hi * m;
    const bf16x8 h = __builtin_convertvector(__builtin_shufflevector(lo, hi, 0, 4, 1, 5, 2, 6, 3, 7), bf16x8);
    u32x4_t r;
    __builtin_memcpy(&r, &h, 16);
    return r;
  } else if constexpr (std::is_same_v<T, double>) {
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    f64x2 d;
    __builtin_memcpy(&d, &v, 16);
    d = d * m;
    u32x4_t r;
    __builtin_memcpy(&r, &d, 16);
    return r;
  } else {
    static_assert(std::is_same_v<T, float>, "scaled types: float, double, float16, bfloat16");
    f32x4 f;
    __builtin_memcpy(&f, &v, 16);
    f = f * m;
    u32x4_t r;
    __builtin_memcpy(&r, &f, 16);
    return r;
  }
}

struct TreeArgs {
  const void *leaf[kMaxLeaves];
  void *out;
  uint64_t head, nvec, n;
  int vec;        // 1: all operands co-aligned mod 16 B with `out`
  unsigned swap;  // bit l: level l combines v[i + w] (op) v[i] (the right side is inout)
};

// one level's combine; `sw` is wave-uniform (a scalar branch)
template <typename T, int OP>
__device__ __forceinline__ T comb(T l, T r, bool sw) { return sw ? apply<T, OP>(r, l) : apply<T, OP>(l, r); }
template <typename T, int OP>
__device__ __forceinline__ u32x4 comb16(u32x4 l, u32x4 r, bool sw) {
  return sw ? apply16<T, OP>(r, l) : apply16<T, OP>(l, r);
}

template <typename T, int OP, int NL>
__device__ __forceinline__ T tree_scalar(const TreeArgs &t, size_t i) {
  T v[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) v[j] = ((const T *)t.leaf[j])[i];
  int lvl = 0;
#pragma unroll
  for (int w = 1; w < NL; w <<= 1, lvl++)
#pragma unroll
    for (int j = 0; j < NL; j += 2 * w) v[j] = comb<T, OP>(v[j], v[j + w], (t.swap >> lvl) & 1);
  return v[0];
}

// Leaves are loaded and reduced in groups of G = min(NL, 8): positions
// [8g, 8g + 8) form a complete subtree of the reference's tree (levels w = 1,
// 2, 4), and the group results combine by the upper levels (w = 8) exactly
// as the leaves would.  U vectors of each leaf per lane in flight (tree_nl).  One tile of kBlock * U vectors per workgroup, no
// grid-stride loop, unguarded loads in every full tile (measured on MI355X,
// tools/tree_variants.hip: a grid-strided form with a guard on every load ran
// 31 us vs 24.5 us for 8 x 16 MiB).
// SC (the scaled tree, bine_reduce_tree_scaled): the final value of every
// vector is multiplied by `m` in registers right before its store (scale16
// below) -- a separate instantiation; with SC = false the body is the one the
// unscaled kernels and the direct transport's k_dm_move_tree always had.
template <typename T, int OP, int NL, int U, bool GUARD, bool SC = false>
__device__ __forceinline__ void tree_tile(const u32x4 *const *lp, u32x4 *vo, size_t base, size_t nvec,
                                          unsigned swap, mul_of<T> m = {}) {
  constexpr int G = NL < 8 ? NL : 8, NG = NL / G, LG = G == 2 ? 1 : G == 4 ? 2 : 3;
  u32x4 part[U][NG];
#pragma unroll
  for (int g = 0; g < NG; g++) {
    u32x4 v[U][G];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (!GUARD || i < nvec) {
        // tree position 0: plain load; positions 1..NL-1: non-temporal.  The
        // rank's own leaf sits at position `pos` of the primitive, which is 0
        // only on some ranks, so this is "one plain + NL-1 non-temporal
        // streams", not "own leaf cached": at the C3 chunk (16 MiB per leaf)
        // no leaf is L2-resident anyway, and the mix measured fastest
        // (tools/tree_variants.hip).  Two separate statements: a select
        // between the two loads of one address is folded into one plain load.
        if (g == 0) v[u][0] = lp[0][i];
#pragma unroll
        for (int j = g == 0 ? 1 : 0; j < G; j++) v[u][j] = __builtin_nontemporal_load(lp[g * G + j] + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      int lvl = 0;
#pragma unroll
      for (int w = 1; w < G; w <<= 1, lvl++)
#pragma unroll
        for (int j = 0; j < G; j += 2 * w) v[u][j] = comb16<T, OP>(v[u][j], v[u][j + w], (swap >> lvl) & 1);
      part[u][g] = v[u][0];
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    int lvl = LG;
#pragma unroll
    for (int w = 1; w < NG; w <<= 1, lvl++)
#pragma unroll
      for (int g = 0; g < NG; g += 2 * w) part[u][g] = comb16<T, OP>(part[u][g], part[u][g + w], (swap >> lvl) & 1);
    if constexpr (SC) part[u][0] = scale16<T>(part[u][0], m);
    const size_t i = base + (size_t)u * kBlock;
    // non-temporal stores: 23.91 vs 24.12 us at the C3 chunk shape, 0.99 of
    // the 9 streams' read-only ceiling (profiles/r3_tree_variants.txt); nt
    // stores keep the line in the XCD's L2 for the allgather that sends it
    if (!GUARD || i < nvec) __builtin_nontemporal_store(part[u][0], vo + i);
  }
}

// elements before the 16-B aligned body and after its last vector (one
// workgroup; launched only when there are any: keeping this code out of the
// body kernel keeps its register count -- and occupancy -- at the body's own)
template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_edges(TreeArgs t) {
  constexpr size_t V = 16 / sizeof(T);
  T *out = (T *)t.out;
  for (size_t i = threadIdx.x; i < t.head; i += kBlock) out[i] = tree_scalar<T, OP, NL>(t, i);
  for (size_t i = t.head + t.nvec * V + threadIdx.x; i < t.n; i += kBlock) out[i] = tree_scalar<T, OP, NL>(t, i);
}

template <typename T, int OP, int NL, int U>
__global__ __launch_bounds__(kBlock) void k_reduce_tree(TreeArgs t) {
  T *out = (T *)t.out;
  // leaf base pointers into registers once (loading them from the kernel
  // arguments inside guarded loads put an s_waitcnt in front of every load)
  const u32x4 *lp[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) lp[j] = reinterpret_cast<const u32x4 *>((const T *)t.leaf[j] + t.head);
  u32x4 *vo = reinterpret_cast<u32x4 *>(out + t.head);
  const size_t base = (size_t)blockIdx.x * kBlock * U + threadIdx.x;
  if ((size_t)(blockIdx.x + 1) * kBlock * U <= t.nvec) tree_tile<T, OP, NL, U, false>(lp, vo, base, t.nvec, t.swap);
  else tree_tile<T, OP, NL, U, true>(lp, vo, base, t.nvec, t.swap);
}

// operands not co-aligned mod 16 B: scalar grid-stride
template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_scalar(TreeArgs t) {
  T *out = (T *)t.out;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < t.n; i += (size_t)gridDim.x * kBlock)
    out[i] = tree_scalar<T, OP, NL>(t, i);
}

// The scaled tree (bine_reduce_tree_scaled; the flagged trees of the scaled
// collectives): sibling kernels of the three above with S applied to the final
// value in registers -- the same loads, the same tree, the same store, one
// multiply more per element.  Siblings, not a flag on the kernels above, so
// that those keep their arguments and their device code.  Instantiated by
// tree_nl for the four floating types, never in the opset-1 compilation.
template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_edges_sc(TreeArgs t, mul_of<T> m) {
  constexpr size_t V = 16 / sizeof(T);
  T *out = (T *)t.out;
  for (size_t i = threadIdx.x; i < t.head; i += kBlock) out[i] = scale1<T>(tree_scalar<T, OP, NL>(t, i), m);
  for (size_t i = t.head + t.nvec * V + threadIdx.x; i < t.n; i += kBlock)
    out[i] = scale1<T>(tree_scalar<T, OP, NL>(t, i), m);
}

template <typename T, int OP, int NL, int U>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_sc(TreeArgs t, mul_of<T> m) {
  T *out = (T *)t.out;
  const u32x4 *lp[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) lp[j] = reinterpret_cast<const u32x4 *>((const T *)t.leaf[j] + t.head);
  u32x4 *vo = reinterpret_cast<u32x4 *>(out + t.head);
  const size_t base = (size_t)blockIdx.x * kBlock * U + threadIdx.x;
  if ((size_t)(blockIdx.x + 1) * kBlock * U <= t.nvec)
    tree_tile<T, OP, NL, U, false, true>(lp, vo, base, t.nvec, t.swap, m);
  else tree_tile<T, OP, NL, U, true, true>(lp, vo, base, t.nvec, t.swap, m);
}

template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_scalar_sc(TreeArgs t, mul_of<T> m) {
  T *out = (T *)t.out;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < t.n; i += (size_t)gridDim.x * kBlock)
    out[i] = scale1<T>(tree_scalar<T, OP, NL>(t, i), m);
}

// the launches of one tree: the plain kernels, or (SC) their _sc siblings,
// which take the multiplier as one more argument
template <typename T, int OP, int NL, bool SC>
static hipError_t tree_launch(const TreeArgs &t, hipStream_t st, [[maybe_unused]] mul_of<T> m) {
  constexpr int U = NL == 2 ? 8 : NL <= 8 ? 4 : 2;  // tools/tree_variants.hip: <8,4> 25.2 us, <8,2> 26.5 us
  constexpr size_t V = 16 / sizeof(T);
  const dim3 blk(kBlock);
  if (t.vec) {
    const dim3 tiles((unsigned)((t.nvec + (size_t)kBlock * U - 1) / ((size_t)kBlock * U)));
    if (tiles.x) {
      if constexpr (SC) hipLaunchKernelGGL((k_reduce_tree_sc<T, OP, NL, U>), tiles, blk, 0, st, t, m);
      else hipLaunchKernelGGL((k_reduce_tree<T, OP, NL, U>), tiles, blk, 0, st, t);
    }
    if (t.head || t.head + t.nvec * V < t.n) {
      if constexpr (SC) hipLaunchKernelGGL((k_reduce_tree_edges_sc<T, OP, NL>), dim3(1), blk, 0, st, t, m);
      else hipLaunchKernelGGL((k_reduce_tree_edges<T, OP, NL>), dim3(1), blk, 0, st, t);
    }
  } else {
    const dim3 blocks(scalar_blocks(t.n));
    if constexpr (SC) hipLaunchKernelGGL((k_reduce_tree_scalar_sc<T, OP, NL>), blocks, blk, 0, st, t, m);
    else hipLaunchKernelGGL((k_reduce_tree_scalar<T, OP, NL>), blocks, blk, 0, st, t);
  }
  return hipGetLastError();
}

// sc != nullptr: the scaled siblings with multiplier *sc (the four floating
// types only, and not in the opset-1 compilation, which has no scaled entry
// point; hipErrorInvalidValue otherwise)
template <typename T, int OP, int NL>
static hipError_t tree_nl(const TreeArgs &t, hipStream_t st, const double *sc) {
  if (!sc) return tree_launch<T, OP, NL, false>(t, st, {});
  if constexpr (BINE_OPSET != 1 && kScaleT<T>) return tree_launch<T, OP, NL, true>(t, st, (mul_of<T>)*sc);
  else return hipErrorInvalidValue;
}

// fills in the split of t.n elements of T, then the tree for (op, nl)
template <typename T>
static hipError_t tree_op(int nl, TreeArgs &t, int op, hipStream_t st, const double *sc) {
  const uintptr_t oo = (uintptr_t)t.out;
  bool co = (oo % sizeof(T)) == 0;
  for (int j = 0; j < nl; j++) co = co && (((uintptr_t)t.leaf[j] ^ oo) & 15) == 0;
  const VecSplit vs = co ? vec_split(oo, t.n, sizeof(T)) : VecSplit{t.n, 0};
  t.vec = co ? 1 : 0;
  t.head = vs.head;
  t.nvec = vs.nvec;
  return with_op<T>(op, [&](auto opc) {
    return with_nl(nl, [&](auto nlc) { return tree_nl<T, decltype(opc)::value, decltype(nlc)::value>(t, st, sc); });
  });
}

static int reduce_tree_run(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op, void *stream,
                           unsigned swap, const double *sc) {
  if (nl < 2 || nl > kMaxLeaves || (nl & (nl - 1))) return BINE_ERR_ARG;
  size_t scale;
  dtype = canon_dtype(dtype, op, &scale);
  if (dtype < 0) return BINE_ERR_ARG;
  TreeArgs t{};
  for (int j = 0; j < nl; j++) t.leaf[j] = leaf[j];
  t.out = out;
  t.n = count * scale;
  t.swap = swap;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) {
    return status(tree_op<typename decltype(tag)::type>(nl, t, op, st, sc));
  });
}

int BINE_FN(launch_reduce_tree)(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                                void *stream, unsigned swap) {
  if (count == 0) return BINE_SUCCESS;
#if BINE_OPSET == 0
  if (const int o = owner_opset(dtype, op))
    return o == 2 ? launch_reduce_tree_h16(nl, leaf, out, count, dtype, op, stream, swap)
                  : launch_reduce_tree_logic(nl, leaf, out, count, dtype, op, stream, swap);
#endif
  return reduce_tree_run(nl, leaf, out, count, dtype, op, stream, swap, nullptr);
}

#if BINE_OPSET != 1
// the same tree with S applied to every final value in the same launch
// (k_reduce_tree_sc); the caller has checked bine_scale_valid(dtype, op)
int BINE_FN(launch_reduce_tree_scaled)(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                                       void *stream, unsigned swap, double scale) {
  if (!bine_scale_valid(dtype, op)) return BINE_ERR_ARG;
  if (count == 0) return BINE_SUCCESS;
#if BINE_OPSET == 0
  if (owner_opset(dtype, op) == 2)
    return launch_reduce_tree_scaled_h16(nl, leaf, out, count, dtype, op, stream, swap, scale);
#endif
  return reduce_tree_run(nl, leaf, out, count, dtype, op, stream, swap, &scale);
}
#endif

#if BINE_OPSET != 1
// ----------------------------------------------------------------------------
// k_scale: out[i] = S(in[i]) (bine_scale; the trailing SCALE primitive of the
// scaled collectives).  k_copy's shape: one tile of kBlock * kScaleU 16-B
// vectors per workgroup, every load issued before the first store,
// non-temporal stores; the loads non-temporal too when out of place (OOP: the
// input is read once), plain in place (the line is written right back).
// Elements before the first 16-B boundary of `out` and after the last full
// vector go scalar through workgroup 0; operands that are not co-aligned mod
// 16 B take the scalar grid-stride kernel.  `in` may equal `out`.
constexpr int kScaleU = 8;

template <typename T, bool OOP>
__global__ __launch_bounds__(kBlock) void k_scale(const T *in, T *out, size_t head, size_t nvec, size_t n,
                                                  mul_of<T> m) {
  constexpr size_t V = 16 / sizeof(T);
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += kBlock) out[i] = scale1<T>(in[i], m);
    for (size_t i = head + nvec * V + threadIdx.x; i < n; i += kBlock) out[i] = scale1<T>(in[i], m);
  }
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(in + head);
  u32x4 *vd = reinterpret_cast<u32x4 *>(out + head);
  const size_t base = (size_t)blockIdx.x * kBlock * kScaleU + threadIdx.x;
  if (base + (kScaleU - 1) * (size_t)kBlock < nvec) {
    u32x4 x[kScaleU];
#pragma unroll
    for (int u = 0; u < kScaleU; u++) x[u] = ld<OOP>(vs + base + (size_t)u * kBlock);
#pragma unroll
    for (int u = 0; u < kScaleU; u++)
      __builtin_nontemporal_store(scale16<T>(x[u], m), vd + base + (size_t)u * kBlock);
  } else {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) vd[i] = scale16<T>(vs[i], m);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_scale_scalar(const T *in, T *out, size_t n, mul_of<T> m) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    out[i] = scale1<T>(in[i], m);
}

template <typename T>
static hipError_t scale_t(const void *in, void *out, size_t n, double scale, hipStream_t st) {
  const mul_of<T> m = (mul_of<T>)scale;  // (float)scale: round to nearest even
  const T *pi = (const T *)in;
  T *po = (T *)out;
  const uintptr_t io = (uintptr_t)in, oo = (uintptr_t)out;
  if (((io ^ oo) & 15) != 0 || (oo % sizeof(T)) != 0) {
    hipLaunchKernelGGL((k_scale_scalar<T>), dim3(scalar_blocks(n)), dim3(kBlock), 0, st, pi, po, n, m);
    return hipGetLastError();
  }
  const auto [head, nvec] = vec_split(oo, n, sizeof(T));
  const size_t tiles = (nvec + (size_t)kBlock * kScaleU - 1) / ((size_t)kBlock * kScaleU);
  const unsigned blocks = (unsigned)(tiles ? tiles : 1);
  if (in == out) hipLaunchKernelGGL((k_scale<T, false>), dim3(blocks), dim3(kBlock), 0, st, pi, po, head, nvec, n, m);
  else hipLaunchKernelGGL((k_scale<T, true>), dim3(blocks), dim3(kBlock), 0, st, pi, po, head, nvec, n, m);
  return hipGetLastError();
}

int BINE_FN(launch_scale)(const void *in, void *out, size_t count, int dtype, double scale, void *stream) {
  if (!bine_scale_valid(dtype, BINE_SUM)) return BINE_ERR_ARG;
  if (count == 0) return BINE_SUCCESS;
#if BINE_OPSET == 0
  if (owner_opset(dtype, BINE_SUM) == 2) return launch_scale_h16(in, out, count, dtype, scale, stream);
#endif
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    if constexpr (kScaleT<T>) return status(scale_t<T>(in, out, count, scale, st));
    else return BINE_ERR_ARG;
  });
}

// ----------------------------------------------------------------------------
// segmented sum of squares and segmented scale (bine_sumsq_segments /
// bine_clip_segments: the global gradient norm and the clipping of a bucket).
// Both take TileTable's dispatch over the table plan_seg_launches builds with
// destination = source = the buffer (plan_norm_launches): a tile is kBlock *
// kScaleU 16-B aligned vectors of whole elements, and a segment's first
// workgroup also takes the elements before the first and after the last vector.
static_assert(kCopyTileVecs == (uint64_t)kBlock * kScaleU, "the planner's tile is k_scale's");

struct NormSeg {
  uint8_t *p;
  uint64_t bytes;
};

// The workgroup's sum of one double per lane, in an order fixed by the lane
// numbers alone: the 64 lanes of a wave by a butterfly of __shfl_xor (both
// partners add the same two values, so every lane holds the same bits), the
// waves through LDS in wave order.  Valid in every thread.
__device__ __forceinline__ double wg_sum(double v, double *part) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; w++) s += part[w];
  return s;
}

// x widened exactly to binary64 and squared there (exact for the three narrow
// types: at most 24-bit significands; one rounding for double)
template <typename T>
__device__ __forceinline__ double sq64(T x) {
  const double d = (double)x;
  return d * d;
}
// the squares of one 16-B vector's elements, added in element order
template <typename T>
__device__ __forceinline__ double sumsq16(u32x4 v) {
  constexpr int N = 16 / (int)sizeof(T);
  T e[N];
  __builtin_memcpy(e, &v, 16);
  double s = sq64<T>(e[0]);
#pragma unroll
  for (int i = 1; i < N; i++) s += sq64<T>(e[i]);
  return s;
}

// k_sumsq_segs: workgroup t stores the sum of squares of its tile to
// scratch[t].  Every load is issued before the first use; a lane adds its
// vectors' sums in vector order, wg_sum combines the lanes.  No atomics, no
// order decided by arrival: the bits depend on the data, the counts, the type
// and the buffers' addresses mod 16 B alone.
struct SumsqSegs {
  TileTable<kSegsPerLaunch> tab;
  double *scratch;  // this launch's first workgroup's double
  NormSeg s[kSegsPerLaunch];
};
static_assert(sizeof(SumsqSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void k_sumsq_segs(SumsqSegs a) {
  __shared__ double part[kBlock / 64];
  const uint32_t t = blockIdx.x;
  const auto [k, wt] = a.tab.find(t);
  const uint8_t *p = a.s[k].p;
  const size_t n = a.s[k].bytes;
  const size_t head = seg_head((uintptr_t)p, n), nvec = seg_nvec(n, head);
  double acc = 0.0;
  if (wt == 0) {  // head and tail elements of this segment
    const T *e = reinterpret_cast<const T *>(p);
    const size_t ne = n / sizeof(T), he = head / sizeof(T), te = (head + nvec * 16) / sizeof(T);
    for (size_t i = threadIdx.x; i < he; i += kBlock) acc += sq64<T>(e[i]);
    for (size_t i = te + threadIdx.x; i < ne; i += kBlock) acc += sq64<T>(e[i]);
  }
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(p + head);
  const size_t base = (size_t)wt * kBlock * kScaleU + threadIdx.x;
  if (base + (kScaleU - 1) * (size_t)kBlock < nvec) {
    u32x4 x[kScaleU];
#pragma unroll
    for (int u = 0; u < kScaleU; u++) x[u] = ld<NT>(vs + base + (size_t)u * kBlock);
#pragma unroll
    for (int u = 0; u < kScaleU; u++) acc += sumsq16<T>(x[u]);
  } else {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) acc += sumsq16<T>(ld<NT>(vs + i));
    }
  }
  acc = wg_sum(acc, part);
  if (threadIdx.x == 0) a.scratch[t] = acc;
}

int BINE_FN(launch_sumsq_tiles)(const std::vector<SegLaunch> &ls, const void *const *bufs, const size_t *counts,
                                int dtype, double *scratch, bool nt, void *stream) {
#if BINE_OPSET == 0
  if (h16_dtype(dtype)) return launch_sumsq_tiles_h16(ls, bufs, counts, dtype, scratch, nt, stream);
#endif
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    if constexpr (kScaleT<T>) {
      uint64_t t0 = 0;
      for (const SegLaunch &L : ls) {
        SumsqSegs a;
        a.scratch = scratch + t0;
        fill_segs(a, L, [&](int s) {
          return NormSeg{(uint8_t *)const_cast<void *>(bufs[L.seg[s]]), (uint64_t)(counts[L.seg[s]] * sizeof(T))};
        });
        if (nt) hipLaunchKernelGGL((k_sumsq_segs<T, true>), dim3(L.tile0[L.nseg]), dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL((k_sumsq_segs<T, false>), dim3(L.tile0[L.nseg]), dim3(kBlock), 0, st, a);
        if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
        t0 += L.tile0[L.nseg];
      }
      return BINE_SUCCESS;
    } else return BINE_ERR_ARG;
  });
}

#if BINE_OPSET == 0
// k_sumsq_fold: workgroup s adds the partials of the launch's s-th segment --
// lane l takes partials l, l + kBlock, ... in index order, wg_sum combines the
// lanes -- and stores out[seg[s]].  k_sumsq_total: the empty segments' +0.0,
// then out[n] = out[0] + ... + out[n - 1], added in that order by one thread
// out of LDS.
struct SumsqFold {
  uint32_t tile0[kSegsPerLaunch + 1];
  uint16_t seg[kSegsPerLaunch];
  const double *scratch;  // this launch's first workgroup's double
  double *out;
};
struct SumsqTotal {
  int n;
  uint32_t empty[BINE_MULTI_MAX / 32];  // bit k: segment k has no element
  double *out;
};
static_assert(BINE_MULTI_MAX % 32 == 0 && BINE_MULTI_MAX <= 65536, "SumsqTotal::empty, SumsqFold::seg");

__global__ __launch_bounds__(kBlock) void k_sumsq_fold(SumsqFold a) {
  __shared__ double part[kBlock / 64];
  const uint32_t s = blockIdx.x, hi = a.tile0[s + 1];
  double acc = 0.0;
  for (uint32_t i = a.tile0[s] + threadIdx.x; i < hi; i += kBlock) acc += a.scratch[i];
  acc = wg_sum(acc, part);
  if (threadIdx.x == 0) a.out[a.seg[s]] = acc;
}

__global__ __launch_bounds__(kBlock) void k_sumsq_total(SumsqTotal a) {
  __shared__ double v[BINE_MULTI_MAX];
  for (int k = threadIdx.x; k < a.n; k += kBlock) {
    const bool empty = (a.empty[k >> 5] >> (k & 31)) & 1;
    if (empty) a.out[k] = 0.0;
    v[k] = empty ? 0.0 : a.out[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < a.n; k++) s += v[k];
    a.out[a.n] = s;
  }
}

// BINE_SUMSQ_NT in the environment (read at every call): 1 / 0 = non-temporal
// / plain loads in k_sumsq_segs; unset: plain
static bool sumsq_nt() {
  const char *e = getenv("BINE_SUMSQ_NT");
  return e && *e == '1';
}

int launch_sumsq_segments(int n, const void *const *bufs, const size_t *counts, int dtype, double *out,
                          double *scratch, size_t scratch_doubles, void *stream) {
  if (!norm_esz(dtype)) return BINE_ERR_ARG;
  std::vector<uint64_t> addr;
  if (const int rc = seg_list_addrs(n, counts, {bufs}, addr)) return rc;
  std::vector<SegLaunch> ls;
  uint64_t tiles = 0;
  if (const int rc = plan_norm_launches(n, addr.data(), counts, dtype, ls, &tiles)) return rc;
  if (!out || ((uintptr_t)out & 7)) return BINE_ERR_ARG;
  if (scratch_doubles < tiles || (tiles && (!scratch || ((uintptr_t)scratch & 7)))) return BINE_ERR_ARG;
  if (const int rc = launch_sumsq_tiles(ls, bufs, counts, dtype, scratch, sumsq_nt(), stream)) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint64_t t0 = 0;
  for (const SegLaunch &L : ls) {
    SumsqFold f;
    fill_slots(L, f.tile0, f.seg, [&](int s) { return (uint16_t)L.seg[s]; });
    f.scratch = scratch + t0;
    f.out = out;
    hipLaunchKernelGGL(k_sumsq_fold, dim3((unsigned)L.nseg), dim3(kBlock), 0, st, f);
    if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    t0 += L.tile0[L.nseg];
  }
  SumsqTotal tot;
  tot.n = n;
  tot.out = out;
  memset(tot.empty, 0, sizeof tot.empty);
  for (int k = 0; k < n; k++)
    if (!counts[k]) tot.empty[k >> 5] |= 1u << (k & 31);
  hipLaunchKernelGGL(k_sumsq_total, dim3(1), dim3(kBlock), 0, st, tot);
  return hipGetLastError() == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP;
}
#endif  // BINE_OPSET == 0

// k_scale_segs: k_scale's in-place tile body on tile t's segment, the factor
// read from device memory.  Every workgroup derives the coefficient itself
// (one binary64 square root and one division, both IEEE: no fast-math),
//   r = max_norm / (sqrt(*norm2) + eps),  c = r < 1.0 ? r : 1.0,
// so no launch sits between the norm and the scale; the first workgroup stores
// it to *coef_out.  c == 1.0: nothing is stored.  A full tile's loads are
// issued before the coefficient's arithmetic, which so overlaps them.
struct ScaleSegs {
  TileTable<kSegsPerLaunch> tab;  // nseg 0: the launch only stores the coefficient
  const double *norm2;
  double *coef_out;  // NULL: not stored
  double max_norm, eps;
  NormSeg s[kSegsPerLaunch];
};
static_assert(sizeof(ScaleSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

__device__ __forceinline__ double clip_coef(const ScaleSegs &a) {
  const double r = a.max_norm / (__builtin_sqrt(*a.norm2) + a.eps);
  return r < 1.0 ? r : 1.0;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_scale_segs(ScaleSegs a) {
  constexpr size_t V = 16 / sizeof(T);
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.coef_out) *a.coef_out = clip_coef(a);
  if (a.tab.nseg == 0) return;
  const auto [k, wt] = a.tab.find(blockIdx.x);
  uint8_t *p = a.s[k].p;
  const size_t n = a.s[k].bytes;
  const size_t head = seg_head((uintptr_t)p, n), nvec = seg_nvec(n, head);
  u32x4 *vd = reinterpret_cast<u32x4 *>(p + head);
  const size_t base = (size_t)wt * kBlock * kScaleU + threadIdx.x;
  const bool full = base + (kScaleU - 1) * (size_t)kBlock < nvec;
  u32x4 x[kScaleU];
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) x[u] = vd[base + (size_t)u * kBlock];
  }
  const double c = clip_coef(a);
  if (c == 1.0) return;
  const mul_of<T> m = (mul_of<T>)c;  // (float)c: round to nearest even, as bine_scale's host conversion
  if (wt == 0) {  // head and tail elements of this segment
    T *e = reinterpret_cast<T *>(p);
    const size_t ne = n / sizeof(T), he = head / sizeof(T);
    for (size_t i = threadIdx.x; i < he; i += kBlock) e[i] = scale1<T>(e[i], m);
    for (size_t i = he + nvec * V + threadIdx.x; i < ne; i += kBlock) e[i] = scale1<T>(e[i], m);
  }
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++)
      __builtin_nontemporal_store(scale16<T>(x[u], m), vd + base + (size_t)u * kBlock);
  } else {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) vd[i] = scale16<T>(vd[i], m);
    }
  }
}

int BINE_FN(launch_clip_segments)(int n, void *const *bufs, const size_t *counts, int dtype, const double *norm2,
                                  double max_norm, double eps, double *coef_out, void *stream) {
  if (!norm_esz(dtype)) return BINE_ERR_ARG;
#if BINE_OPSET == 0
  if (h16_dtype(dtype))  // the twin runs every check below
    return launch_clip_segments_h16(n, bufs, counts, dtype, norm2, max_norm, eps, coef_out, stream);
#endif
  std::vector<uint64_t> addr;
  if (const int rc = seg_list_addrs(n, counts, {bufs}, addr)) return rc;
  std::vector<SegLaunch> ls;
  if (const int rc = plan_norm_launches(n, addr.data(), counts, dtype, ls, nullptr)) return rc;
  if (!norm2 || ((uintptr_t)norm2 & 7) || ((uintptr_t)coef_out & 7)) return BINE_ERR_ARG;
  if (!(max_norm >= 0.0) || !(eps >= 0.0)) return BINE_ERR_ARG;  // negative or NaN
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    if constexpr (kScaleT<T>) {
      ScaleSegs a;
      a.norm2 = norm2, a.coef_out = coef_out, a.max_norm = max_norm, a.eps = eps;
      auto fill = [&](const SegLaunch &L) {
        fill_segs(a, L, [&](int s) {
          return NormSeg{(uint8_t *)bufs[L.seg[s]], (uint64_t)(counts[L.seg[s]] * sizeof(T))};
        });
      };
      if (ls.empty()) {  // nothing to scale: the coefficient alone, from a launch without segments
        if (!coef_out) return BINE_SUCCESS;
        fill(SegLaunch{});
        hipLaunchKernelGGL((k_scale_segs<T>), dim3(1), dim3(kBlock), 0, st, a);
        return status(hipGetLastError());
      }
      for (const SegLaunch &L : ls) {
        fill(L);
        hipLaunchKernelGGL((k_scale_segs<T>), dim3(L.tile0[L.nseg]), dim3(kBlock), 0, st, a);
        if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
        a.coef_out = nullptr;  // stored once, by the first launch
      }
      return BINE_SUCCESS;
    } else return BINE_ERR_ARG;
  });
}
#endif  // BINE_OPSET != 1

#if BINE_OPSET == 2
// ----------------------------------------------------------------------------
// wide (binary32-accumulating) reductions of the 16-bit types (bine_amd.h,
// "wide reductions"): k_widen / k_narrow, the conversion passes of path A, and
// k_reduce_tree_wide, path B's tree -- the leaves stay 16-bit in memory, every
// level of the reference's tree is one binary32 operation in registers, one
// binary32 multiplication by (float)scale follows (by 1.0f for an unscaled
// call: the identity on every non-NaN binary32 value, -0 and subnormals
// included) and ONE nearest-even narrowing precedes the store.
//
// W8: the 8 elements of one 16-B vector as binary32, in element order.  The
// widened leaves and the final product are pinned in VGPRs by an empty asm (no
// instruction is emitted), so the compiler sees plain binary32 operands: it
// can fold neither a widening into the first operation nor the product into
// the narrowing (v_fma_mix* / v_fma_mixlo_f16; see scale1 for the -0 * 0 case
// such a fold gets wrong).  Every level's value exists as a binary32 VGPR.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
struct W8 {
  f32x4 a, b;  // elements 0..3, 4..7
};
__device__ __forceinline__ void pin(W8 &w) { asm volatile("" : "+v"(w.a), "+v"(w.b)); }

template <typename T>
__device__ __forceinline__ W8 widen16(u32x4 v) {
  W8 w;
  if constexpr (std::is_same_v<T, F16>) {
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    f16x8 h;
    __builtin_memcpy(&h, &v, 16);
    const f32x8 f = __builtin_convertvector(h, f32x8);  // v_cvt_f32_f16: exact, subnormals kept
    w.a = __builtin_shufflevector(f, f, 0, 1, 2, 3);
    w.b = __builtin_shufflevector(f, f, 4, 5, 6, 7);
  } else {
    static_assert(std::is_same_v<T, BF16>, "wide types: float16, bfloat16");
    // a bfloat16 is the upper half of a binary32: even elements by a shift, odd ones by a mask
    const u32x4 vlo = v << 16, vhi = v & 0xffff0000u;
    f32x4 lo, hi;
    __builtin_memcpy(&lo, &vlo, 16);
    __builtin_memcpy(&hi, &vhi, 16);
    w.a = __builtin_shufflevector(lo, hi, 0, 4, 1, 5);
    w.b = __builtin_shufflevector(lo, hi, 2, 6, 3, 7);
  }
  pin(w);
  return w;
}

// round to nearest even into the 16-bit format (v_cvt_f16_f32 -- never the
// packed round-toward-zero conversion -- resp. v_cvt_pk_bf16_f32); subnormal
// results kept, overflow gives +-inf, NaN stays NaN
template <typename T>
__device__ __forceinline__ u32x4 narrow16(W8 w) {
  pin(w);
  const f32x8 f = __builtin_shufflevector(w.a, w.b, 0, 1, 2, 3, 4, 5, 6, 7);
  u32x4 r;
  if constexpr (std::is_same_v<T, F16>) {
    typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
    const f16x8 h = __builtin_convertvector(f, f16x8);
    __builtin_memcpy(&r, &h, 16);
  } else {
    typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
    const bf16x8 h = __builtin_convertvector(f, bf16x8);
    __builtin_memcpy(&r, &h, 16);
  }
  return r;
}

template <typename T>
__device__ __forceinline__ float widen1(T x) {
  float f = (float)x;
  asm volatile("" : "+v"(f));
  return f;
}
template <typename T>
__device__ __forceinline__ T narrow1(float f) {
  asm volatile("" : "+v"(f));
  return (T)f;
}

// one level's combine in binary32: apply<float, OP> element by element
template <int OP>
__device__ __forceinline__ W8 wcomb(W8 l, W8 r, bool sw) {
  const W8 io = sw ? r : l, in = sw ? l : r;
  W8 o;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o.a[k] = apply<float, OP>(io.a[k], in.a[k]);
    o.b[k] = apply<float, OP>(io.b[k], in.b[k]);
  }
  return o;
}

template <typename T, int OP, int NL>
__device__ __forceinline__ T wide_scalar(const TreeArgs &t, size_t i, float m) {
  float v[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) v[j] = widen1<T>(((const T *)t.leaf[j])[i]);
  int lvl = 0;
#pragma unroll
  for (int w = 1; w < NL; w <<= 1, lvl++)
#pragma unroll
    for (int j = 0; j < NL; j += 2 * w) v[j] = comb<float, OP>(v[j], v[j + w], (t.swap >> lvl) & 1);
  return narrow1<T>(v[0] * m);
}

// tree_tile's shape -- the same loads (position 0 plain, the others
// non-temporal), groups of G = min(NL, 8) leaves forming complete subtrees,
// U vectors of each leaf per lane in flight, non-temporal stores -- with
// every vector widened as it is consumed: the loads stay 16-B vectors of
// 16-bit elements, only the values being combined are binary32.
template <typename T, int OP, int NL, int U, bool GUARD>
__device__ __forceinline__ void wide_tile(const u32x4 *const *lp, u32x4 *vo, size_t base, size_t nvec, unsigned swap,
                                          float m) {
  constexpr int G = NL < 8 ? NL : 8, NG = NL / G, LG = G == 2 ? 1 : G == 4 ? 2 : 3;
  W8 part[U][NG];
#pragma unroll
  for (int g = 0; g < NG; g++) {
    u32x4 v[U][G];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (!GUARD || i < nvec) {
        if (g == 0) v[u][0] = lp[0][i];
#pragma unroll
        for (int j = g == 0 ? 1 : 0; j < G; j++) v[u][j] = __builtin_nontemporal_load(lp[g * G + j] + i);
      } else {
#pragma unroll
        for (int j = 0; j < G; j++) v[u][j] = u32x4{0, 0, 0, 0};
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      W8 x[G];
#pragma unroll
      for (int j = 0; j < G; j++) x[j] = widen16<T>(v[u][j]);
      int lvl = 0;
#pragma unroll
      for (int w = 1; w < G; w <<= 1, lvl++)
#pragma unroll
        for (int j = 0; j < G; j += 2 * w) x[j] = wcomb<OP>(x[j], x[j + w], (swap >> lvl) & 1);
      part[u][g] = x[0];
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    int lvl = LG;
#pragma unroll
    for (int w = 1; w < NG; w <<= 1, lvl++)
#pragma unroll
      for (int g = 0; g < NG; g += 2 * w) part[u][g] = wcomb<OP>(part[u][g], part[u][g + w], (swap >> lvl) & 1);
    W8 p;
    p.a = part[u][0].a * m;
    p.b = part[u][0].b * m;
    const size_t i = base + (size_t)u * kBlock;
    if (!GUARD || i < nvec) __builtin_nontemporal_store(narrow16<T>(p), vo + i);
  }
}

template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_wide_edges(TreeArgs t, float m) {
  constexpr size_t V = 16 / sizeof(T);
  T *out = (T *)t.out;
  for (size_t i = threadIdx.x; i < t.head; i += kBlock) out[i] = wide_scalar<T, OP, NL>(t, i, m);
  for (size_t i = t.head + t.nvec * V + threadIdx.x; i < t.n; i += kBlock) out[i] = wide_scalar<T, OP, NL>(t, i, m);
}

template <typename T, int OP, int NL, int U>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_wide(TreeArgs t, float m) {
  T *out = (T *)t.out;
  const u32x4 *lp[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) lp[j] = reinterpret_cast<const u32x4 *>((const T *)t.leaf[j] + t.head);
  u32x4 *vo = reinterpret_cast<u32x4 *>(out + t.head);
  const size_t base = (size_t)blockIdx.x * kBlock * U + threadIdx.x;
  if ((size_t)(blockIdx.x + 1) * kBlock * U <= t.nvec) wide_tile<T, OP, NL, U, false>(lp, vo, base, t.nvec, t.swap, m);
  else wide_tile<T, OP, NL, U, true>(lp, vo, base, t.nvec, t.swap, m);
}

template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_reduce_tree_wide_scalar(TreeArgs t, float m) {
  T *out = (T *)t.out;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < t.n; i += (size_t)gridDim.x * kBlock)
    out[i] = wide_scalar<T, OP, NL>(t, i, m);
}

// vectors of each leaf per lane in flight: k_reduce_tree's, halved where the
// binary32 intermediates would otherwise cost a wave of occupancy (DESIGN.md,
// "wide reductions": the register budget)
template <int NL>
constexpr int kWideU = NL == 2 ? 8 : NL == 4 ? 4 : NL == 8 ? 2 : 1;

template <typename T, int OP, int NL>
static hipError_t wide_launch(const TreeArgs &t, hipStream_t st, float m) {
  constexpr int U = kWideU<NL>;
  constexpr size_t V = 16 / sizeof(T);
  const dim3 blk(kBlock);
  if (t.vec) {
    const dim3 tiles((unsigned)((t.nvec + (size_t)kBlock * U - 1) / ((size_t)kBlock * U)));
    if (tiles.x) hipLaunchKernelGGL((k_reduce_tree_wide<T, OP, NL, U>), tiles, blk, 0, st, t, m);
    if (t.head || t.head + t.nvec * V < t.n)
      hipLaunchKernelGGL((k_reduce_tree_wide_edges<T, OP, NL>), dim3(1), blk, 0, st, t, m);
  } else {
    hipLaunchKernelGGL((k_reduce_tree_wide_scalar<T, OP, NL>), dim3(scalar_blocks(t.n)), blk, 0, st, t, m);
  }
  return hipGetLastError();
}

int launch_reduce_tree_wide_h16(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                                void *stream, unsigned swap, double scale) {
  if (!bine_wide_valid(dtype, op)) return BINE_ERR_ARG;
  if (nl < 2 || nl > kMaxLeaves || (nl & (nl - 1))) return BINE_ERR_ARG;
  if (count == 0) return BINE_SUCCESS;
  TreeArgs t{};
  for (int j = 0; j < nl; j++) t.leaf[j] = leaf[j];
  t.out = out;
  t.n = count;
  t.swap = swap;
  const uintptr_t oo = (uintptr_t)out;
  bool co = (oo % 2) == 0;
  for (int j = 0; j < nl; j++) co = co && (((uintptr_t)leaf[j] ^ oo) & 15) == 0;
  const VecSplit vs = co ? vec_split(oo, count, 2) : VecSplit{count, 0};
  t.vec = co ? 1 : 0;
  t.head = vs.head;
  t.nvec = vs.nvec;
  const float m = (float)scale;  // round to nearest even
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return status(with_op<T>(op, [&](auto opc) {
      return with_nl(nl, [&](auto nlc) { return wide_launch<T, decltype(opc)::value, decltype(nlc)::value>(t, st, m); });
    }));
  });
}

// ----------------------------------------------------------------------------
// k_widen: out32[i] = in16[i] widened exactly; k_narrow: out16[i] = in32[i]
// rounded to nearest even.  One 16-B vector of 16-bit elements faces two of
// binary32; one tile of kBlock * kWnU 16-bit vectors per workgroup, every load
// issued before the first store.  The elements before the first 16-B boundary
// of the 16-bit operand and after its last whole vector go scalar through
// workgroup 0; operands whose 16-B boundaries do not coincide take the scalar
// grid-stride kernels.  The source is read once: non-temporal loads.  k_widen
// stores plainly (the collective that follows reads the workspace), k_narrow
// non-temporally, as k_scale and the trees store their results.
constexpr int kWnU = 4;

template <typename T>
__global__ __launch_bounds__(kBlock) void k_widen(const T *in, float *out, size_t head, size_t nvec, size_t n) {
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += kBlock) out[i] = widen1<T>(in[i]);
    for (size_t i = head + nvec * 8 + threadIdx.x; i < n; i += kBlock) out[i] = widen1<T>(in[i]);
  }
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(in + head);
  f32x4 *vd = reinterpret_cast<f32x4 *>(out + head);
  const size_t base = (size_t)blockIdx.x * kBlock * kWnU + threadIdx.x;
  if (base + (kWnU - 1) * (size_t)kBlock < nvec) {
    u32x4 x[kWnU];
#pragma unroll
    for (int u = 0; u < kWnU; u++) x[u] = __builtin_nontemporal_load(vs + base + (size_t)u * kBlock);
#pragma unroll
    for (int u = 0; u < kWnU; u++) {
      const W8 w = widen16<T>(x[u]);
      const size_t i = base + (size_t)u * kBlock;
      vd[2 * i] = w.a;
      vd[2 * i + 1] = w.b;
    }
  } else {
#pragma unroll
    for (int u = 0; u < kWnU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) {
        const W8 w = widen16<T>(vs[i]);
        vd[2 * i] = w.a;
        vd[2 * i + 1] = w.b;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_narrow(const float *in, T *out, size_t head, size_t nvec, size_t n) {
  if (blockIdx.x == 0) {
    for (size_t i = threadIdx.x; i < head; i += kBlock) out[i] = narrow1<T>(in[i]);
    for (size_t i = head + nvec * 8 + threadIdx.x; i < n; i += kBlock) out[i] = narrow1<T>(in[i]);
  }
  const f32x4 *vs = reinterpret_cast<const f32x4 *>(in + head);
  u32x4 *vd = reinterpret_cast<u32x4 *>(out + head);
  const size_t base = (size_t)blockIdx.x * kBlock * kWnU + threadIdx.x;
  if (base + (kWnU - 1) * (size_t)kBlock < nvec) {
    W8 x[kWnU];
#pragma unroll
    for (int u = 0; u < kWnU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      x[u].a = __builtin_nontemporal_load(vs + 2 * i);
      x[u].b = __builtin_nontemporal_load(vs + 2 * i + 1);
    }
#pragma unroll
    for (int u = 0; u < kWnU; u++) __builtin_nontemporal_store(narrow16<T>(x[u]), vd + base + (size_t)u * kBlock);
  } else {
#pragma unroll
    for (int u = 0; u < kWnU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) {
        W8 w;
        w.a = vs[2 * i];
        w.b = vs[2 * i + 1];
        vd[i] = narrow16<T>(w);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_widen_scalar(const T *in, float *out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    out[i] = widen1<T>(in[i]);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_narrow_scalar(const float *in, T *out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    out[i] = narrow1<T>(in[i]);
}

// the split of n elements at (p16, p32): `head` elements up to the first 16-B
// boundary of the 16-bit operand, where the binary32 operand must stand on a
// 16-B boundary too; false: the boundaries do not coincide (all scalar)
static bool wn_split(uintptr_t p16, uintptr_t p32, size_t n, VecSplit *vs) {
  if (p16 % 2 || p32 % 4) return false;
  const size_t head = ((16 - (p16 & 15)) & 15) / 2;
  if ((p32 + 4 * head) & 15) return false;
  *vs = {std::min(head, n), (n - std::min(head, n)) / 8};
  return true;
}
static unsigned wn_blocks(size_t nvec) {
  const size_t tiles = (nvec + (size_t)kBlock * kWnU - 1) / ((size_t)kBlock * kWnU);
  return (unsigned)(tiles ? tiles : 1);
}

int launch_widen_h16(const void *in16, void *out32, size_t count, int dtype, void *stream) {
  if (!bine_wide_valid(dtype, BINE_SUM)) return BINE_ERR_ARG;
  if (count == 0) return BINE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    VecSplit vs;
    if (wn_split((uintptr_t)in16, (uintptr_t)out32, count, &vs))
      hipLaunchKernelGGL((k_widen<T>), dim3(wn_blocks(vs.nvec)), dim3(kBlock), 0, st, (const T *)in16, (float *)out32,
                         vs.head, vs.nvec, count);
    else
      hipLaunchKernelGGL((k_widen_scalar<T>), dim3(scalar_blocks(count)), dim3(kBlock), 0, st, (const T *)in16,
                         (float *)out32, count);
    return status(hipGetLastError());
  });
}

int launch_narrow_h16(const void *in32, void *out16, size_t count, int dtype, void *stream) {
  if (!bine_wide_valid(dtype, BINE_SUM)) return BINE_ERR_ARG;
  if (count == 0) return BINE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    VecSplit vs;
    if (wn_split((uintptr_t)out16, (uintptr_t)in32, count, &vs))
      hipLaunchKernelGGL((k_narrow<T>), dim3(wn_blocks(vs.nvec)), dim3(kBlock), 0, st, (const float *)in32, (T *)out16,
                         vs.head, vs.nvec, count);
    else
      hipLaunchKernelGGL((k_narrow_scalar<T>), dim3(scalar_blocks(count)), dim3(kBlock), 0, st, (const float *)in32,
                         (T *)out16, count);
    return status(hipGetLastError());
  });
}

// ----------------------------------------------------------------------------
// k_adamw_segs: one AdamW step over a list of shards (bine_adamw_segments,
// bine_amd.h).  p, m, v are binary32 and updated in place, g (G: float,
// float16, bfloat16) is read only, pout (O, optional) receives the new
// parameter narrowed.  TileTable's dispatch over plan_norm_launches' table of
// p, cut at kAdamwSegsPerLaunch descriptors (plan_adamw_launches): a tile is
// kBlock * kScaleU 16-B aligned vectors of p, and a segment's first workgroup
// also takes the elements before the first and after the last vector.
//
// Every line of adamw1 is one correctly rounded binary32 operation
// (-ffp-contract=off: no FMA; IEEE division and square root; subnormals kept).
// The widened gradient and the new parameter pass through widen1 / narrow1,
// whose empty asm keeps a conversion from folding into a v_fma_mix*.
//
// A segment whose m, v, g and pout stand on a 4-element boundary wherever p
// stands on a 16-B one takes the vector body (a lane handles 4 consecutive
// elements: 16-B accesses of p, m, v, 8-B or 16-B ones of g and pout; all
// loads of a full tile issued before the first use, non-temporal stores); any
// other segment takes the element body (AdamwSegs::elem, set by the host), the
// same arithmetic through element-sized accesses.
struct AdamwSeg {
  float *p, *m, *v;
  const void *g;
  void *pout;  // NULL when the call has none
  uint64_t n;  // elements
};
struct AdamwSegs {
  TileTable<kAdamwSegsPerLaunch> tab;
  uint64_t elem;        // bit s: slot s takes the element body
  const double *gcoef;  // NULL: 1.0
  double grad_mul;
  float c[8];  // bine_adamw_consts: dk, b1, 1 - b1, b2, 1 - b2, rbc2, eps, ss
  AdamwSeg s[kAdamwSegsPerLaunch];
  const StepState *state;  // the DYN form's skip flag, multiplier and constants (last: s[] keeps its offsets)
};
static_assert(sizeof(AdamwSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// 4 consecutive elements of T as one access
template <typename T>
using vec4_of = std::conditional_t<sizeof(T) == 4, u32x4, u32x2>;

template <typename G>
__device__ __forceinline__ float adamw_widen(G x) {
  if constexpr (std::is_same_v<G, float>) return x;
  else return widen1<G>(x);
}
template <typename O>
__device__ __forceinline__ O adamw_narrow(float f) {
  if constexpr (std::is_same_v<O, float>) return f;
  else return narrow1<O>(f);
}

__device__ __forceinline__ void adamw1(float &p, float &m, float &v, float g, float gm, const float (&c)[8]) {
  const float gs = g * gm;
  const float p1 = p * c[0];
  m = (m * c[1]) + (gs * c[2]);
  v = (v * c[3]) + ((gs * gs) * c[4]);
  const float d = (__builtin_sqrtf(v) * c[5]) + c[6];
  p = p1 - (c[7] * (m / d));
}

// one lane's 4 elements: vector i of the segment's body
template <typename G, typename O, bool PO, bool NT>
__device__ __forceinline__ void adamw_vec(u32x4 xp, u32x4 xm, u32x4 xv, vec4_of<G> xg, float gm, const float (&c)[8],
                                          u32x4 *vp, u32x4 *vm, u32x4 *vv, [[maybe_unused]] vec4_of<O> *vo, size_t i) {
  float p[4], m[4], v[4];
  G g[4];
  [[maybe_unused]] O o[4];
  __builtin_memcpy(p, &xp, 16);
  __builtin_memcpy(m, &xm, 16);
  __builtin_memcpy(v, &xv, 16);
  __builtin_memcpy(g, &xg, sizeof g);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    adamw1(p[e], m[e], v[e], adamw_widen<G>(g[e]), gm, c);
    if constexpr (PO) o[e] = adamw_narrow<O>(p[e]);
  }
  __builtin_memcpy(&xp, p, 16);
  __builtin_memcpy(&xm, m, 16);
  __builtin_memcpy(&xv, v, 16);
  if constexpr (NT) {
    __builtin_nontemporal_store(xp, vp + i);
    __builtin_nontemporal_store(xm, vm + i);
    __builtin_nontemporal_store(xv, vv + i);
  } else {
    vp[i] = xp;
    vm[i] = xm;
    vv[i] = xv;
  }
  if constexpr (PO) {
    vec4_of<O> xo;
    __builtin_memcpy(&xo, o, sizeof o);
    if constexpr (NT) __builtin_nontemporal_store(xo, vo + i);
    else vo[i] = xo;
  }
}

// DYN (bine_adamw_segments_dyn): where the plain form reads *gcoef, every
// workgroup reads skip, gm and the eight constants from a.state (what
// k_step_update left there) -- after a full tile's loads are issued, so the
// state's latency hides behind them.  skip != 0: the workgroup returns before
// its first store.  a.gcoef, a.grad_mul and a.c are not read.
template <typename G, typename O, bool PO, bool DYN = false>
__global__ __launch_bounds__(kBlock) void k_adamw_segs(AdamwSegs a) {
  using GV = vec4_of<G>;
  using OV = vec4_of<O>;
  const auto [k, wt] = a.tab.find(blockIdx.x);
  float *p = a.s[k].p, *m = a.s[k].m, *v = a.s[k].v;
  const G *g = static_cast<const G *>(a.s[k].g);
  [[maybe_unused]] O *po = static_cast<O *>(a.s[k].pout);
  const size_t n = a.s[k].n;
  // the split in elements: p is 4-B aligned, so the head is whole elements and a vector is four
  const size_t he = seg_head((uintptr_t)p, 4 * n) / 4, nvec = (n - he) / 4;
  const bool elem = (a.elem >> k) & 1;
  u32x4 *vp = reinterpret_cast<u32x4 *>(p + he), *vm = reinterpret_cast<u32x4 *>(m + he);
  u32x4 *vv = reinterpret_cast<u32x4 *>(v + he);
  const GV *vg = reinterpret_cast<const GV *>(g + he);
  OV *vo = nullptr;
  if constexpr (PO) vo = reinterpret_cast<OV *>(po + he);
  const size_t base = (size_t)wt * kBlock * kScaleU + threadIdx.x;
  const bool full = !elem && ((size_t)wt + 1) * kBlock * kScaleU <= nvec;  // workgroup-uniform
  u32x4 xp[kScaleU], xm[kScaleU], xv[kScaleU];
  GV xg[kScaleU];
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      xp[u] = vp[i];
      xm[u] = vm[i];
      xv[u] = vv[i];
      xg[u] = vg[i];
    }
  }
  float gm;
  [[maybe_unused]] float cd[8];
  if constexpr (DYN) {
    if (a.state->d[5] != 0.0) return;  // workgroup-uniform: a skipped step stores nothing
    gm = (float)a.state->d[6];
#pragma unroll
    for (int j = 0; j < 8; j++) cd[j] = a.state->c[j];
  } else {
    // gm = (float)(c * grad_mul): the product in binary64, one rounding
    const double cf = a.gcoef ? *a.gcoef : 1.0;
    gm = (float)(cf * a.grad_mul);
  }
  const float(&c)[8] = *[&]() -> const float(*)[8] {
    if constexpr (DYN) return &cd;
    else return &a.c;
  }();
  auto one = [&](size_t i) {
    float pp = p[i], mm = m[i], vx = v[i];
    adamw1(pp, mm, vx, adamw_widen<G>(g[i]), gm, c);
    p[i] = pp;
    m[i] = mm;
    v[i] = vx;
    if constexpr (PO) po[i] = adamw_narrow<O>(pp);
  };
  if (wt == 0) {  // head and tail elements of this segment
    for (size_t i = threadIdx.x; i < he; i += kBlock) one(i);
    for (size_t i = he + nvec * 4 + threadIdx.x; i < n; i += kBlock) one(i);
  }
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++)
      adamw_vec<G, O, PO, true>(xp[u], xm[u], xv[u], xg[u], gm, c, vp, vm, vv, vo, base + (size_t)u * kBlock);
  } else if (!elem) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) adamw_vec<G, O, PO, false>(vp[i], vm[i], vv[i], vg[i], gm, c, vp, vm, vv, vo, i);
    }
  } else {  // the tile's elements one by one
    const size_t lo = he + (size_t)wt * kBlock * kScaleU * 4, end = he + nvec * 4;
    const size_t hi = lo + (size_t)kBlock * kScaleU * 4 < end ? lo + (size_t)kBlock * kScaleU * 4 : end;
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) one(i);
  }
}

// f(dtype_tag<T, dtype>{}) for the three types g and pout take
template <typename F>
static int with_adamw_dtype(int dtype, F &&f) {
  switch (dtype) {
    case BINE_FLOAT: return f(dtype_tag<float, BINE_FLOAT>{});
    case BINE_FLOAT16: return f(dtype_tag<F16, BINE_FLOAT16>{});
    case BINE_BFLOAT16: return f(dtype_tag<BF16, BINE_BFLOAT16>{});
    default: return BINE_ERR_ARG;
  }
}

// k_adamw_segs per launch of `ls`; a.gcoef / grad_mul / c (plain) or a.state (DYN) are the caller's
template <bool DYN>
static int adamw_issue(AdamwSegs &a, const std::vector<AdamwLaunch> &ls, void *const *p, void *const *m,
                       void *const *v, const void *const *g, void *const *pout, const size_t *counts, int gdtype,
                       int odtype, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return with_adamw_dtype(gdtype, [&](auto gtag) {
    using G = typename decltype(gtag)::type;
    return with_adamw_dtype(odtype, [&](auto otag) -> int {
      using O = typename decltype(otag)::type;
      for (const AdamwLaunch &L : ls) {
        a.elem = L.elem;
        fill_segs(a, L, [&](int s) {
          const int k = L.seg[s];
          return AdamwSeg{(float *)p[k], (float *)m[k], (float *)v[k], g[k], pout ? pout[k] : nullptr,
                          (uint64_t)counts[k]};
        });
        const dim3 grid(L.tile0[L.nseg]), blk(kBlock);
        // without pout one instantiation per G serves every odtype
        if (pout) hipLaunchKernelGGL((k_adamw_segs<G, O, true, DYN>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((k_adamw_segs<G, float, false, DYN>), grid, blk, 0, st, a);
        if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
      }
      return BINE_SUCCESS;
    });
  });
}

int launch_adamw_segments_h16(int n, void *const *p, void *const *m, void *const *v, const void *const *g,
                              void *const *pout, const size_t *counts, int gdtype, int odtype, double lr,
                              double beta1, double beta2, double eps, double weight_decay, int64_t step,
                              const double *gcoef, double grad_mul, void *stream) {
  AdamwSegs a;
  std::vector<AdamwLaunch> ls;
  if (const int rc = adamw_args(n, p, m, v, g, pout, counts, gdtype, odtype, lr, beta1, beta2, eps, weight_decay,
                                step, gcoef, grad_mul, a.c, &ls))
    return rc;
  a.gcoef = gcoef;
  a.grad_mul = grad_mul;
  a.state = nullptr;
  return adamw_issue<false>(a, ls, p, m, v, g, pout, counts, gdtype, odtype, stream);
}

int launch_adamw_segments_dyn_h16(int n, void *const *p, void *const *m, void *const *v, const void *const *g,
                                  void *const *pout, const size_t *counts, int gdtype, int odtype, const void *state,
                                  void *stream) {
  AdamwSegs a;
  std::vector<AdamwLaunch> ls;
  if (const int rc = adamw_dyn_args(n, p, m, v, g, pout, counts, gdtype, odtype, state, &ls)) return rc;
  a.gcoef = nullptr;
  a.grad_mul = 0.0;
  for (float &x : a.c) x = 0.0f;
  a.state = static_cast<const StepState *>(state);
  return adamw_issue<true>(a, ls, p, m, v, g, pout, counts, gdtype, odtype, stream);
}

// k_step_update: the loss-scale / step-count update of bine_step_update
// (bine_amd.h), one thread running step_update_rule (bine_internal.h) -- the
// statement the host twin compiles -- on the global norm k_sumsq_total left in
// device memory.
__global__ __launch_bounds__(64) void k_step_update(StepState *s, const double *norm2, bine_step_hyper h) {
  if (blockIdx.x == 0 && threadIdx.x == 0) step_update_rule(s, *norm2, h);
}

int launch_step_update_h16(void *state, const double *norm2, const bine_step_hyper *h, void *stream) {
  if (const int rc = step_update_args(state, norm2, h)) return rc;
  hipLaunchKernelGGL(k_step_update, dim3(1), dim3(1), 0, (hipStream_t)stream, static_cast<StepState *>(state), norm2,
                     *h);
  return status(hipGetLastError());
}

// ----------------------------------------------------------------------------
// FP8 quantization of a list of tensors with per-tensor scaling (bine_amd.h):
// k_amax_segs, k_fp8_scales and k_quant_segs (which also dequantizes).  Both segment
// kernels take TileTable's dispatch over plan_norm_launches' table of the WIDE
// side (float, float16 or bfloat16): a tile is kBlock * kScaleU 16-B aligned
// vectors, and a segment's first workgroup also takes the elements before the
// first and after the last vector.

// k_amax_segs: the largest magnitude pattern of each tensor.  A workgroup takes
// kAmaxTilesPerWg consecutive tiles of its segment (amax_launch_of).  A lane
// keeps the maximum of its elements' patterns without the sign bit IN THE
// ELEMENT'S OWN FORMAT -- widening is monotone on them, NaNs above infinity
// included -- and the workgroup's winner is widened once (widen_bits: exact,
// integer arithmetic, a NaN's payload shifted and not quieted).  Thread 0 then
// loads out[k], which the launcher zeroed in stream, and issues at most one
// atomic maximum on it: none where the winner is not above what it loaded.
template <typename T>
__device__ __forceinline__ uint32_t mag16(u32x4 v) {
  if constexpr (sizeof(T) == 4) {
    v &= 0x7fffffffu;
  } else {
    v = __builtin_elementwise_max(v & 0x7fffu, (v >> 16) & 0x7fffu);
  }
  const uint32_t a = v.x > v.y ? v.x : v.y, b = v.z > v.w ? v.z : v.w;
  return a > b ? a : b;
}
template <typename T>
__device__ __forceinline__ uint32_t mag1(T x) {
  uint_of<T> b;
  __builtin_memcpy(&b, &x, sizeof b);
  return (uint32_t)b & (sizeof(T) == 4 ? 0x7fffffffu : 0x7fffu);
}
template <typename T>
__device__ __forceinline__ uint32_t widen_bits(uint32_t m) {
  if constexpr (std::is_same_v<T, float>) return m;
  else if constexpr (std::is_same_v<T, BF16>) return m << 16;
  else {
    const uint32_t ex = m >> 10, man = m & 0x3ffu;
    if (ex == 0x1f) return 0x7f800000u | (man << 13);
    if (ex) return ((ex + 112) << 23) | (man << 13);
    if (!man) return 0;
    const int p = 31 - __builtin_clz(man);  // man * 2^-24 with its leading one at bit p
    return ((uint32_t)(p + 103) << 23) | ((man << (23 - p)) & 0x7fffffu);
  }
}
// the workgroup's maximum of one value per lane; valid in every thread
__device__ __forceinline__ uint32_t wg_max(uint32_t v, uint32_t *part) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = part[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; w++) s = part[w] > s ? part[w] : s;
  return s;
}

struct AmaxSegs {
  TileTable<kSegsPerLaunch> tab;
  uint32_t *out;
  uint16_t seg[kSegsPerLaunch];  // the caller's tensor per slot
  NormSeg s[kSegsPerLaunch];
};
static_assert(sizeof(AmaxSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

template <typename T>
__global__ __launch_bounds__(kBlock) void k_amax_segs(AmaxSegs a) {
  __shared__ uint32_t part[kBlock / 64];
  const auto [k, wt] = a.tab.find(blockIdx.x);
  const uint8_t *p = a.s[k].p;
  const size_t n = a.s[k].bytes;
  const size_t head = seg_head((uintptr_t)p, n), nvec = seg_nvec(n, head);
  uint32_t acc = 0;
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(p + head);
  // the workgroup's kAmaxTilesPerWg consecutive tiles, one after another
#pragma unroll 1
  for (uint32_t j = 0; j < kAmaxTilesPerWg; j++) {
    const size_t tile = (size_t)wt * kAmaxTilesPerWg + j;
    if (tile * kBlock * kScaleU >= nvec) break;  // workgroup-uniform: past the segment's last vector
    const size_t base = tile * kBlock * kScaleU + threadIdx.x;
    if (base + (kScaleU - 1) * (size_t)kBlock < nvec) {
      u32x4 x[kScaleU];
#pragma unroll
      for (int u = 0; u < kScaleU; u++) x[u] = vs[base + (size_t)u * kBlock];
#pragma unroll
      for (int u = 0; u < kScaleU; u++) {
        const uint32_t m = mag16<T>(x[u]);
        acc = m > acc ? m : acc;
      }
    } else {
#pragma unroll
      for (int u = 0; u < kScaleU; u++) {
        const size_t i = base + (size_t)u * kBlock;
        if (i < nvec) {
          const uint32_t m = mag16<T>(vs[i]);
          acc = m > acc ? m : acc;
        }
      }
    }
  }
  if (wt == 0) {  // head and tail elements of this segment
    const T *e = reinterpret_cast<const T *>(p);
    const size_t ne = n / sizeof(T), he = head / sizeof(T), te = (head + nvec * 16) / sizeof(T);
    for (size_t i = threadIdx.x; i < he; i += kBlock) acc = mag1<T>(e[i]) > acc ? mag1<T>(e[i]) : acc;
    for (size_t i = te + threadIdx.x; i < ne; i += kBlock) acc = mag1<T>(e[i]) > acc ? mag1<T>(e[i]) : acc;
  }
  acc = wg_max(acc, part);
  if (threadIdx.x == 0 && acc) {
    // out[k] only grows, so whatever this load sees is at most its current
    // value: a winner not above it cannot change the maximum and skips the
    // atomic.  Atomics on one address serialise (8,192 of them on a 256 MiB
    // tensor doubled the kernel's time); the load costs nothing
    // measurable (tools/amax_variants.hip).
    uint32_t *o = a.out + a.seg[k];
    const uint32_t w = widen_bits<T>(acc);
    if (w > __hip_atomic_load(o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(o, w);
  }
}

__global__ __launch_bounds__(kBlock) void k_amax_zero(int n, uint32_t *out) {
  const int k = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (k < n) out[k] = 0;
}

int launch_amax_segments_h16(const std::vector<AmaxLaunch> &ls, int n, const void *const *bufs, const size_t *counts,
                             int dtype, uint32_t *out, void *stream) {
  if (n == 0) return BINE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  // the zero fill the atomic maxima start from: a launch of its own, ahead in stream
  hipLaunchKernelGGL(k_amax_zero, dim3((unsigned)(n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, out);
  if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
  return with_adamw_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (const AmaxLaunch &L : ls) {
      AmaxSegs a;
      a.out = out;
      fill_segs(a, L, [&](int s) {
        return NormSeg{(uint8_t *)const_cast<void *>(bufs[L.seg[s]]), (uint64_t)(counts[L.seg[s]] * sizeof(T))};
      });
      for (int s = 0; s < kSegsPerLaunch; s++) a.seg[s] = s < L.nseg ? (uint16_t)L.seg[s] : 0;
      hipLaunchKernelGGL((k_amax_segs<T>), dim3(L.tile0[L.nseg]), dim3(kBlock), 0, st, a);
      if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    }
    return BINE_SUCCESS;
  });
}

// k_fp8_scales: thread k runs fp8_scale_rule (bine_internal.h) -- the statement
// the host twin compiles -- on amax[k]
__global__ __launch_bounds__(kBlock) void k_fp8_scales(int n, const uint32_t *amax, int fmt, float *scales) {
  const int k = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (k < n) fp8_scale_rule(amax[k], fmt, scales + k, scales + n + k);
}

int launch_fp8_scales_h16(int n, const uint32_t *amax, int fmt, float *scales, void *stream) {
  if (n == 0) return BINE_SUCCESS;
  hipLaunchKernelGGL(k_fp8_scales, dim3((unsigned)(n + kBlock - 1) / kBlock), dim3(kBlock), 0, (hipStream_t)stream, n,
                     amax, fmt, scales);
  return status(hipGetLastError());
}

// Four binary32 values as four FP8 bytes, element 0 lowest.  A NaN becomes
// 0x7F by its own select (the conversion sees 0.0 in its place, byte 0x00,
// and the select ORs the NaN byte in); everything else is clamped to +-FMAX,
// so the packed conversion never sees a value past the format's range and
// only has to round: nearest even, the format's subnormals kept, -0 kept.
template <int FMT>
__device__ __forceinline__ uint32_t quant4(float y0, float y1, float y2, float y3) {
  constexpr float kMax = FMT == BINE_FP8_E4M3 ? 448.0f : 57344.0f;
  uint32_t nan = 0;
  auto prep = [&](float y, int sh) {
    if (y != y) {
      nan |= 0x7fu << sh;
      return 0.0f;
    }
    return fminf(fmaxf(y, -kMax), kMax);
  };
  const float c0 = prep(y0, 0), c1 = prep(y1, 8), c2 = prep(y2, 16), c3 = prep(y3, 24);
  int w = 0;
  if constexpr (FMT == BINE_FP8_E4M3) {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c0, c1, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c2, c3, w, true);
  }
  return (uint32_t)w | nan;
}
template <typename T, int FMT>
__device__ __forceinline__ uint8_t quant1(T x, float s) {
  return (uint8_t)quant4<FMT>(adamw_widen<T>(x) * s, 0.0f, 0.0f, 0.0f);
}
// the bytes of one 16-B source vector: one word for float, two for the 16-bit types
template <typename T>
using q8_of = std::conditional_t<sizeof(T) == 4, uint32_t, u32x2>;
template <typename T, int FMT>
__device__ __forceinline__ q8_of<T> quant16(u32x4 v, float s) {
  if constexpr (sizeof(T) == 4) {
    float f[4];
    __builtin_memcpy(f, &v, 16);
    return quant4<FMT>(f[0] * s, f[1] * s, f[2] * s, f[3] * s);
  } else {
    const W8 w = widen16<T>(v);
    u32x2 r;
    r.x = quant4<FMT>(w.a.x * s, w.a.y * s, w.a.z * s, w.a.w * s);
    r.y = quant4<FMT>(w.b.x * s, w.b.y * s, w.b.z * s, w.b.w * s);
    return r;
  }
}

// the non-NaN byte b as the binary32 pattern of its value, exactly
template <int FMT>
__device__ __forceinline__ uint32_t fp8_decode_bits(uint32_t b) {
  constexpr int MB = FMT == BINE_FP8_E4M3 ? 3 : 2, bias = FMT == BINE_FP8_E4M3 ? 7 : 15;
  const uint32_t mag = b & 0x7fu, sgn = (b & 0x80u) << 24;
  if (FMT == BINE_FP8_E5M2 && mag == 0x7cu) return sgn | 0x7f800000u;
  if (mag >> MB) return sgn | ((mag << (23 - MB)) + ((uint32_t)(127 - bias) << 23));  // exponent and fraction, rebased
  const float f = (float)mag * (FMT == BINE_FP8_E4M3 ? 0x1p-9f : 0x1p-16f);  // subnormal: mag * 2^(1 - bias - MB)
  uint32_t r;
  __builtin_memcpy(&r, &f, 4);
  return sgn | r;
}
// byte b as an element of T (its pattern): narrow(decode(b) * inv); a NaN byte
// gives T's quiet NaN with the byte's sign
template <typename T, int FMT>
__device__ __forceinline__ uint_of<T> dequant1(uint32_t b, float inv) {
  const bool nan = FMT == BINE_FP8_E4M3 ? (b & 0x7fu) == 0x7fu : (b & 0x7fu) > 0x7cu;
  if (nan) {
    const uint32_t q = ((b & 0x80u) << 24) | 0x7fc00000u;
    if constexpr (std::is_same_v<T, float>) return q;
    else if constexpr (std::is_same_v<T, BF16>) return (uint16_t)(q >> 16);
    else return (uint16_t)(((b & 0x80u) << 8) | 0x7e00u);
  }
  const uint32_t d = fp8_decode_bits<FMT>(b);
  float f;
  __builtin_memcpy(&f, &d, 4);
  const T t = adamw_narrow<T>(f * inv);
  uint_of<T> r;
  __builtin_memcpy(&r, &t, sizeof r);
  return r;
}
template <typename T, int FMT>
__device__ __forceinline__ u32x4 dequant16(q8_of<T> b, float inv) {
  constexpr int V = 16 / (int)sizeof(T);
  uint32_t w[V / 4];
  __builtin_memcpy(w, &b, sizeof w);
  uint_of<T> e[V];
#pragma unroll
  for (int j = 0; j < V; j++) e[j] = dequant1<T, FMT>((w[j / 4] >> (8 * (j % 4))) & 0xffu, inv);
  u32x4 r;
  __builtin_memcpy(&r, e, 16);
  return r;
}

// One descriptor per slot: the wide buffer, the FP8 bytes, the element count.
// A slot whose byte side stands on a V-byte boundary wherever the wide side
// stands on a 16-B one (V = 16 / sizeof(T)) takes the vector body -- a lane
// handles one wide vector and its V bytes per access, all loads of a full tile
// issued before the first use, non-temporal loads of a full tile (the source is
// read last here) and non-temporal stores on every path; any other slot takes the element body (QuantSegs::elem,
// set by the host): the same operations through element and byte accesses.
struct QuantSeg {
  uint8_t *wide, *b8;
  uint64_t n;  // elements
};
struct QuantSegs {
  TileTable<kSegsPerLaunch> tab;
  uint64_t elem[(kSegsPerLaunch + 63) / 64];  // bit s: slot s takes the element body
  const float *scales;                        // per tensor; NULL: 1
  uint16_t seg[kSegsPerLaunch];               // the caller's tensor per slot
  QuantSeg s[kSegsPerLaunch];
};
static_assert(sizeof(QuantSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

// DEQ false: b8 = encode(wide * scale); true: wide = narrow(decode(b8) * scale)
template <typename T, int FMT, bool DEQ>
__global__ __launch_bounds__(kBlock) void k_quant_segs(QuantSegs a) {
  constexpr size_t V = 16 / sizeof(T);
  using BV = q8_of<T>;
  const auto [k, wt] = a.tab.find(blockIdx.x);
  T *wide = reinterpret_cast<T *>(a.s[k].wide);
  uint8_t *b8 = a.s[k].b8;
  const size_t n = a.s[k].n;
  // the split in elements: wide is aligned to its element, so the head is whole elements
  const size_t he = seg_head((uintptr_t)wide, sizeof(T) * n) / sizeof(T), nvec = (n - he) / V;
  const bool elem = (a.elem[k >> 6] >> (k & 63)) & 1;
  u32x4 *vw = reinterpret_cast<u32x4 *>(wide + he);
  BV *vb = reinterpret_cast<BV *>(b8 + he);
  const size_t base = (size_t)wt * kBlock * kScaleU + threadIdx.x;
  const bool full = !elem && ((size_t)wt + 1) * kBlock * kScaleU <= nvec;  // workgroup-uniform
  [[maybe_unused]] u32x4 xw[kScaleU];
  [[maybe_unused]] BV xb[kScaleU];
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if constexpr (DEQ) xb[u] = __builtin_nontemporal_load(vb + i);
      else xw[u] = __builtin_nontemporal_load(vw + i);
    }
  }
  const float s = a.scales ? a.scales[a.seg[k]] : 1.0f;
  auto one = [&](size_t i) {
    if constexpr (DEQ) {
      __builtin_nontemporal_store(dequant1<T, FMT>(b8[i], s), reinterpret_cast<uint_of<T> *>(wide) + i);
    } else {
      __builtin_nontemporal_store(quant1<T, FMT>(wide[i], s), b8 + i);
    }
  };
  if (wt == 0) {  // head and tail elements of this segment
    for (size_t i = threadIdx.x; i < he; i += kBlock) one(i);
    for (size_t i = he + nvec * V + threadIdx.x; i < n; i += kBlock) one(i);
  }
  if (full) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if constexpr (DEQ) __builtin_nontemporal_store(dequant16<T, FMT>(xb[u], s), vw + i);
      else __builtin_nontemporal_store(quant16<T, FMT>(xw[u], s), vb + i);
    }
  } else if (!elem) {
#pragma unroll
    for (int u = 0; u < kScaleU; u++) {
      const size_t i = base + (size_t)u * kBlock;
      if (i < nvec) {
        if constexpr (DEQ) __builtin_nontemporal_store(dequant16<T, FMT>(vb[i], s), vw + i);
        else __builtin_nontemporal_store(quant16<T, FMT>(vw[i], s), vb + i);
      }
    }
  } else {  // the tile's elements one by one
    const size_t lo = he + (size_t)wt * kBlock * kScaleU * V, end = he + nvec * V;
    const size_t hi = lo + (size_t)kBlock * kScaleU * V < end ? lo + (size_t)kBlock * kScaleU * V : end;
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) one(i);
  }
}

template <bool DEQ>
static int quant_issue(const std::vector<QuantLaunch> &ls, const void *const *wide, const void *const *b8,
                       const size_t *counts, int dtype, int fmt, const float *scales, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return with_adamw_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (const QuantLaunch &L : ls) {
      QuantSegs a;
      a.scales = scales;
      for (size_t w = 0; w < sizeof a.elem / sizeof a.elem[0]; w++) a.elem[w] = L.elem[w];
      fill_segs(a, L, [&](int s) {
        const int k = L.seg[s];
        return QuantSeg{(uint8_t *)const_cast<void *>(wide[k]), (uint8_t *)const_cast<void *>(b8[k]),
                        (uint64_t)counts[k]};
      });
      for (int s = 0; s < kSegsPerLaunch; s++) a.seg[s] = s < L.nseg ? (uint16_t)L.seg[s] : 0;
      const dim3 grid(L.tile0[L.nseg]), blk(kBlock);
      if (fmt == BINE_FP8_E4M3) hipLaunchKernelGGL((k_quant_segs<T, BINE_FP8_E4M3, DEQ>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((k_quant_segs<T, BINE_FP8_E5M2, DEQ>), grid, blk, 0, st, a);
      if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    }
    return BINE_SUCCESS;
  });
}

int launch_quant_segments_h16(const std::vector<QuantLaunch> &ls, const void *const *src, void *const *dst8,
                              const size_t *counts, int sdtype, int fmt, const float *scales, void *stream) {
  return quant_issue<false>(ls, src, dst8, counts, sdtype, fmt, scales, stream);
}

int launch_dequant_segments_h16(const std::vector<QuantLaunch> &ls, const void *const *src8, void *const *dst,
                                const size_t *counts, int ddtype, int fmt, const float *inv_scales, void *stream) {
  return quant_issue<true>(ls, dst, src8, counts, ddtype, fmt, inv_scales, stream);
}

// ----------------------------------------------------------------------------
// MX block-scaled quantization of a list of tensors (bine_amd.h): k_mx_segs,
// which also dequantizes.  TileTable's dispatch over plan_mx_launches' table of
// the WIDE side; here a tile is kBlock * kScaleU 16-B vectors counted from the
// segment's FIRST ELEMENT, as the 32-element blocks are, so a tile is whole
// blocks and a workgroup owns its tile's blocks, data bytes and scale bytes.
// No LDS, no atomics: a block lives in 8 (float) or 4 (16-bit) adjacent lanes
// of the vector body, in 32 adjacent lanes of the element body.

// the maximum of v over the 2^LOG adjacent lanes that hold one block, valid in
// each of them (LOG <= 5).  DPP within a row of 16: two quad permutations leave
// a quad agreeing, the half-row mirror then brings the other quad's value, the
// row mirror the other half's; the 32-lane step crosses rows by a shuffle.
template <int LOG>
__device__ __forceinline__ uint32_t mx_group_max(uint32_t v) {
  auto step = [&](int o) { v = (uint32_t)o > v ? (uint32_t)o : v; };
  if constexpr (LOG >= 1) step(__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  if constexpr (LOG >= 2) step(__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  if constexpr (LOG >= 3) step(__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));  // row_half_mirror
  if constexpr (LOG >= 4) step(__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));  // row_mirror
  if constexpr (LOG >= 5) step(__shfl_xor((int)v, 16, 64));
  return v;
}

// 2^(127 - S), the quantizer's factor (S <= 252: a normal number), and 2^(S -
// 127), the dequantizer's (S <= 254; at S = 0 the subnormal 2^-127)
__device__ __forceinline__ float mx_qfactor(uint32_t S) {
  const uint32_t b = (254u - S) << 23;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
__device__ __forceinline__ float mx_dfactor(uint32_t S) {
  const uint32_t b = S ? S << 23 : 0x00400000u;
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}

// y (never NaN here) as an E2M1 nibble: nearest with ties to the even code by
// counting the thresholds passed -- the midpoints of 0, 0.5, 1, 1.5, 2, 3, 4,
// 6, each closed on the side of its even neighbour; everything above 5 is 6,
// which is the clamp.  Plain comparisons, so the contract's bits by
// construction (DESIGN.md 6.10 has what v_cvt_scalef32_pk_fp4_f32 was found
// to do on the same inputs, tools/mx_variants.hip).
__device__ __forceinline__ uint32_t fp4_enc1(float y) {
  uint32_t b;
  __builtin_memcpy(&b, &y, 4);
  const float a = __builtin_fabsf(y);
  const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                     (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return c | ((b >> 28) & 8u);
}
// the nibble as the binary32 pattern of its value, exactly
__device__ __forceinline__ uint32_t fp4_decode_bits(uint32_t nib) {
  const uint32_t m = nib & 7u, sgn = (nib & 8u) << 28;
  if (m < 2) return sgn | (m ? 0x3f000000u : 0u);                // 0, 0.5 (the subnormal)
  return sgn | (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);  // 1.f * 2^(e - 1)
}

// the data bytes of one 16-B wide vector: FP8 one word for float and two for
// the 16-bit types; E2M1 half of that
template <typename T, int FMT>
using mxw_of = std::conditional_t<FMT != BINE_MX_E2M1, q8_of<T>,
                                  std::conditional_t<sizeof(T) == 4, uint16_t, uint32_t>>;

// one element: the byte (FP8) or the nibble (E2M1) of widen(x) * 2^(127 - S); S != 0xFF
template <typename T, int FMT>
__device__ __forceinline__ uint32_t mx_quant1(T x, uint32_t S) {
  const float y = adamw_widen<T>(x) * mx_qfactor(S);
  if constexpr (FMT == BINE_MX_E2M1) return fp4_enc1(y);
  else return quant4<FMT>(y, 0.0f, 0.0f, 0.0f) & 0xffu;
}
template <typename T, int FMT>
__device__ __forceinline__ mxw_of<T, FMT> mx_quant16(u32x4 v, uint32_t S) {
  constexpr int V = 16 / (int)sizeof(T);
  float y[V];
  const float f = mx_qfactor(S);
  if constexpr (sizeof(T) == 4) {
    __builtin_memcpy(y, &v, 16);
  } else {
    const W8 w = widen16<T>(v);
    __builtin_memcpy(y, &w.a, 16);
    __builtin_memcpy(y + 4, &w.b, 16);
  }
#pragma unroll
  for (int j = 0; j < V; j++) y[j] *= f;
  uint32_t w[V / 4] = {};
  if constexpr (FMT == BINE_MX_E2M1) {
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < V; j++) r |= fp4_enc1(y[j]) << (4 * j);
    return S == 0xffu ? (mxw_of<T, FMT>)0 : (mxw_of<T, FMT>)r;
  } else {
#pragma unroll
    for (int j = 0; j < V / 4; j++)
      w[j] = S == 0xffu ? 0u : quant4<FMT>(y[4 * j], y[4 * j + 1], y[4 * j + 2], y[4 * j + 3]);
    mxw_of<T, FMT> r;
    __builtin_memcpy(&r, w, sizeof r);
    return r;
  }
}

// data byte (nibble) b of a block with scale byte S as an element of T (its pattern)
template <typename T, int FMT>
__device__ __forceinline__ uint_of<T> mx_dequant1(uint32_t b, uint32_t S) {
  if (S == 0xffu) {
    if constexpr (std::is_same_v<T, float>) return 0x7fc00000u;
    else if constexpr (std::is_same_v<T, BF16>) return (uint16_t)0x7fc0u;
    else return (uint16_t)0x7e00u;
  }
  if constexpr (FMT == BINE_MX_E2M1) {
    const uint32_t d = fp4_decode_bits(b);
    float f;
    __builtin_memcpy(&f, &d, 4);
    const T t = adamw_narrow<T>(f * mx_dfactor(S));
    uint_of<T> r;
    __builtin_memcpy(&r, &t, sizeof r);
    return r;
  } else {
    return dequant1<T, FMT>(b, mx_dfactor(S));
  }
}
template <typename T, int FMT>
__device__ __forceinline__ u32x4 mx_dequant16(mxw_of<T, FMT> b, uint32_t S) {
  constexpr int V = 16 / (int)sizeof(T), BITS = FMT == BINE_MX_E2M1 ? 4 : 8;
  uint32_t w[2] = {};
  __builtin_memcpy(w, &b, sizeof b);
  uint_of<T> e[V];
#pragma unroll
  for (int j = 0; j < V; j++)
    e[j] = mx_dequant1<T, FMT>((w[j * BITS / 32] >> (j * BITS % 32)) & ((1u << BITS) - 1), S);
  u32x4 r;
  __builtin_memcpy(&r, e, 16);
  return r;
}

// One descriptor per slot: the wide buffer, the data bytes, the scale bytes,
// the element count.
struct MxSeg {
  uint8_t *wide, *d8, *sc;
  uint64_t n;  // elements
};
struct MxSegs {
  TileTable<kMxSegsPerLaunch> tab;
  uint64_t elem[(kMxSegsPerLaunch + 63) / 64];  // bit s: slot s takes the element body
  MxSeg s[kMxSegsPerLaunch];
};
static_assert(sizeof(MxSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");
static_assert(kCopyTileVecs == (uint64_t)kBlock * kScaleU, "plan_mx_launches' tile is this kernel's");

// DEQ false: (d8, sc) = quantize(wide); true: wide = dequantize(d8, sc)
template <typename T, int FMT, bool DEQ>
__global__ __launch_bounds__(kBlock) void k_mx_segs(MxSegs a) {
  constexpr size_t V = 16 / sizeof(T);        // elements of one vector
  constexpr int LOG = sizeof(T) == 4 ? 3 : 2;  // log2 of the lanes that hold one block (32 / V)
  constexpr size_t TV = (size_t)kBlock * kScaleU;
  using DW = mxw_of<T, FMT>;
  const auto [k, wt] = a.tab.find(blockIdx.x);
  T *wide = reinterpret_cast<T *>(a.s[k].wide);
  uint8_t *d8 = a.s[k].d8, *sc = a.s[k].sc;
  const size_t n = a.s[k].n;
  const bool elem = (a.elem[k >> 6] >> (k & 63)) & 1;
  // the tile's elements [lo, hi); the vector body takes its whole blocks [lo, vend)
  const size_t lo = (size_t)wt * TV * V;
  const size_t hi = lo + TV * V < n ? lo + TV * V : n;
  const size_t vend = elem ? lo : hi & ~(size_t)(kMxBlock - 1);
  if (vend > lo) {
    const size_t nv = (vend - lo) / V;  // a multiple of the lanes of a block
    u32x4 *vw = reinterpret_cast<u32x4 *>(wide) + lo / V;
    DW *vd = reinterpret_cast<DW *>(d8) + lo / V;
    uint8_t *vs = sc + lo / kMxBlock;
    const size_t t = threadIdx.x;
    if (nv == TV) {  // a full tile: every load issued before the first use
      if constexpr (DEQ) {
        DW xb[kScaleU];
        uint32_t S[kScaleU];
#pragma unroll
        for (int u = 0; u < kScaleU; u++) {
          xb[u] = __builtin_nontemporal_load(vd + t + (size_t)u * kBlock);
          S[u] = __builtin_nontemporal_load(vs + ((t + (size_t)u * kBlock) >> LOG));
        }
#pragma unroll
        for (int u = 0; u < kScaleU; u++)
          __builtin_nontemporal_store(mx_dequant16<T, FMT>(xb[u], S[u]), vw + t + (size_t)u * kBlock);
      } else {
        u32x4 xw[kScaleU];
#pragma unroll
        for (int u = 0; u < kScaleU; u++) xw[u] = __builtin_nontemporal_load(vw + t + (size_t)u * kBlock);
#pragma unroll
        for (int u = 0; u < kScaleU; u++) {
          const size_t i = t + (size_t)u * kBlock;
          const uint32_t S = mx_scale_rule(widen_bits<T>(mx_group_max<LOG>(mag16<T>(xw[u]))), FMT);
          __builtin_nontemporal_store(mx_quant16<T, FMT>(xw[u], S), vd + i);
          if ((t & ((1u << LOG) - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, vs + (i >> LOG));
        }
      }
    } else {
#pragma unroll 1
      for (int u = 0; u < kScaleU; u++) {
        const size_t i = t + (size_t)u * kBlock;
        const bool in = i < nv;  // the same in all lanes of a block
        if constexpr (DEQ) {
          if (in) __builtin_nontemporal_store(mx_dequant16<T, FMT>(vd[i], vs[i >> LOG]), vw + i);
        } else {
          // every lane takes part in the cross-lane maximum: the loads and the stores are guarded, not it
          u32x4 x = {0, 0, 0, 0};
          if (in) x = vw[i];
          const uint32_t S = mx_scale_rule(widen_bits<T>(mx_group_max<LOG>(mag16<T>(x))), FMT);
          if (in) {
            __builtin_nontemporal_store(mx_quant16<T, FMT>(x, S), vd + i);
            if ((t & ((1u << LOG) - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, vs + (i >> LOG));
          }
        }
      }
    }
  }
  // the element body: [vend, hi), one element per lane, 32 adjacent lanes a
  // block (vend is a block's first element and kBlock a multiple of 32); the
  // lanes of a block leave the loop together
  const uint_of<T> *wb = reinterpret_cast<const uint_of<T> *>(wide);
#pragma unroll 1
  for (size_t i = vend + threadIdx.x; (i & ~(size_t)(kMxBlock - 1)) < hi; i += kBlock) {
    const bool in = i < hi;
    if constexpr (DEQ) {
      if (in) {
        const uint32_t S = sc[i / kMxBlock];
        const uint32_t b = FMT == BINE_MX_E2M1 ? (d8[i >> 1] >> (4 * (i & 1))) & 15u : d8[i];
        __builtin_nontemporal_store(mx_dequant1<T, FMT>(b, S), reinterpret_cast<uint_of<T> *>(wide) + i);
      }
    } else {
      uint_of<T> xb = 0;
      if (in) xb = wb[i];
      const uint32_t m = (uint32_t)xb & (sizeof(T) == 4 ? 0x7fffffffu : 0x7fffu);
      const uint32_t S = mx_scale_rule(widen_bits<T>(mx_group_max<5>(m)), FMT);
      T x;
      __builtin_memcpy(&x, &xb, sizeof x);
      const uint32_t q = S == 0xffu ? 0u : mx_quant1<T, FMT>(x, S);  // a lane past the end: +0, code 0
      if constexpr (FMT == BINE_MX_E2M1) {
        const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q, 0xB1, 0xf, 0xf, false);  // lane ^ 1
        if (in && !(i & 1)) __builtin_nontemporal_store((uint8_t)(q | (other << 4)), d8 + (i >> 1));
      } else {
        if (in) __builtin_nontemporal_store((uint8_t)q, d8 + i);
      }
      if ((i & (kMxBlock - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, sc + i / kMxBlock);
    }
  }
}

template <bool DEQ>
static int mx_issue(const std::vector<MxLaunch> &ls, const void *const *wide, const void *const *d8,
                    const void *const *sc, const size_t *counts, int dtype, int fmt, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return with_adamw_dtype(dtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (const MxLaunch &L : ls) {
      MxSegs a;
      for (size_t w = 0; w < sizeof a.elem / sizeof a.elem[0]; w++) a.elem[w] = L.elem[w];
      fill_segs(a, L, [&](int s) {
        const int k = L.seg[s];
        return MxSeg{(uint8_t *)const_cast<void *>(wide[k]), (uint8_t *)const_cast<void *>(d8[k]),
                     (uint8_t *)const_cast<void *>(sc[k]), (uint64_t)counts[k]};
      });
      const dim3 grid(L.tile0[L.nseg]), blk(kBlock);
      if (fmt == BINE_MX_E4M3) hipLaunchKernelGGL((k_mx_segs<T, BINE_MX_E4M3, DEQ>), grid, blk, 0, st, a);
      else if (fmt == BINE_MX_E5M2) hipLaunchKernelGGL((k_mx_segs<T, BINE_MX_E5M2, DEQ>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((k_mx_segs<T, BINE_MX_E2M1, DEQ>), grid, blk, 0, st, a);
      if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    }
    return BINE_SUCCESS;
  });
}

int launch_mx_quant_segments_h16(const std::vector<MxLaunch> &ls, const void *const *src, void *const *dst8,
                                 void *const *scl8, const size_t *counts, int sdtype, int fmt, void *stream) {
  return mx_issue<false>(ls, src, dst8, scl8, counts, sdtype, fmt, stream);
}

int launch_mx_dequant_segments_h16(const std::vector<MxLaunch> &ls, const void *const *src8, const void *const *scl8,
                                   void *const *dst, const size_t *counts, int ddtype, int fmt, void *stream) {
  return mx_issue<true>(ls, dst, src8, scl8, counts, ddtype, fmt, stream);
}

// ----------------------------------------------------------------------------
// The ordered binary32 sum of MX wire blocks (bine_mx_sum_segments, bine_amd.h):
// k_mx_sum_segs.  TileTable's dispatch over plan_mx_sum_launches' table of the
// DESTINATION, k_mx_segs' tiles (kBlock * kScaleU 16-B vectors of dst from the
// segment's first element: whole blocks; every count is a multiple of 32, so
// there is no short block).  Stream j of a slot is (packed + j * block) + its
// data and scale offsets.  No LDS, no atomics, no barrier.

// data code b of a block with scale byte S as binary32: decode(b) * 2^(S - 127),
// exact (the header); a NaN byte and S = 0xFF give a quiet NaN
template <int FMT>
__device__ __forceinline__ float mx_value(uint32_t b, uint32_t S) {
  const uint32_t r = mx_dequant1<float, FMT>(b, S);
  float f;
  __builtin_memcpy(&f, &r, 4);
  return f;
}
// T's positive quiet NaN: what mx_dequant1 gives for S = 0xFF
template <typename T>
__device__ __forceinline__ uint_of<T> mx_qnan() {
  return mx_dequant1<T, BINE_MX_E2M1>(0u, 0xffu);
}

struct MxSumSeg {
  uint8_t *dst;
  uint64_t doff, soff;  // the tensor's data and scale bytes in a block
  uint64_t n;           // elements, a multiple of 32
};
struct MxSumSegs {
  TileTable<kMxSegsPerLaunch> tab;
  uint64_t elem[(kMxSegsPerLaunch + 63) / 64];  // bit s: slot s takes the element body
  const uint8_t *packed;
  uint64_t block;  // bytes from one stream to the next
  uint32_t ns;     // streams, 1 .. kMxSumMaxStreams
  float scale;
  MxSumSeg s[kMxSegsPerLaunch];
};
static_assert(sizeof(MxSumSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");

template <typename T, int FMT>
__global__ __launch_bounds__(kBlock) void k_mx_sum_segs(MxSumSegs a) {
  constexpr size_t V = 16 / sizeof(T);  // elements of one dst vector
  constexpr size_t TV = (size_t)kBlock * kScaleU;
  constexpr int BITS = FMT == BINE_MX_E2M1 ? 4 : 8;
  constexpr int R = 128 / BITS;  // the elements of one 16-B data load: a lane's run
  static_assert(TV * V % ((size_t)kBlock * R) == 0, "a tile is whole steps of kBlock runs");
  const auto [k, wt] = a.tab.find(blockIdx.x);
  T *dst = reinterpret_cast<T *>(a.s[k].dst);
  const size_t n = a.s[k].n;
  const bool elem = (a.elem[k >> 6] >> (k & 63)) & 1;
  const uint8_t *dat = a.packed + a.s[k].doff, *scl = a.packed + a.s[k].soff;
  const size_t block = a.block;
  const uint32_t ns = a.ns;
  const float sc = a.scale;
  // the tile's elements [lo, hi): whole blocks
  const size_t lo = (size_t)wt * TV * V;
  const size_t hi = lo + TV * V < n ? lo + TV * V : n;
  if (!elem) {
#pragma unroll 1
    for (size_t e0 = lo + (size_t)threadIdx.x * R; e0 < hi; e0 += (size_t)kBlock * R) {  // e0 + R <= hi: hi % 32 == 0
      // every stream's load issued before the first use; j < ns is uniform
      u32x4 x[kMxSumMaxStreams];
      uint32_t S[kMxSumMaxStreams];
#pragma unroll
      for (int j = 0; j < kMxSumMaxStreams; j++)
        if ((uint32_t)j < ns) {
          x[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(dat + (size_t)j * block) + e0 / R);
          S[j] = __builtin_nontemporal_load(scl + (size_t)j * block + e0 / kMxBlock);
        }
      float acc[R];
      bool dead = false;  // the same in every lane of a block
#pragma unroll
      for (int j = 0; j < kMxSumMaxStreams; j++)
        if ((uint32_t)j < ns) {
          dead |= S[j] == 0xffu;
#pragma unroll
          for (int i = 0; i < R; i++) {
            const float d = mx_value<FMT>((x[j][i * BITS / 32] >> (i * BITS % 32)) & ((1u << BITS) - 1), S[j]);
            acc[i] = j ? acc[i] + d : d;
          }
        }
#pragma unroll
      for (int i = 0; i < R; i++) acc[i] = acc[i] * sc;
      u32x4 *vo = reinterpret_cast<u32x4 *>(dst + e0);
      const uint32_t q = mx_qnan<T>();
#pragma unroll
      for (int v = 0; v < R / (int)V; v++) {
        u32x4 r;
        if constexpr (sizeof(T) == 4) {
          __builtin_memcpy(&r, acc + 4 * v, 16);
          if (dead) r = u32x4{q, q, q, q};
        } else {
          W8 w;
          __builtin_memcpy(&w.a, acc + 8 * v, 16);
          __builtin_memcpy(&w.b, acc + 8 * v + 4, 16);
          r = narrow16<T>(w);
          if (dead) r = u32x4{q, q, q, q} * 0x10001u;
        }
        __builtin_nontemporal_store(r, vo + v);
      }
    }
  } else {  // one element per lane, byte loads
#pragma unroll 1
    for (size_t i = lo + threadIdx.x; i < hi; i += kBlock) {
      auto code = [&](uint32_t j) -> uint32_t {
        const uint8_t *d8 = dat + (size_t)j * block;
        return FMT == BINE_MX_E2M1 ? (d8[i >> 1] >> (4 * (i & 1))) & 15u : d8[i];
      };
      uint32_t S = scl[i / kMxBlock];
      bool dead = S == 0xffu;
      float acc = mx_value<FMT>(code(0), S);
#pragma unroll 1
      for (uint32_t j = 1; j < ns; j++) {
        S = scl[(size_t)j * block + i / kMxBlock];
        dead |= S == 0xffu;
        acc = acc + mx_value<FMT>(code(j), S);
      }
      const T t = adamw_narrow<T>(acc * sc);
      uint_of<T> r;
      __builtin_memcpy(&r, &t, sizeof r);
      __builtin_nontemporal_store(dead ? mx_qnan<T>() : r, reinterpret_cast<uint_of<T> *>(dst) + i);
    }
  }
}

int launch_mx_sum_segments_h16(const std::vector<MxLaunch> &ls, const std::vector<uint64_t> &off, int n, int nstreams,
                               const void *packed, size_t block_bytes, void *const *dst, const size_t *counts,
                               int ddtype, int fmt, float scale, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return with_adamw_dtype(ddtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (const MxLaunch &L : ls) {
      MxSumSegs a;
      for (size_t w = 0; w < sizeof a.elem / sizeof a.elem[0]; w++) a.elem[w] = L.elem[w];
      a.packed = (const uint8_t *)packed;
      a.block = block_bytes;
      a.ns = (uint32_t)nstreams;
      a.scale = scale;
      fill_segs(a, L, [&](int s) {
        const int k = L.seg[s];
        return MxSumSeg{(uint8_t *)dst[k], off[(size_t)k], off[(size_t)n + k], (uint64_t)counts[k]};
      });
      const dim3 grid(L.tile0[L.nseg]), blk(kBlock);
      if (fmt == BINE_MX_E4M3) hipLaunchKernelGGL((k_mx_sum_segs<T, BINE_MX_E4M3>), grid, blk, 0, st, a);
      else if (fmt == BINE_MX_E5M2) hipLaunchKernelGGL((k_mx_sum_segs<T, BINE_MX_E5M2>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((k_mx_sum_segs<T, BINE_MX_E2M1>), grid, blk, 0, st, a);
      if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    }
    return BINE_SUCCESS;
  });
}

// ----------------------------------------------------------------------------
// MX quantization with an error-feedback residual (bine_mx_quant_ef_segments,
// bine_amd.h): k_mx_ef_segs.  k_mx_segs' quantizing form over the same tile
// table of the source, with v = widen(x) + r in x's place and r = v - decode *
// 2^(S - 127) stored back: one pass, no LDS, no atomics, no barrier.  A block
// lives in 8 (float) or 4 (16-bit) adjacent lanes of the vector body, in 32 of
// the element body.  The codes come from mx_quant16<float> / mx_quant1<float>
// on v, so they are k_mx_segs' bytes for a float source v by construction.

// The value of a code the quantizer wrote, exactly.  FP8: the conversion
// instruction, which has no branch between the normal and the subnormal codes
// (fp8_decode_bits has one, two with dequant1's NaN test: DESIGN.md 6.11); the
// quantizer clamps, so no NaN or infinity code reaches it.  B: the byte of w.
template <int FMT, int B>
__device__ __forceinline__ float mx_ef_value(uint32_t w) {
  if constexpr (FMT == BINE_MX_E4M3) return __builtin_amdgcn_cvt_f32_fp8((int)w, B);
  else if constexpr (FMT == BINE_MX_E5M2) return __builtin_amdgcn_cvt_f32_bf8((int)w, B);
  else {
    const uint32_t d = fp4_decode_bits((w >> (4 * B)) & 15u);
    float f;
    __builtin_memcpy(&f, &d, 4);
    return f;
  }
}
// Four values v of one block under its scale byte S: their codes (four bytes,
// or four nibbles in the low half), and r = v - decode * 2^(S - 127) -- one
// multiplication, exact, and one subtraction; +0.0 under S = 0xFF.
template <int FMT>
__device__ __forceinline__ uint32_t mx_ef_quad(f32x4 v, uint32_t S, f32x4 &r) {
  u32x4 vb;
  __builtin_memcpy(&vb, &v, 16);
  const uint32_t w = (uint32_t)mx_quant16<float, FMT>(vb, S);
  const float f = mx_dfactor(S);
  const f32x4 d = {mx_ef_value<FMT, 0>(w) * f, mx_ef_value<FMT, 1>(w) * f, mx_ef_value<FMT, 2>(w) * f,
                   mx_ef_value<FMT, 3>(w) * f};
  const f32x4 e = v - d;
  r = S == 0xffu ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : e;
  return w;
}
__device__ __forceinline__ uint32_t mx_ef_mag(f32x4 v) {
  u32x4 b;
  __builtin_memcpy(&b, &v, 16);
  return mag16<float>(b);
}

// One descriptor per slot: the source, the residual, the data bytes, the scale
// bytes, the element count.
struct MxEfSeg {
  uint8_t *src, *res, *d8, *sc;
  uint64_t n;  // elements
};
template <int N>
struct MxEfSegsOf {
  TileTable<N> tab;
  uint64_t elem[(N + 63) / 64];  // bit s: slot s takes the element body
  MxEfSeg s[N];
};
using MxEfSegs = MxEfSegsOf<kMxEfSegsPerLaunch>;
static_assert(sizeof(MxEfSegs) <= 4096, "by-value kernel arguments: within HIP's 4 KiB");
static_assert(sizeof(MxEfSegsOf<kMxEfSegsPerLaunch + 1>) > 4096, "BINE_MX_EF_SEGS_PER_LAUNCH is the largest that fits");

template <typename T, int FMT>
__global__ __launch_bounds__(kBlock) void k_mx_ef_segs(MxEfSegs a) {
  constexpr size_t V = 16 / sizeof(T);         // elements of one source vector
  constexpr int RV = (int)(V / 4);             // residual vectors per source vector
  constexpr int LOG = sizeof(T) == 4 ? 3 : 2;  // log2 of the lanes that hold one block (32 / V)
  constexpr size_t TV = (size_t)kBlock * kScaleU;
  using DW = mxw_of<T, FMT>;
  const auto [k, wt] = a.tab.find(blockIdx.x);
  const T *src = reinterpret_cast<const T *>(a.s[k].src);
  float *res = reinterpret_cast<float *>(a.s[k].res);
  uint8_t *d8 = a.s[k].d8, *sc = a.s[k].sc;
  const size_t n = a.s[k].n;
  const bool elem = (a.elem[k >> 6] >> (k & 63)) & 1;
  // the tile's elements [lo, hi); the vector body takes its whole blocks [lo, vend)
  const size_t lo = (size_t)wt * TV * V;
  const size_t hi = lo + TV * V < n ? lo + TV * V : n;
  const size_t vend = elem ? lo : hi & ~(size_t)(kMxBlock - 1);
  // one source vector x and its residual vectors r: the data word, the new residuals, the scale byte
  auto one = [&](u32x4 x, f32x4 (&r)[RV], uint32_t &S) -> DW {
    f32x4 v[RV];
    if constexpr (sizeof(T) == 4) {
      __builtin_memcpy(&v[0], &x, 16);
      v[0] = v[0] + r[0];
    } else {
      const W8 w = widen16<T>(x);
      v[0] = w.a + r[0];
      v[1] = w.b + r[1];
    }
    uint32_t m = mx_ef_mag(v[0]);
    if constexpr (RV == 2) {
      const uint32_t m1 = mx_ef_mag(v[1]);
      m = m1 > m ? m1 : m;
    }
    S = mx_scale_rule(mx_group_max<LOG>(m), FMT);
    uint32_t w[RV];
#pragma unroll
    for (int j = 0; j < RV; j++) w[j] = mx_ef_quad<FMT>(v[j], S, r[j]);
    DW d;
    if constexpr (RV == 1) {
      d = (DW)w[0];
    } else if constexpr (FMT == BINE_MX_E2M1) {
      d = w[0] | (w[1] << 16);
    } else {
      d = DW{w[0], w[1]};
    }
    return d;
  };
  if (vend > lo) {
    const size_t nv = (vend - lo) / V;  // a multiple of the lanes of a block
    const u32x4 *vx = reinterpret_cast<const u32x4 *>(src) + lo / V;
    f32x4 *vr = reinterpret_cast<f32x4 *>(res) + lo / 4;
    DW *vd = reinterpret_cast<DW *>(d8) + lo / V;
    uint8_t *vs = sc + lo / kMxBlock;
    const size_t t = threadIdx.x;
    if (nv == TV) {  // a full tile: every load issued before the first use
      u32x4 x[kScaleU];
      f32x4 r[kScaleU][RV];
#pragma unroll
      for (int u = 0; u < kScaleU; u++) {
        const size_t i = t + (size_t)u * kBlock;
        x[u] = __builtin_nontemporal_load(vx + i);
#pragma unroll
        for (int j = 0; j < RV; j++) r[u][j] = __builtin_nontemporal_load(vr + i * RV + j);
      }
#pragma unroll
      for (int u = 0; u < kScaleU; u++) {
        const size_t i = t + (size_t)u * kBlock;
        uint32_t S;
        const DW d = one(x[u], r[u], S);
        __builtin_nontemporal_store(d, vd + i);
#pragma unroll
        for (int j = 0; j < RV; j++) __builtin_nontemporal_store(r[u][j], vr + i * RV + j);
        if ((t & ((1u << LOG) - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, vs + (i >> LOG));
      }
    } else {
#pragma unroll 1
      for (int u = 0; u < kScaleU; u++) {
        const size_t i = t + (size_t)u * kBlock;
        const bool in = i < nv;  // the same in all lanes of a block
        // every lane takes part in the cross-lane maximum: the loads and the stores are guarded, not it
        u32x4 x = {0, 0, 0, 0};
        f32x4 r[RV] = {};
        if (in) {
          x = vx[i];
#pragma unroll
          for (int j = 0; j < RV; j++) r[j] = vr[i * RV + j];
        }
        uint32_t S;
        const DW d = one(x, r, S);
        if (in) {
          __builtin_nontemporal_store(d, vd + i);
#pragma unroll
          for (int j = 0; j < RV; j++) __builtin_nontemporal_store(r[j], vr + i * RV + j);
          if ((t & ((1u << LOG) - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, vs + (i >> LOG));
        }
      }
    }
  }
  // the element body: [vend, hi), one element per lane, 32 adjacent lanes a
  // block (vend is a block's first element and kBlock a multiple of 32); the
  // lanes of a block leave the loop together
#pragma unroll 1
  for (size_t i = vend + threadIdx.x; (i & ~(size_t)(kMxBlock - 1)) < hi; i += kBlock) {
    const bool in = i < hi;
    float x = 0.0f, r = 0.0f;  // a lane past the end: v = +0, code 0
    if (in) {
      x = adamw_widen<T>(src[i]);
      r = res[i];
    }
    const float v = x + r;
    uint32_t vb;
    __builtin_memcpy(&vb, &v, 4);
    const uint32_t S = mx_scale_rule(mx_group_max<5>(vb & 0x7fffffffu), FMT);
    const uint32_t q = S == 0xffu ? 0u : mx_quant1<float, FMT>(v, S);
    const float e = v - mx_ef_value<FMT, 0>(q) * mx_dfactor(S);
    if constexpr (FMT == BINE_MX_E2M1) {
      const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q, 0xB1, 0xf, 0xf, false);  // lane ^ 1
      if (in && !(i & 1)) __builtin_nontemporal_store((uint8_t)(q | (other << 4)), d8 + (i >> 1));
    } else {
      if (in) __builtin_nontemporal_store((uint8_t)q, d8 + i);
    }
    if (in) __builtin_nontemporal_store(S == 0xffu ? 0.0f : e, res + i);
    if ((i & (kMxBlock - 1)) == 0) __builtin_nontemporal_store((uint8_t)S, sc + i / kMxBlock);
  }
}

int launch_mx_quant_ef_segments_h16(const std::vector<MxEfLaunch> &ls, const void *const *src, void *const *res,
                                    void *const *dst8, void *const *scl8, const size_t *counts, int sdtype, int fmt,
                                    void *stream) {
  hipStream_t st = (hipStream_t)stream;
  return with_adamw_dtype(sdtype, [&](auto tag) -> int {
    using T = typename decltype(tag)::type;
    for (const MxEfLaunch &L : ls) {
      MxEfSegs a;
      for (size_t w = 0; w < sizeof a.elem / sizeof a.elem[0]; w++) a.elem[w] = L.elem[w];
      fill_segs(a, L, [&](int s) {
        const int k = L.seg[s];
        return MxEfSeg{(uint8_t *)const_cast<void *>(src[k]), (uint8_t *)res[k], (uint8_t *)dst8[k],
                       (uint8_t *)scl8[k], (uint64_t)counts[k]};
      });
      const dim3 grid(L.tile0[L.nseg]), blk(kBlock);
      if (fmt == BINE_MX_E4M3) hipLaunchKernelGGL((k_mx_ef_segs<T, BINE_MX_E4M3>), grid, blk, 0, st, a);
      else if (fmt == BINE_MX_E5M2) hipLaunchKernelGGL((k_mx_ef_segs<T, BINE_MX_E5M2>), grid, blk, 0, st, a);
      else hipLaunchKernelGGL((k_mx_ef_segs<T, BINE_MX_E2M1>), grid, blk, 0, st, a);
      if (hipGetLastError() != hipSuccess) return BINE_ERR_HIP;
    }
    return BINE_SUCCESS;
  });
}
#endif  // BINE_OPSET == 2

#if BINE_OPSET == 0
// ----------------------------------------------------------------------------
// direct peer-memory transport (bine_comm_set_direct, direct.cpp): one launch
// moves up to kMaxDm messages, `wgs` workgroups each.  A message's sequence
// number is seq = base[peer] + j + 1, base = this rank's count of earlier
// sub-messages to (push) or from (pull) that peer, kept in its own inbox and
// advanced by the launch's last workgroup; slot = seq mod kSlots.  Everything
// else follows from (seq, peer): the slot in the receiver's inbox, the flag to
// wait on -- push: the receiver's ack of the slot's previous use (seq -
// kSlots); pull: the sender's ready mark for seq -- and the flag to publish.
// Thread 0 of each workgroup polls the wait flag with a time limit; the
// workgroup copies its grid-strided share; every workgroup counts itself in;
// the last one of the message resets the counter for the slot's next use and
// publishes seq in the peer's inbox.  A wait that times out marks the
// transport poisoned; every later launch then exits at once, so no wait
// outlives the time limit.  No host-side state: launches can be captured and
// replayed.
//
// Memory protocol (round 4).  Bytes stored into a peer's inbox slot are
// written THROUGH to memory (global_store_dwordx4 ... sc0 sc1 nt: system
// coherent, so no L2 keeps them dirty); a workgroup waits for its stores'
// acknowledgements (vmcnt 0) before it counts itself in with a RELAXED
// system-scope atomic, and the last arriver publishes the flag with a relaxed
// system-scope store -- the flag is issued after every byte of the message
// was acknowledged.  No L2 write-back anywhere: round 3 released every
// workgroup's stores with buffer_wbl2 sc0 sc1, and those write-backs
// serialise -- a 16 MiB message by 512 workgroups took 47 us with them and
// 9.4 us written through (5.9 us with no protocol at all;
// profiles/r4_fence_probe.txt).  A reader polls with relaxed system-scope
// loads; once the flag is seen, its thread 0 invalidates once (the acquire
// fence: buffer_inv sc0 sc1, waited for) before the workgroup barrier -- the
// invalidation is of the CU's L1 and the XCD's L2, shared by every wave of
// the workgroup -- and the waves then read the slot with ordinary
// non-temporal loads.

__device__ __forceinline__ uint64_t ld_rlx_sys(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// thread 0 of a reader, after it saw the flag: one system-scope acquire
// (invalidation), completed before the workgroup barrier that follows
__device__ __forceinline__ void acquire_once() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
  vm_wait();
}
// the end of a workgroup's share of a message: its stores acknowledged, then
// counted in (relaxed); true on the message's last arriver (thread 0 only)
__device__ __forceinline__ bool count_in(uint32_t *cnt, uint32_t nwg) {
  vm_wait();
  __syncthreads();
  if (threadIdx.x != 0) return false;
  const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (old + 1 != nwg) return false;
  __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the slot's next use: a later launch
  return true;
}
__device__ __forceinline__ void publish(uint64_t *flag, uint64_t seq) {
  __hip_atomic_store(flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// diagnostics (BINE_DIRECT_STAMPS, DmArgs::stamps): thread 0 of a workgroup
// appends its (entry, wait done, copy done) wall_clock64 stamps
__device__ __forceinline__ void dm_stamp(uint64_t *st, uint32_t serial, int kind, int msg, int wg, uint64_t t0,
                                         uint64_t t1, uint64_t t2) {
  if (!st) return;
  const uint64_t i = __hip_atomic_fetch_add(st, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (i >= st[1]) return;
  uint64_t *r = st + dm::kStampHdr + i * dm::kStampWords;
  r[0] = (uint64_t)serial << 32 | (uint64_t)kind << 24 | (uint64_t)(msg & 255) << 16 | (uint64_t)(wg & 0xffff);
  r[1] = t0;
  r[2] = t1;
  r[3] = t2;
}

// A wait that timed out: poison the transport -- the
// inbox word every later launch checks and the mapped host word the host
// reads -- and, for the first waiter of this rank to time out (the one whose
// exchange flips the inbox word), leave what it waited for in the host words
// (dm::TimeoutRecord, read by DirectState::describe): which kernel and phase,
// the peer, the slot, the sequence number wanted and the flag value last
// seen, the launch's serial, the workgroup and how long it waited.  Only
// that waiter sets the host word, after its record (release), so a host that
// sees the word set sees the record (a later waiter setting the word could
// let the host see it before the first one's record had landed).
__device__ __noinline__ void dm_time_out(uint32_t *poison, uint32_t *host, uint32_t kind, uint32_t phase, int rank,
                                         int peer, uint64_t slot, uint64_t want, uint64_t seen, uint32_t serial,
                                         uint64_t waited) {
  const uint32_t was = __hip_atomic_exchange(poison, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (!host) return;
  if (was == 0) {
    uint64_t *h = reinterpret_cast<uint64_t *>(host);
    const uint64_t v[dm::kRecWords] = {(uint64_t)kind << 8 | phase,
                                       (uint64_t)(uint32_t)rank,
                                       (uint64_t)(uint32_t)peer,
                                       slot,
                                       want,
                                       seen,
                                       serial,
                                       (uint64_t)blockIdx.x << 16 | threadIdx.x,
                                       waited};
#pragma unroll
    for (int i = 0; i < dm::kRecWords; i++)
      __hip_atomic_store(h + dm::kRecFirst + i, v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// one workgroup's share of message mi (workgroup wi of a.wgs): wait, copy,
// release, count in; the last workgroup of the message publishes.  false: the
// transport is poisoned (the workgroup must leave the launch at once)
__device__ __forceinline__ bool dm_copy_msg(const DmArgs &a, int mi, int wi, int nwg) {
  using namespace dm;
  const DmMsg &m = a.m[mi];
  uint8_t *own = a.own;
  uint32_t *poison = reinterpret_cast<uint32_t *>(own + kPoisonOff);
  uint64_t *base = reinterpret_cast<uint64_t *>(own + (m.push ? kBaseSendOff : kBaseRecvOff)) + m.peer;
  const uint64_t seq = __hip_atomic_load(base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint64_t)m.j + 1;
  const size_t k = (size_t)(seq % kSlots);
  uint8_t *remote = reinterpret_cast<uint8_t *const *>(own + kPeerTabOff)[m.peer];
  const size_t data_off = kFlagsBytes;
  const uint8_t *src;
  uint8_t *dst;
  const uint64_t *wait_ptr;
  uint64_t wait_val;
  uint64_t *sig_ptr;
  uint32_t *cnt_ptr;
  if (m.push) {
    src = m.src;
    dst = remote + data_off + ((size_t)a.rank * kSlots + k) * a.slot;
    wait_ptr = seq > (uint64_t)kSlots ? reinterpret_cast<const uint64_t *>(own + kAckOff + ((size_t)m.peer * kSlots + k) * kFlagStride)
                                      : nullptr;
    wait_val = seq - kSlots;
    sig_ptr = reinterpret_cast<uint64_t *>(remote + kReadyOff + ((size_t)a.rank * kSlots + k) * kFlagStride);
    cnt_ptr = reinterpret_cast<uint32_t *>(own + kCntPushOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
  } else {
    src = own + data_off + ((size_t)m.peer * kSlots + k) * a.slot;
    dst = m.dst;
    wait_ptr = reinterpret_cast<const uint64_t *>(own + kReadyOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
    wait_val = seq;
    sig_ptr = reinterpret_cast<uint64_t *>(remote + kAckOff + ((size_t)a.rank * kSlots + k) * kFlagStride);
    cnt_ptr = reinterpret_cast<uint32_t *>(own + kCntPullOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
  }
  __shared__ int go;
  uint64_t t0 = 0, t1 = 0;
  if (threadIdx.x == 0) {
    if (a.stamps) t0 = wall_clock64();
    int ok = __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0;
    if (ok && wait_ptr) {
      const long long w0 = wall_clock64();
      uint64_t seen;
      while ((seen = ld_rlx_sys(wait_ptr)) < wait_val) {
        if (wall_clock64() - w0 > (long long)a.timeout_ticks) {
          dm_time_out(poison, a.poison_host, m.push ? dm::kWaitMovePush : dm::kWaitMovePull, 0, a.rank, m.peer, k,
                      wait_val, seen, a.serial, wall_clock64() - w0);
          ok = 0;
          break;
        }
        if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    // a pull reads what the peer wrote into our slot: one acquire; a push
    // only writes the slot the peer acknowledged (its reads were complete
    // before it counted in), nothing to acquire
    if (ok && !m.push) acquire_once();
    go = ok;
    if (a.stamps) t1 = wall_clock64();
  }
  __syncthreads();
  if (!go) return false;  // poisoned: the transport is dead, counters and bases no longer matter
  // grid-strided 16-B vectors (src / dst co-aligned mod 16: slots and plan
  // offsets are), bytes before the first boundary and after the last vector
  // by workgroup 0
  const size_t head = std::min<uint64_t>((16 - ((uintptr_t)dst & 15)) & 15, m.bytes);
  const size_t nvec = (m.bytes - head) / 16;
  if (wi == 0) {
    // a push's bytes into the slot written through too (system-scope byte
    // stores); a pull reads them after the acquire above
    auto put = [&](size_t i) {
      if (m.push) __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      else dst[i] = src[i];
    };
    for (size_t i = threadIdx.x; i < head; i += kBlock) put(i);
    for (size_t i = head + nvec * 16 + threadIdx.x; i < m.bytes; i += kBlock) put(i);
  }
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(src + head);
  u32x4 *vd = reinterpret_cast<u32x4 *>(dst + head);
  constexpr int U = 4;
  const size_t stride = (size_t)nwg * kBlock * U;
  if (m.push) {
    const __amdgpu_buffer_rsrc_t r = wt_rsrc(vd);  // (a push's head is empty: vd is the slot)
    for (size_t b0 = (size_t)wi * kBlock * U + threadIdx.x; b0 < nvec; b0 += stride) {
      u32x4 x[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t i = b0 + (size_t)u * kBlock;
        if (i < nvec) x[u] = __builtin_nontemporal_load(vs + i);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t i = b0 + (size_t)u * kBlock;
        if (i < nvec) st_wt(r, i, x[u]);
      }
    }
  } else {
    for (size_t b0 = (size_t)wi * kBlock * U + threadIdx.x; b0 < nvec; b0 += stride) {
      u32x4 x[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t i = b0 + (size_t)u * kBlock;
        if (i < nvec) x[u] = __builtin_nontemporal_load(vs + i);
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t i = b0 + (size_t)u * kBlock;
        if (i < nvec) __builtin_nontemporal_store(x[u], vd + i);
      }
    }
  }
  // stores acknowledged (written through) / slot reads complete, count in; the
  // last one of the message publishes
  const bool last = count_in(cnt_ptr, (uint32_t)nwg);
  if (threadIdx.x == 0 && a.stamps) dm_stamp(a.stamps, a.serial, m.push ? 0 : 1, mi, wi, t0, t1, wall_clock64());
  if (last) publish(sig_ptr, seq);
  return true;
}

// one workgroup's share of a push GROUP led by message mi (the same bytes to
// several peers, DmMsg::grp): each member's slot-reuse acknowledgement is
// awaited, the source is read once and stored into every member's slot, and
// every member is counted in and published exactly as a standalone push
__device__ __forceinline__ bool dm_mcast_msg(const DmArgs &a, int mi, int wi, int nwg) {
  using namespace dm;
  uint8_t *own = a.own;
  uint32_t *poison = reinterpret_cast<uint32_t *>(own + kPoisonOff);
  __shared__ u32x4 *dv[kMaxDm];
  __shared__ uint64_t dseq[kMaxDm];
  __shared__ int dmem[kMaxDm];
  __shared__ int nd, go;
  if (threadIdx.x == 0) {
    int ok = __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0;
    int n = 0;
    for (int j = 0; j < a.nmsg; j++) {
      const DmMsg &m = a.m[j];
      if (!m.push || m.grp != mi) continue;
      const uint64_t seq = __hip_atomic_load(reinterpret_cast<const uint64_t *>(own + kBaseSendOff) + m.peer,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint64_t)m.j + 1;
      const size_t k = (size_t)(seq % kSlots);
      uint8_t *remote = reinterpret_cast<uint8_t *const *>(own + kPeerTabOff)[m.peer];
      dv[n] = reinterpret_cast<u32x4 *>(remote + kFlagsBytes + ((size_t)a.rank * kSlots + k) * a.slot);
      dseq[n] = seq;
      dmem[n] = j;
      n++;
      if (ok && seq > (uint64_t)kSlots) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(own + kAckOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
        const long long t0 = wall_clock64();
        uint64_t seen;
        while ((seen = ld_rlx_sys(w)) < seq - kSlots) {
          if (wall_clock64() - t0 > (long long)a.timeout_ticks) {
            dm_time_out(poison, a.poison_host, dm::kWaitGroupPush, 0, a.rank, m.peer, k, seq - kSlots, seen, a.serial,
                        wall_clock64() - t0);
            ok = 0;
            break;
          }
          if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
            ok = 0;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
      }
    }
    nd = n;
    go = ok;
  }
  __syncthreads();
  if (!go) return false;  // (writes only into acknowledged slots: nothing to acquire)
  const DmMsg &L = a.m[mi];
  const uint8_t *src = L.src;
  const int n = nd;
  // every slot is 16-B aligned (a multiple of 4 KiB from the inbox base):
  // whole vectors from byte 0, the tail bytes by workgroup 0
  const size_t nvec = L.bytes / 16;
  if (wi == 0)
    for (int d = 0; d < n; d++)
      for (size_t i = nvec * 16 + threadIdx.x; i < L.bytes; i += kBlock)
        __hip_atomic_store(reinterpret_cast<uint8_t *>(dv[d]) + i, src[i], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  const u32x4 *vs = reinterpret_cast<const u32x4 *>(src);
  constexpr int U = 4;
  const size_t stride = (size_t)nwg * kBlock * U;
  for (size_t b0 = (size_t)wi * kBlock * U + threadIdx.x; b0 < nvec; b0 += stride) {
    u32x4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const size_t i = b0 + (size_t)u * kBlock;
      if (i < nvec) x[u] = __builtin_nontemporal_load(vs + i);
    }
    for (int d = 0; d < n; d++) {
      const __amdgpu_buffer_rsrc_t r = wt_rsrc(dv[d]);
#pragma unroll
      for (int u = 0; u < U; u++) {
        const size_t i = b0 + (size_t)u * kBlock;
        if (i < nvec) st_wt(r, i, x[u]);
      }
    }
  }
  vm_wait();  // every member's bytes acknowledged (written through)
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int d = 0; d < n; d++) {
      const DmMsg &m = a.m[dmem[d]];
      const size_t k = (size_t)(dseq[d] % kSlots);
      uint32_t *cnt = reinterpret_cast<uint32_t *>(own + kCntPushOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
      const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (old + 1 == (uint32_t)nwg) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint8_t *remote = reinterpret_cast<uint8_t *const *>(own + kPeerTabOff)[m.peer];
        publish(reinterpret_cast<uint64_t *>(remote + kReadyOff + ((size_t)a.rank * kSlots + k) * kFlagStride),
                dseq[d]);
      }
    }
  }
  return true;
}

// copy workgroup b of the launch: the entry of DmArgs::cidx it belongs to
// (entry c has cwgs[c] workgroups: wgs for a message alone, wgs x members for
// a push group, so a group keeps the parallelism of its members), then its
// message alone or the group it leads
__device__ __forceinline__ bool dm_copy_wg(const DmArgs &a, unsigned b) {
  int c = 0;
  unsigned start = 0;
  while (c + 1 < a.ncopy && b >= start + (unsigned)a.cwgs[c]) start += (unsigned)a.cwgs[c++];
  const int mi = a.cidx[c], wi = (int)(b - start), nwg = a.cwgs[c];
  return a.m[mi].push && a.m[mi].grp == mi ? dm_mcast_msg(a, mi, wi, nwg) : dm_copy_msg(a, mi, wi, nwg);
}

// thread 0, after its workgroup's share of the launch: the last workgroup of
// the launch advances the sequence bases of every message (every workgroup has
// read them; the next launch is stream-ordered after this one)
__device__ __forceinline__ void dm_launch_done(const DmArgs &a) {
  using namespace dm;
  if (threadIdx.x != 0) return;
  uint8_t *own = a.own;
  uint32_t *lc = reinterpret_cast<uint32_t *>(own + kLaunchCntOff);
  // relaxed: every workgroup read its bases before it got here (the values
  // fed its addresses), and the next launch follows in stream order
  const uint32_t ol = __hip_atomic_fetch_add(lc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ol + 1 == gridDim.x) {
    __hip_atomic_store(lc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = 0; i < a.nmsg; i++) {
      uint64_t *bp = reinterpret_cast<uint64_t *>(own + (a.m[i].push ? kBaseSendOff : kBaseRecvOff)) + a.m[i].peer;
      __hip_atomic_store(bp, __hip_atomic_load(bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_dm_move(DmArgs a) {
  if (!dm_copy_wg(a, blockIdx.x)) return;
  dm_launch_done(a);
}

// every message: in range; copied by its own workgroups (cidx, each once),
// carried by its group's leader (a push with the leader's bytes and source),
// or -- tree launches -- a leaf; false otherwise
static bool dm_args_ok(const DmArgs &a, bool leaves_ok) {
  if (a.nmsg <= 0 || a.nmsg > kMaxDm || a.wgs < 1 || !a.own || !a.slot || a.ncopy < 0 || a.ncopy > a.nmsg)
    return false;
  uint64_t seen = 0;
  int ncw = 0;
  for (int c = 0; c < a.ncopy; c++) {
    const int i = a.cidx[c];
    if (i < 0 || i >= a.nmsg || (seen >> i & 1) || a.m[i].leaf >= 0 || (a.m[i].grp >= 0 && a.m[i].grp != i) ||
        a.cwgs[c] < 1 || a.cwgs[c] > 1 << 16)
      return false;
    seen |= 1ull << i;
    ncw += a.cwgs[c];
  }
  if (ncw != a.ncw) return false;
  for (int i = 0; i < a.nmsg; i++) {
    const DmMsg &m = a.m[i];
    if (m.peer < 0 || m.peer >= dm::kMaxPeers || m.j < 0 || m.j >= dm::kSlots || m.bytes > a.slot) return false;
    if (m.grp >= 0) {
      if (!m.push || m.grp >= a.nmsg || !(seen >> m.grp & 1) || a.m[m.grp].grp != m.grp ||
          a.m[m.grp].src != m.src || a.m[m.grp].bytes != m.bytes)
        return false;
    } else if (!(seen >> i & 1) && !(leaves_ok && m.leaf >= 0)) {
      return false;
    }
  }
  return true;
}

// blocks per CU a direct-transport launch leaves free (dm_residency_cap)
static int dm_margin() {
  static const int m = [] {
    const char *e = getenv("BINE_DIRECT_RESIDENCY_MARGIN");
    return e && *e ? std::max(0, atoi(e)) : 1;
  }();
  return m;
}

// Workgroup slots one direct-transport launch may take on the current device
// (bine_internal.h dm_fit_residency, dm_residency_cap): CUs x (resident blocks
// per CU of kernel `k` (the occupancy API: registers, LDS, wave slots) -
// margin) / share; 0 if unknown.  Both factors are queried once per kernel
// and device.
static int dm_cap(const void *k, int share) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, std::pair<int, int>> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find({k, dev});
  if (it == cache.end()) {
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k, kBlock, 0) != hipSuccess) {
      (void)hipGetLastError();
      cus = per = 0;
    }
    it = cache.emplace(std::make_pair(k, dev), std::make_pair(cus, per)).first;
  }
  return dm_residency_cap(it->second.first, it->second.second, dm_margin(), share);
}

int launch_dm_move(const DmArgs &a0, void *stream) {
  if (a0.nmsg <= 0) return BINE_SUCCESS;
  if (!dm_args_ok(a0, false)) return BINE_ERR_ARG;
  DmArgs a = a0;
  if (dm_fit_residency(a.cwgs, a.ncopy, nullptr, dm_cap((const void *)k_dm_move, a.share)) > 0) {
    a.ncw = 0;
    for (int c = 0; c < a.ncopy; c++) a.ncw += a.cwgs[c];
  }
  hipLaunchKernelGGL(k_dm_move, dim3((unsigned)a.ncw), dim3(kBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP;
}

// k_dm_move_tree<T, OP, NL> (bine_internal.h DmTree): the copy messages as in
// k_dm_move, then `twgs` workgroups that evaluate the flat reduce-scatter's
// tree straight out of the leaf pulls' inbox slots
template <typename T, int OP, int NL>
__global__ __launch_bounds__(kBlock) void k_dm_move_tree(DmArgs a, DmTree t) {
  using namespace dm;
  const unsigned ncw = (unsigned)a.ncw;
  if (blockIdx.x < ncw) {
    if (!dm_copy_wg(a, blockIdx.x)) return;
    dm_launch_done(a);
    return;
  }
  uint8_t *own = a.own;
  uint32_t *poison = reinterpret_cast<uint32_t *>(own + kPoisonOff);
  // every leaf: its slot in our inbox, the sender's ready mark to wait for
  // -- polled side by side, lane j for leaf j in one loop (one flag round
  // trip, not one per leaf)
  const u32x4 *lp[NL];
  const uint64_t *wp = nullptr;
  uint64_t wseq = 0;
  int wpeer = -1;
  size_t wslot = 0;
  __shared__ int go;
  uint64_t t0 = 0, t1 = 0;
  if (threadIdx.x == 0) {
    if (a.stamps) t0 = wall_clock64();
    go = __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NL; j++) {
    if (j == t.pos) {
      lp[j] = reinterpret_cast<const u32x4 *>(t.own_leaf);
      continue;
    }
    const DmMsg &m = a.m[t.leaf_msg[j]];
    const uint64_t seq = __hip_atomic_load(reinterpret_cast<const uint64_t *>(own + kBaseRecvOff) + m.peer,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint64_t)m.j + 1;
    const size_t k = (size_t)(seq % kSlots);
    lp[j] = reinterpret_cast<const u32x4 *>(own + kFlagsBytes + ((size_t)m.peer * kSlots + k) * a.slot);
    if ((int)threadIdx.x == j) {
      wp = reinterpret_cast<const uint64_t *>(own + kReadyOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
      wseq = seq;
      wpeer = m.peer;
      wslot = k;
    }
  }
  if (wp && go) {
    const long long tw = wall_clock64();
    uint64_t seen;
    while ((seen = ld_rlx_sys(wp)) < wseq) {
      if (wall_clock64() - tw > (long long)a.timeout_ticks) {
        dm_time_out(poison, a.poison_host, dm::kWaitTreeLeaf, 0, a.rank, wpeer, wslot, wseq, seen, a.serial,
                    wall_clock64() - tw);
        go = 0;
        break;
      }
      if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
        go = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  __syncthreads();  // every leaf's poll has completed
  if (threadIdx.x == 0) {
    if (go) acquire_once();  // every leaf's mark seen: what the senders wrote before it
    if (a.stamps) t1 = wall_clock64();
  }
  __syncthreads();
  if (!go) return;
  // the tree over this workgroup's tiles (k_reduce_tree's tile body).  Fewer
  // vectors in flight per lane than k_reduce_tree: the copy workgroups of the
  // launch get this kernel's register allocation too
  constexpr int U = NL <= 4 ? 4 : NL == 8 ? 2 : 1;
  const int tw = (int)(blockIdx.x - ncw);
  u32x4 *vo = reinterpret_cast<u32x4 *>(t.out);
  const size_t tile = (size_t)kBlock * U, ntiles = (t.nvec + tile - 1) / tile;
  for (size_t ti = (size_t)tw; ti < ntiles; ti += (size_t)t.twgs) {
    const size_t b = ti * tile + threadIdx.x;
    if ((ti + 1) * tile <= t.nvec) tree_tile<T, OP, NL, U, false>(lp, vo, b, t.nvec, t.swap);
    else tree_tile<T, OP, NL, U, true>(lp, vo, b, t.nvec, t.swap);
  }
  // every leaf slice read (loads complete): count in per leaf; the last tree
  // workgroup of a leaf acknowledges its slot to the sender (as a pull's last
  // workgroup does)
  vm_wait();
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.stamps) dm_stamp(a.stamps, a.serial, 2, 255, tw, t0, t1, wall_clock64());
#pragma unroll
    for (int j = 0; j < NL; j++) {
      if (j == t.pos) continue;
      const DmMsg &m = a.m[t.leaf_msg[j]];
      const uint64_t seq = __hip_atomic_load(reinterpret_cast<const uint64_t *>(own + kBaseRecvOff) + m.peer,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint64_t)m.j + 1;
      const size_t k = (size_t)(seq % kSlots);
      uint32_t *cnt = reinterpret_cast<uint32_t *>(own + kCntPullOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
      const uint32_t old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if (old + 1 == (uint32_t)t.twgs) {
        __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint8_t *remote = reinterpret_cast<uint8_t *const *>(own + kPeerTabOff)[m.peer];
        publish(reinterpret_cast<uint64_t *>(remote + kAckOff + ((size_t)a.rank * kSlots + k) * kFlagStride), seq);
      }
    }
  }
  dm_launch_done(a);
}

// The element types the direct transport's in-launch reductions
// (k_dm_move_tree, k_dm_fused) are instantiated for, with SUM / PROD / MAX /
// MIN: the one list behind dm_fused_supported, the two launchers and
// dm_launch_cap.
template <typename T>
constexpr bool kDmT = std::is_same_v<T, float> || std::is_same_v<T, double> || std::is_same_v<T, int32_t> ||
                      std::is_same_v<T, int64_t> || std::is_same_v<T, uint32_t> || std::is_same_v<T, uint64_t>;

// with_dtype restricted to those types; BINE_ERR_UNSUPPORTED for the rest
template <typename F>
static int with_dm_dtype(int dtype, F &&f) {
  return with_dtype(dtype, [&](auto tag) -> int {
    if constexpr (kDmT<typename decltype(tag)::type>) return f(tag);
    else return BINE_ERR_UNSUPPORTED;
  });
}

bool dm_fused_supported(int dtype, int op) {
  return op >= BINE_SUM && op <= BINE_MIN && with_dm_dtype(dtype, [](auto) { return BINE_SUCCESS; }) == BINE_SUCCESS;
}

bool dm_tree_supported(int dtype, int op, int nl) {
  return dm_fused_supported(dtype, op) && with_nl(nl, [](auto) { return true; }, false);
}

template <typename T, int OP>
static const void *dmt_kernel(int nl) {
  return with_nl(nl, [](auto nlc) { return (const void *)k_dm_move_tree<T, OP, decltype(nlc)::value>; },
                 (const void *)nullptr);
}

template <typename T, int OP>
static hipError_t dmt_launch(const DmArgs &a0, const DmTree &t0, hipStream_t st) {
  return with_nl(t0.nl, [&](auto nlc) {
    constexpr int NL = decltype(nlc)::value;
    DmArgs a = a0;
    DmTree t = t0;
    if (dm_fit_residency(a.cwgs, a.ncopy, &t.twgs, dm_cap((const void *)k_dm_move_tree<T, OP, NL>, a.share)) > 0) {
      a.ncw = 0;
      for (int c = 0; c < a.ncopy; c++) a.ncw += a.cwgs[c];
    }
    hipLaunchKernelGGL((k_dm_move_tree<T, OP, NL>), dim3((unsigned)(a.ncw + t.twgs)), dim3(kBlock), 0, st, a, t);
    return hipGetLastError();
  });
}

int launch_dm_move_tree(const DmArgs &a, const DmTree &t, int dtype, int op, void *stream) {
  if (!dm_tree_supported(dtype, op, t.nl)) return BINE_ERR_UNSUPPORTED;
  if (!dm_args_ok(a, true) || t.twgs < 1 || t.pos < 0 || t.pos >= t.nl || !t.nvec || t.nvec * 16 > a.slot ||
      !t.out || !t.own_leaf || ((uintptr_t)t.out & 15) || ((uintptr_t)t.own_leaf & 15))
    return BINE_ERR_ARG;
  // every leaf position but pos once, by a leaf pull of nvec vectors; no other leaves
  uint64_t seen = 0;
  int nleaf = 0;
  for (int i = 0; i < a.nmsg; i++) nleaf += a.m[i].leaf >= 0;
  if (nleaf != t.nl - 1) return BINE_ERR_ARG;
  for (int j = 0; j < t.nl; j++) {
    if (j == t.pos) continue;
    const int i = t.leaf_msg[j];
    if (i < 0 || i >= a.nmsg || (seen >> i & 1) || a.m[i].push || a.m[i].leaf != j || a.m[i].bytes != t.nvec * 16)
      return BINE_ERR_ARG;
    seen |= 1ull << i;
  }
  hipStream_t st = (hipStream_t)stream;
  return with_dm_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return status(with_op<T>(op, [&](auto opc) { return dmt_launch<T, decltype(opc)::value>(a, t, st); }));
  });
}

// ----------------------------------------------------------------------------
// k_dm_fused: a flat-form small collective in one launch (bine_internal.h
// DmFusedArgs).  Flags, counters, slots and sequence bases are k_dm_move's.

namespace dmf {
using namespace dm;

// where message m of this launch reads, writes, waits and publishes
struct Msg {
  const u32x4 *src;
  u32x4 *dst;
  const uint64_t *wait;  // nullptr: nothing to wait for
  uint64_t wait_val;
  uint64_t *sig;
  uint32_t *cnt;
  uint64_t seq, nvec;
  // this workgroup's slice flags (bine_internal.h dm::kSliceReadyOff; null
  // when the launch has more workgroups than the layout holds): the one it
  // may wait on instead of `wait`, the one it sets after its slice, and (a
  // push) this rank's record of the slot's previous use
  const uint64_t *swait;
  uint64_t *ssig;
  uint64_t *geom;
  int k;
};

// a slice flag's value: the sequence number and the setter's workgroup count
__device__ __forceinline__ uint64_t slice_val(uint64_t seq, int wgs) {
  return seq << kSliceWgsBits | (uint64_t)wgs;
}

__device__ __forceinline__ Msg resolve(const DmFusedArgs &a, const DmMsg &m) {
  Msg r;
  uint8_t *own = a.own;
  const uint64_t *base = reinterpret_cast<const uint64_t *>(own + (m.push ? kBaseSendOff : kBaseRecvOff)) + m.peer;
  r.seq = __hip_atomic_load(base, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (uint64_t)m.j + 1;
  const size_t k = (size_t)(r.seq % kSlots);
  r.k = (int)k;
  uint8_t *remote = reinterpret_cast<uint8_t *const *>(own + kPeerTabOff)[m.peer];
  r.nvec = m.bytes / 16;
  const bool sl = a.slices && a.wgs <= kSliceMax;
  const size_t w = blockIdx.x;
  if (m.push) {
    r.src = reinterpret_cast<const u32x4 *>(m.src);
    r.dst = reinterpret_cast<u32x4 *>(remote + kFlagsBytes + ((size_t)a.rank * kSlots + k) * a.slot);
    r.wait = r.seq > (uint64_t)kSlots
                 ? reinterpret_cast<const uint64_t *>(own + kAckOff + ((size_t)m.peer * kSlots + k) * kFlagStride)
                 : nullptr;
    r.wait_val = r.seq - kSlots;
    r.sig = reinterpret_cast<uint64_t *>(remote + kReadyOff + ((size_t)a.rank * kSlots + k) * kFlagStride);
    r.cnt = reinterpret_cast<uint32_t *>(own + kCntPushOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
    r.swait = sl ? reinterpret_cast<const uint64_t *>(own + kSliceAckOff + slice_off(w, (size_t)m.peer, k))
                 : nullptr;
    r.ssig = sl ? reinterpret_cast<uint64_t *>(remote + kSliceReadyOff + slice_off(w, (size_t)a.rank, k)) : nullptr;
    r.geom = reinterpret_cast<uint64_t *>(own + kGeomOff + ((size_t)m.peer * kSlots + k) * 16);
  } else {
    r.src = reinterpret_cast<const u32x4 *>(own + kFlagsBytes + ((size_t)m.peer * kSlots + k) * a.slot);
    r.dst = reinterpret_cast<u32x4 *>(m.dst);
    r.wait = reinterpret_cast<const uint64_t *>(own + kReadyOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
    r.wait_val = r.seq;
    r.sig = reinterpret_cast<uint64_t *>(remote + kAckOff + ((size_t)a.rank * kSlots + k) * kFlagStride);
    r.cnt = reinterpret_cast<uint32_t *>(own + kCntPullOff + ((size_t)m.peer * kSlots + k) * kFlagStride);
    r.swait = sl ? reinterpret_cast<const uint64_t *>(own + kSliceReadyOff + slice_off(w, (size_t)m.peer, k))
                 : nullptr;
    r.ssig = sl ? reinterpret_cast<uint64_t *>(remote + kSliceAckOff + slice_off(w, (size_t)a.rank, k)) : nullptr;
    r.geom = nullptr;
  }
  return r;
}

// whether this workgroup may go on with message m: the whole message's flag,
// or -- when both ends cut it with this launch's workgroup count -- the flag
// of its own slice.  A push's slice of the slot's previous use was acked by
// the receiver's workgroup w only for the bytes THAT message's cut gave it:
// usable when this rank's record says that use was a k_dm_fused push of the
// same vector count (same wgs: in the ack's value).  `seen` = the whole
// flag's last value (the time-out record's).
__device__ __forceinline__ bool flag_ok(const DmFusedArgs &a, const Msg &m, bool push, bool geom_ok, uint64_t *seen) {
  *seen = ld_rlx_sys(m.wait);
  if (*seen >= m.wait_val) return true;
  if (!m.swait || (push && !geom_ok)) return false;
  const uint64_t v = ld_rlx_sys(m.swait);
  return (v >> kSliceWgsBits) >= m.wait_val && (v & ((1u << kSliceWgsBits) - 1)) == (uint64_t)a.wgs;
}

// The waits and arrivals of a phase's messages run side by side, one thread
// per message: one flag round trip per phase instead of one per message
// (a small collective is a chain of such round trips).
//
// wait_all: thread t < n polls message first + t's flag (relaxed
// system-scope loads, bounded); after the barrier, when any of them is a
// ready mark (acq: its slot is read next), thread 0 acquires once -- every
// poll has completed before the barrier -- and a second barrier orders the
// workgroup's reads after it.  false: the transport is poisoned (now or
// earlier).
__device__ __forceinline__ bool wait_all(const DmFusedArgs &a, int first, int n, bool acq, uint32_t phase) {
  __shared__ int bad;
  uint32_t *poison = reinterpret_cast<uint32_t *>(a.own + kPoisonOff);
  if (threadIdx.x == 0) bad = __hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
  __syncthreads();
  if ((int)threadIdx.x < n && !bad) {
    const DmMsg &mm = a.m[first + threadIdx.x];
    const Msg m = resolve(a, mm);
    if (m.wait) {
      const long long t0 = wall_clock64();
      uint64_t seen;
      // a push's slice acks cover this push's slice only if the slot's
      // previous use was a k_dm_fused push of the same vector count
      const bool geom_ok = mm.push && m.swait && ld_rlx_sys(m.geom) == m.wait_val &&
                           ld_rlx_sys(m.geom + 1) == m.nvec;
      while (!flag_ok(a, m, mm.push, geom_ok, &seen)) {
        if (wall_clock64() - t0 > (long long)a.timeout_ticks) {
          dm_time_out(poison, a.poison_host, mm.push ? dm::kWaitFusedPush : dm::kWaitFusedPull, phase, a.rank,
                      mm.peer, m.seq % kSlots, m.wait_val, seen, a.serial, wall_clock64() - t0);
          bad = 1;
          break;
        }
        if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
          bad = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
    }
  }
  __syncthreads();
  const bool ok = !bad;
  if (threadIdx.x == 0 && ok && acq && n) acquire_once();
  __syncthreads();  // the reads after the acquire; `bad` is reused by the next wait
  return ok;
}

// arrive_all: the workgroup's shares of messages first .. first + n - 1 are
// done (stores acknowledged, reads complete); thread t counts in for message
// t, and the last workgroup of a message publishes its seq (k_dm_move's
// protocol)
__device__ __forceinline__ void arrive_all(const DmFusedArgs &a, int first, int n) {
  vm_wait();
  __syncthreads();
  if ((int)threadIdx.x < n) {
    const DmMsg &mm = a.m[first + threadIdx.x];
    const Msg m = resolve(a, mm);
    // this workgroup's slice is done: its flag (the peer's workgroup w may go on)
    if (m.ssig) publish(m.ssig, slice_val(m.seq, a.wgs));
    const uint32_t old = __hip_atomic_fetch_add(m.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (old + 1 == (uint32_t)a.wgs) {
      __hip_atomic_store(m.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the slot's next use
      if (mm.push) {  // the use this push made of the slot (read by the slot's next push, a later launch)
        __hip_atomic_store(m.geom, m.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(m.geom + 1, m.nvec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      publish(m.sig, m.seq);
    }
  }
  __syncthreads();  // every thread's resolve() before thread 0's launch-counter add (the kernel's end)
}

// this workgroup's slice of a message of n vectors
__device__ __forceinline__ void slice(uint64_t n, int wgs, uint64_t *lo, uint64_t *hi) {
  *lo = n * blockIdx.x / (uint64_t)wgs;
  *hi = n * (blockIdx.x + 1) / (uint64_t)wgs;
}

// a push writes the peer's slot through; a pull reads its own slot after
// the acquire of wait_all.  U vectors per lane in flight (all loads, then
// all stores): with one, every store waits for its own load and the slice
// streams at a fraction of HBM bandwidth.
__device__ __forceinline__ void copy_slice(const Msg &m, int wgs, bool push) {
  constexpr int U = 4;
  uint64_t lo, hi;
  slice(m.nvec, wgs, &lo, &hi);
  const __amdgpu_buffer_rsrc_t r = wt_rsrc(push ? m.dst : nullptr);
  for (uint64_t b = lo + threadIdx.x; b < hi; b += (uint64_t)kBlock * U) {
    u32x4 x[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t i = b + (uint64_t)u * kBlock;
      if (i < hi) x[u] = __builtin_nontemporal_load(m.src + i);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t i = b + (uint64_t)u * kBlock;
      if (i < hi) {
        if (push) st_wt(r, i, x[u]);
        else __builtin_nontemporal_store(x[u], m.dst + i);
      }
    }
  }
}

// this workgroup's slice [lo, hi) of a tree of NL leaves (own leaf at `pos`:
// plain loads; the received ones in the inbox slots: non-temporal), each
// result vector stored to `out` and pushed from registers into the nc
// allgather slots; U vectors of every leaf per lane in flight, U x NL <= 8
// (the registers of the kernel's other phases)
template <typename T, int OP, int NL>
__device__ __forceinline__ void tree_slice(const u32x4 *const *lp, int nl, int pos, unsigned swap, u32x4 *out,
                                           const __amdgpu_buffer_rsrc_t *cp, int nc, uint64_t lo, uint64_t hi) {
  constexpr int U = NL >= 8 ? 1 : 8 / NL;
  for (uint64_t b = lo + threadIdx.x; b < hi; b += (uint64_t)kBlock * U) {
    u32x4 v[U][NL];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t i = b + (uint64_t)u * kBlock;
      if (i < hi) {
#pragma unroll
        for (int j = 0; j < NL; j++) {
          if (j >= nl) continue;  // a tree of nl <= NL leaves (a non-power-of-two P's)
          if (j == pos) v[u][j] = lp[j][i];
          else v[u][j] = __builtin_nontemporal_load(lp[j] + i);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint64_t i = b + (uint64_t)u * kBlock;
      if (i >= hi) continue;
      int lvl = 0;
#pragma unroll
      for (int w = 1; w < NL; w <<= 1, lvl++)
#pragma unroll
        for (int j = 0; j < NL; j += 2 * w)
          if (j + w < nl) v[u][j] = comb16<T, OP>(v[u][j], v[u][j + w], (swap >> lvl) & 1);
      out[i] = v[u][0];
#pragma unroll
      for (int c = 0; c < kMaxFusedPeers; c++)
        if (c < nc) st_wt(cp[c], i, v[u][0]);
    }
  }
}
}  // namespace dmf

template <typename T, int OP>
__global__ __launch_bounds__(kBlock) void k_dm_fused(DmFusedArgs a) {
  using namespace dmf;
  const int nm = a.d0 + a.nd;
  const uint64_t t0 = a.stamps ? wall_clock64() : 0;
  // phase A: our blocks of every chunk into the peers' inboxes (each slot's
  // previous use acknowledged first)
  if (!wait_all(a, 0, a.na, false, 0)) return;
  const uint64_t t1 = a.stamps ? wall_clock64() : 0;
  // workgroup w starts at message w mod na and rotates: at any moment the
  // workgroups spread over every peer's link instead of all pushing to the
  // same peer first (on a node each peer is its own xGMI link)
  for (int k = 0; k < a.na; k++) {
    const int i = (int)((blockIdx.x + (unsigned)k) % (unsigned)a.na);
    copy_slice(resolve(a, a.m[i]), a.wgs, true);
  }
  arrive_all(a, 0, a.na);
  // phases B_c: the peers' blocks of chunk c, read in place in our inbox as
  // the tree's leaves; each result vector goes to `out` and, for the flat
  // allgather, straight from registers into every peer's slot -- whose
  // previous use must have been acknowledged first
  for (int ti = 0; ti < a.nt; ti++) {
    const DmFusedTree &t = a.t[ti];
    if (!wait_all(a, t.b0, t.nb + t.nc, t.nb > 0, 1 + ti)) return;
    const u32x4 *lp[kMaxLeaves];
#pragma unroll
    for (int j = 0; j < kMaxLeaves; j++)
      lp[j] = j >= a.nl ? nullptr
              : j == a.pos ? reinterpret_cast<const u32x4 *>(t.own_leaf)
                           : resolve(a, a.m[t.leaf[j]]).src;
    __amdgpu_buffer_rsrc_t cp[kMaxFusedPeers];
#pragma unroll
    for (int i = 0; i < kMaxFusedPeers; i++)
      if (i < t.nc) cp[i] = wt_rsrc(resolve(a, a.m[t.b0 + t.nb + i]).dst);
    u32x4 *out = reinterpret_cast<u32x4 *>(t.out);
    uint64_t lo, hi;
    slice(t.nvec, a.wgs, &lo, &hi);
    if (a.nl <= 2) tree_slice<T, OP, 2>(lp, a.nl, a.pos, a.swap, out, cp, t.nc, lo, hi);
    else if (a.nl <= 4) tree_slice<T, OP, 4>(lp, a.nl, a.pos, a.swap, out, cp, t.nc, lo, hi);
    else if (a.nl <= 8) tree_slice<T, OP, 8>(lp, a.nl, a.pos, a.swap, out, cp, t.nc, lo, hi);
    else tree_slice<T, OP, 16>(lp, a.nl, a.pos, a.swap, out, cp, t.nc, lo, hi);
    // every leaf slice is read (the senders may reuse their slots) and every
    // result slice is in the peers' inboxes
    arrive_all(a, t.b0, t.nb + t.nc);
  }
  // phase D: the peers' results out of our inbox
  if (!wait_all(a, a.d0, a.nd, true, 15)) return;
  for (int k = 0; k < a.nd; k++) {  // rotated as phase A (the slots lie in different HBM channels anyway)
    const int i = (int)((blockIdx.x + (unsigned)k) % (unsigned)a.nd);
    copy_slice(resolve(a, a.m[a.d0 + i]), a.wgs, false);
  }
  arrive_all(a, a.d0, a.nd);
  if (threadIdx.x == 0 && a.stamps) dm_stamp(a.stamps, a.serial, 4, 255, blockIdx.x, t0, t1, wall_clock64());
  // the launch's last workgroup advances the sequence bases (every workgroup
  // has read them: each resolve() happened before its launch-counter add)
  if (threadIdx.x == 0) {
    uint32_t *lc = reinterpret_cast<uint32_t *>(a.own + dm::kLaunchCntOff);
    const uint32_t ol = __hip_atomic_fetch_add(lc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ol + 1 == gridDim.x) {
      __hip_atomic_store(lc, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int i = 0; i < nm; i++) {
        uint64_t *bp = reinterpret_cast<uint64_t *>(a.own + (a.m[i].push ? dm::kBaseSendOff : dm::kBaseRecvOff)) +
                       a.m[i].peer;
        __hip_atomic_store(bp, __hip_atomic_load(bp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// CUs of the current device (0: unknown), queried once per device
static int dm_cus() {
  static std::mutex mu;
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
    (void)hipGetLastError();
    return 0;
  }
  std::lock_guard<std::mutex> g(mu);
  if (!cus[dev] && hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    cus[dev] = 0;
  }
  return cus[dev];
}

template <typename T, int OP>
static hipError_t fused_launch(const DmFusedArgs &a0, hipStream_t st) {
  DmFusedArgs a = a0;
  int w = a.wgs;
  dm_fit_residency(&w, 1, nullptr, dm_cap((const void *)k_dm_fused<T, OP>, a.share));
  // above one workgroup per CU, whole multiples of the CU count: every CU
  // carries the same share of every phase (C3 at P = 2 on one GPU: 256 and
  // 512 workgroups 0.41-0.42 ms, 320 / 384 / 640 0.47-0.54 ms)
  const int cus = dm_cus();
  if (cus > 0 && w > cus) w -= w % cus;
  a.wgs = w;
  hipLaunchKernelGGL((k_dm_fused<T, OP>), dim3((unsigned)a.wgs), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

int dm_fused_check(const DmFusedArgs &a, int dtype, int op) {
  if (!dm_fused_supported(dtype, op)) return BINE_ERR_UNSUPPORTED;
  const int nm = a.d0 + a.nd;
  if (a.wgs < 1 || !a.own || !a.slot || a.nl < 2 || a.nl > kMaxLeaves || a.pos < 0 || a.pos >= a.nl ||
      a.nt < 1 || a.nt > kMaxFusedTrees || a.na < 0 || a.nd < 0 || nm > kMaxFusedMsgs)
    return BINE_ERR_ARG;
  for (int i = 0; i < nm; i++) {
    const DmMsg &m = a.m[i];
    if (m.peer < 0 || m.peer >= dm::kMaxPeers || m.j < 0 || m.j >= dm::kSlots || m.bytes > a.slot ||
        m.bytes % 16 || ((uintptr_t)(m.push ? (const void *)m.src : (const void *)m.dst) & 15))
      return BINE_ERR_ARG;
  }
  // the layout: A pushes, then each tree's leaf pulls and result pushes, then D pulls
  int at = a.na;
  for (int i = 0; i < a.na; i++)
    if (!a.m[i].push) return BINE_ERR_ARG;
  for (int ti = 0; ti < a.nt; ti++) {
    const DmFusedTree &t = a.t[ti];
    if (t.b0 != at || t.nb != a.nl - 1 || t.nc < 0 || !t.nvec || !t.out || !t.own_leaf ||
        ((uintptr_t)t.out & 15) || ((uintptr_t)t.own_leaf & 15))
      return BINE_ERR_ARG;
    for (int i = t.b0; i < t.b0 + t.nb; i++)
      if (a.m[i].push || a.m[i].bytes != t.nvec * 16) return BINE_ERR_ARG;
    for (int i = t.b0 + t.nb; i < t.b0 + t.nb + t.nc; i++)
      if (!a.m[i].push || a.m[i].bytes != t.nvec * 16) return BINE_ERR_ARG;
    uint32_t seen = 0;
    for (int j = 0; j < a.nl; j++) {
      if (j == a.pos) continue;
      const int i = t.leaf[j];
      if (i < t.b0 || i >= t.b0 + t.nb || (seen >> (i - t.b0) & 1)) return BINE_ERR_ARG;
      seen |= 1u << (i - t.b0);
    }
    at += t.nb + t.nc;
  }
  if (a.d0 != at) return BINE_ERR_ARG;
  for (int i = a.d0; i < nm; i++)
    if (a.m[i].push) return BINE_ERR_ARG;
  return BINE_SUCCESS;
}

int launch_dm_fused(const DmFusedArgs &a, int dtype, int op, void *stream) {
  if (int rc = dm_fused_check(a, dtype, op)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return with_dm_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return status(with_op<T>(op, [&](auto opc) { return fused_launch<T, decltype(opc)::value>(a, st); }));
  });
}

// ----------------------------------------------------------------------------
// cross-GPU flag latency probe (bine_comm_direct_ping).
// One lane of one workgroup on each of two ranks plays ping-pong with the
// transport's own flag protocol -- a relaxed system-scope store of a sequence
// number into the peer's inbox, a relaxed system-scope poll (with the
// protocol's back-off) of the peer's answer in its own -- `iters` times in one
// launch, no kernel boundary in between.  Round trip 1 absorbs the two
// launches' skew; rounds 2 .. iters are timed with wall_clock64 on each side.
// A round trip is two one-way flag latencies: a k_dm_fused phase boundary
// costs one (pico_amd/model.py T_FLAG_US).  Timed out: the transport is
// poisoned like any other wait, *out = 0.
__global__ __launch_bounds__(64) void k_dm_ping(DmPingArgs a) {
  using namespace dm;
  if (threadIdx.x != 0) return;
  uint32_t *poison = reinterpret_cast<uint32_t *>(a.own + kPoisonOff);
  const uint64_t *mine = reinterpret_cast<const uint64_t *>(a.own + kPingOff + (size_t)a.peer * kFlagStride);
  uint8_t *remote = reinterpret_cast<uint8_t *const *>(a.own + kPeerTabOff)[a.peer];
  uint64_t *theirs = reinterpret_cast<uint64_t *>(remote + kPingOff + (size_t)a.rank * kFlagStride);
  if (__hip_atomic_load(poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) {
    __hip_atomic_store(a.out, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  uint64_t t0 = 0;
  for (int i = 1; i <= a.iters; i++) {
    if (i == 2) t0 = wall_clock64();
    const uint64_t s = a.base + (uint64_t)i;
    if (a.initiator) publish(theirs, s);
    const long long w0 = wall_clock64();
    uint64_t seen;
    while ((seen = ld_rlx_sys(mine)) < s) {
      if (wall_clock64() - w0 > (long long)a.timeout_ticks) {
        dm_time_out(poison, a.poison_host, kWaitPing, 0, a.rank, a.peer, 0, s, seen, a.serial, wall_clock64() - w0);
        __hip_atomic_store(a.out, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    if (!a.initiator) publish(theirs, s);
  }
  __hip_atomic_store(a.out, wall_clock64() - t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int launch_dm_ping(const DmPingArgs &a, void *stream) {
  if (a.iters < 2 || !a.own || !a.out || a.peer == a.rank) return BINE_ERR_ARG;
  hipLaunchKernelGGL(k_dm_ping, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? BINE_SUCCESS : BINE_ERR_HIP;
}

// ----------------------------------------------------------------------------
// pico_core input generator (glibc rand_r, LCG jump-ahead)
// ----------------------------------------------------------------------------

struct Affine { uint32_t m, c; };  // x -> m x + c (mod 2^32)

__host__ __device__ inline Affine compose(Affine f, Affine g) {  // f(g(x))
  return {f.m * g.m, f.m * g.c + f.c};
}
__host__ __device__ inline Affine lcg_pow(uint64_t k) {
  Affine r{1u, 0u}, p{1103515245u, 12345u};
  while (k) {
    if (k & 1) r = compose(p, r);
    p = compose(p, p);
    k >>= 1;
  }
  return r;
}
// one glibc rand_r() call (three LCG steps, 11+10+10 bits)
__device__ inline int32_t rand_r_step(uint32_t &s) {
  s = s * 1103515245u + 12345u;
  uint32_t r = (s >> 16) % 2048u;
  s = s * 1103515245u + 12345u;
  r = (r << 10) ^ ((s >> 16) % 1024u);
  s = s * 1103515245u + 12345u;
  r = (r << 10) ^ ((s >> 16) % 1024u);
  return (int32_t)r;
}

constexpr int kFillPer = 16;  // consecutive elements per lane

template <typename T, int DT>
__global__ __launch_bounds__(kBlock) void k_fill_pico(T *buf, size_t n, uint32_t seed) {
  constexpr int calls = (DT == BINE_INT64 || DT == BINE_UINT64) ? 2 : 1;
  const size_t first = ((size_t)blockIdx.x * kBlock + threadIdx.x) * kFillPer;
  if (first >= n) return;
  const Affine j = lcg_pow((uint64_t)first * 3u * calls);
  uint32_t s = j.m * seed + j.c;
  for (int k = 0; k < kFillPer && first + k < n; k++) {
    T v;
    if constexpr (DT == BINE_INT8) v = (T)((rand_r_step(s) % 256) - 128);
    else if constexpr (DT == BINE_UINT8) v = (T)(rand_r_step(s) % 256);
    else if constexpr (DT == BINE_INT16) v = (T)((rand_r_step(s) % 65536) - 32768);
    else if constexpr (DT == BINE_UINT16) v = (T)(rand_r_step(s) % 65536);
    else if constexpr (DT == BINE_INT32 || DT == BINE_UINT32) v = (T)rand_r_step(s);
    else if constexpr (DT == BINE_INT64 || DT == BINE_UINT64) {
      const int64_t hi = (int64_t)rand_r_step(s) << 32;
      v = (T)(hi | (int64_t)rand_r_step(s));
    } else if constexpr (DT == BINE_FLOAT) v = (float)rand_r_step(s) / (float)2147483647 * 100.0f;
    else v = (double)rand_r_step(s) / (double)2147483647 * 100.0;
    buf[first + k] = v;
  }
}

int launch_fill_pico(void *buf, size_t n, int dtype, uint32_t seed, void *stream) {
  if (n == 0) return BINE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t lanes = (n + kFillPer - 1) / kFillPer;
  const unsigned blocks = (unsigned)((lanes + kBlock - 1) / kBlock);
  return with_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((k_fill_pico<T, decltype(tag)::id>), dim3(blocks), dim3(kBlock), 0, st, (T *)buf, n, seed);
    return status(hipGetLastError());
  });
}

// ----------------------------------------------------------------------------
// order-independent checksum
// ----------------------------------------------------------------------------

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finalizer
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <typename U>
__global__ __launch_bounds__(kBlock) void k_checksum(const U *buf, size_t n, unsigned long long *out) {
  uint64_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
    acc += mix64((uint64_t)buf[i] + (uint64_t)i * 0x9E3779B97F4A7C15ull);
  // wave64 reduction (two 32-bit shuffles per step)
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)acc, off, 64);
    const uint32_t hi = __shfl_xor((uint32_t)(acc >> 32), off, 64);
    acc += ((uint64_t)hi << 32) | lo;
  }
  __shared__ uint64_t part[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0;
    for (int w = 0; w < kBlock / 64; w++) s += part[w];
    atomicAdd(out, (unsigned long long)s);
  }
}

int launch_checksum(const void *buf, size_t n, int dtype, uint64_t *host_out, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  unsigned long long *d = nullptr;
  if (hipMalloc(&d, sizeof *d) != hipSuccess) return BINE_ERR_NO_MEM;
  int rc = BINE_SUCCESS;
  if (hipMemsetAsync(d, 0, sizeof *d, st) != hipSuccess) rc = BINE_ERR_HIP;
  size_t blocks = (n + kBlock * 8 - 1) / (kBlock * 8);
  if (blocks > 4096) blocks = 4096;
  if (blocks == 0) blocks = 1;
  if (rc == BINE_SUCCESS) {
    switch (bine_dtype_size(dtype)) {
      case 1: hipLaunchKernelGGL((k_checksum<uint8_t>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const uint8_t *)buf, n, d); break;
      case 2: hipLaunchKernelGGL((k_checksum<uint16_t>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const uint16_t *)buf, n, d); break;
      case 4: hipLaunchKernelGGL((k_checksum<uint32_t>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const uint32_t *)buf, n, d); break;
      case 8: hipLaunchKernelGGL((k_checksum<uint64_t>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const uint64_t *)buf, n, d); break;
      default: rc = BINE_ERR_UNSUPPORTED;
    }
  }
  unsigned long long h = 0;
  if (rc == BINE_SUCCESS && (hipGetLastError() != hipSuccess ||
                             hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
                             hipStreamSynchronize(st) != hipSuccess))
    rc = BINE_ERR_HIP;
  (void)hipFree(d);
  if (rc == BINE_SUCCESS) *host_out = h;
  return rc;
}

// workgroup slots of the current device for one direct-transport kernel
// (bine_dm_launch_cap): kind 0 k_dm_move, 1 k_dm_move_tree<T, OP, nl>,
// 2 k_dm_fused<T, OP>; T / OP from (dtype, op) as the launchers pick them
int dm_launch_cap(int kind, int dtype, int op, int nl, int share) {
  const void *k = nullptr;
  if (kind == 0) {
    k = (const void *)k_dm_move;
  } else if (kind == 1 || kind == 2) {
    with_dm_dtype(dtype, [&](auto tag) {
      using T = typename decltype(tag)::type;
      k = with_op<T>(op, [&](auto opc) {
        constexpr int OP = decltype(opc)::value;
        return kind == 1 ? dmt_kernel<T, OP>(nl) : (const void *)k_dm_fused<T, OP>;
      }, (const void *)nullptr);
      return BINE_SUCCESS;
    });
  }
  return k ? dm_cap(k, share) : -1;
}

}  // namespace bine

extern "C" int bine_set_reduce_tuning(int unroll, int maxblocks, int nontemporal) {
  bine::g_unroll = (unroll == 1 || unroll == 2 || unroll == 4 || unroll == 8) ? unroll : bine::kDefaultUnroll;
  bine::g_maxblocks = maxblocks;
  bine::g_nt = nontemporal;
  return BINE_SUCCESS;
}

#endif  // BINE_OPSET == 0
#if BINE_OPSET != 0
}  // namespace bine
#endif
