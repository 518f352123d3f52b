// segments.cpp -- the planners of the segment family: the LaunchTables
// (bine_internal.h) that kernels.hip issues, one kernel launch each.
//
// Host only, no HIP: plain C++ over addresses and sizes, so the CPU suite can
// check the cover (bine_plan_*) and stand-alone programs can run the planners
// under the host sanitizers (tools/*_check.cpp).  A kernel derives a segment's
// head and vector count by calling the functions the planners call (seg_head /
// seg_nvec, bine_internal.h) on the same descriptor.
//   plan_seg_launches / bine_plan_segments   k_copy_segs    (tools/segments_check.cpp)
//   plan_shard_launches / bine_plan_shards   k_copy_shards  (tools/shards_check.cpp)
//   plan_norm_launches / bine_plan_sumsq     k_sumsq_segs, k_scale_segs: plan_seg_launches'
//                                            table over the buffers themselves (tools/sumsq_check.cpp)
//   plan_adamw_launches / bine_plan_adamw    k_adamw_segs: plan_norm_launches' table over p, cut at
//                                            kAdamwSegsPerLaunch descriptors, with the step's constants
//                                            (bine_adamw_consts) beside them (tools/adamw_check.cpp)
//   plan_quant_launches / bine_plan_quant    k_quant_segs (both directions): plan_norm_launches' table over
//                                            the wide side with one body flag per slot; the FP8 calls'
//                                            refusals (amax_args, fp8_scales_args, quant_args) and
//                                            bine_fp8_scale_host, the host compilation of fp8_scale_rule
//                                            (tools/quant_check.cpp)
//   plan_mx_launches / bine_plan_mx          k_mx_segs (both directions): a table of its own over the wide
//                                            side, tiles counted from the segment's first element as MX
//                                            blocks are, kMxSegsPerLaunch descriptors per launch, one body
//                                            flag per slot; the MX calls' refusals (mx_args, mx_multi_args)
//                                            and bine_mx_scale_host, the host compilation of mx_scale_rule
//                                            (tools/mx_check.cpp)
//   plan_mx_sum_launches / bine_plan_mx_sum  k_mx_sum_segs: plan_mx_launches' table over the destination,
//                                            the body flag dst's alone; the wire layout of a bucket
//                                            (mx_wire_layout, bine_mx_wire_bytes) and the refusals of the
//                                            sum and of the MX reduce-scatter (mx_sum_args, mx_rs_args;
//                                            tools/mxrs_check.cpp)
//   plan_mx_ef_launches / bine_plan_mx_ef    k_mx_ef_segs: plan_mx_launches' tiles over the source, cut at
//                                            kMxEfSegsPerLaunch descriptors, the body flag of source, data
//                                            and residual; the refusals of the error-feedback calls
//                                            (mx_ef_args, mx_ef_rs_args; tools/mxef_check.cpp)
// Dynamic loss scaling keeps its host half here too:
// bine_step_state_init, the refusals (step_update_args, adamw_dyn_args) and
// bine_step_update_host, the host compilation of the statement k_step_update
// runs (step_update_rule, bine_internal.h; tools/step_check.cpp).
#include <algorithm>
#include <climits>
#include <cmath>

#include "bine_internal.h"

namespace bine {

int plan_seg_launches(int n, const uint64_t *dst_addr, const uint64_t *src_addr, const size_t *bytes,
                      std::vector<SegLaunch> &out) {
  out.clear();
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!dst_addr || !src_addr || !bytes)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++) {
    if (bytes[k] == 0) continue;
    if (!dst_addr[k] || !src_addr[k]) return BINE_ERR_ARG;
    if (out.empty() || out.back().nseg == kSegsPerLaunch) out.emplace_back();
    SegLaunch &L = out.back();
    const int s = L.nseg++;
    L.seg[s] = k;
    L.head[s] = seg_head(dst_addr[k], bytes[k]);
    L.nvec[s] = seg_nvec(bytes[k], L.head[s]);
    const uint64_t tiles = (L.nvec[s] + kCopyTileVecs - 1) / kCopyTileVecs;
    const uint64_t end = L.tile0[s] + (tiles ? tiles : 1);
    if (end > kSegMaxWgs) return BINE_ERR_ARG;
    L.tile0[s + 1] = (uint32_t)end;
  }
  return BINE_SUCCESS;
}

// tiles (workgroups) per shard of one tensor: the most any of its shards needs.
// A shard's tile count depends on its destination's phase mod 16 B, which has a
// period of at most 16 in j.
static uint64_t shard_tiles(int nranks, int dir, uint64_t packed, uint64_t block, uint64_t poff, uint64_t flat,
                            uint64_t bytes) {
  uint64_t tps = 1;
  for (int j = 0; j < nranks && j < 16; j++) {
    const uint64_t nvec = seg_nvec(bytes, seg_head(shard_dst(dir, packed, block, poff, flat, bytes, j), bytes));
    tps = std::max(tps, (nvec + kCopyTileVecs - 1) / kCopyTileVecs);
  }
  return tps;
}

int plan_shard_launches(int n, int nranks, int dir, uint64_t packed_addr, const uint64_t *flat_addr,
                        const size_t *bytes, std::vector<ShardLaunch> &out, uint64_t *block_bytes) {
  out.clear();
  if (block_bytes) *block_bytes = 0;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (nranks < 1 || nranks > kShardMaxRanks) return BINE_ERR_ARG;
  if (dir != 0 && dir != 1) return BINE_ERR_ARG;
  if (n > 0 && (!flat_addr || !bytes)) return BINE_ERR_ARG;
  uint64_t block = 0;
  for (int k = 0; k < n; k++) {
    if (bytes[k] == 0) continue;
    if (!flat_addr[k] || !packed_addr) return BINE_ERR_ARG;
    // more than one launch's workgroups for one shard; also keeps every sum below 2^64
    if (bytes[k] / 16 / kCopyTileVecs > kSegMaxWgs) return BINE_ERR_ARG;
    block += bytes[k];
  }
  if (block_bytes) *block_bytes = block;
  uint64_t poff = 0;
  for (int k = 0; k < n; k++) {
    if (bytes[k] == 0) continue;
    // tile0 counts tiles per shard; the launch's grid is nranks times its total
    const uint64_t tps = shard_tiles(nranks, dir, packed_addr, block, poff, flat_addr[k], bytes[k]);
    if (tps * nranks > kSegMaxWgs) return BINE_ERR_ARG;
    if (out.empty() || out.back().nseg == kSegsPerLaunch ||
        (out.back().tile0[out.back().nseg] + tps) * nranks > kSegMaxWgs)
      out.emplace_back();
    ShardLaunch &L = out.back();
    const int s = L.nseg++;
    L.seg[s] = k;
    L.poff[s] = poff;
    L.tile0[s + 1] = (uint32_t)(L.tile0[s] + tps);
    poff += bytes[k];
  }
  return BINE_SUCCESS;
}

size_t norm_esz(int dtype) {
  switch (dtype) {
    case BINE_FLOAT: return 4;
    case BINE_DOUBLE: return 8;
    case BINE_FLOAT16:
    case BINE_BFLOAT16: return 2;
    default: return 0;
  }
}

int plan_norm_launches(int n, const uint64_t *addrs, const size_t *counts, int dtype, std::vector<SegLaunch> &out,
                       uint64_t *tiles) {
  out.clear();
  if (tiles) *tiles = 0;
  const size_t esz = norm_esz(dtype);
  if (!esz) return BINE_ERR_ARG;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!addrs || !counts)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++)
    if (counts[k] && !addrs[k]) return BINE_ERR_ARG;
  std::vector<size_t> bytes((size_t)n);
  for (int k = 0; k < n; k++) {
    if (counts[k] && addrs[k] % esz) return BINE_ERR_ARG;
    if (counts[k] > ((size_t)1 << 56)) return BINE_ERR_ARG;  // keeps the byte count and every sum below 2^64
    bytes[k] = counts[k] * esz;
  }
  if (const int rc = plan_seg_launches(n, addrs, addrs, bytes.data(), out)) return rc;
  uint64_t t = 0;
  for (const SegLaunch &L : out) t += L.tile0[L.nseg];
  if (tiles) *tiles = t;
  return BINE_SUCCESS;
}

size_t adamw_esz(int dtype) { return dtype == BINE_DOUBLE ? 0 : norm_esz(dtype); }

// one of m / v / g / pout against the list rule p has passed: a NULL buffer
// with a non-zero count, a buffer not aligned to its element
static int adamw_list(int n, const uint64_t *a, const size_t *counts, size_t esz) {
  for (int k = 0; k < n; k++)
    if (counts[k] && (!a[k] || a[k] % esz)) return BINE_ERR_ARG;
  return BINE_SUCCESS;
}

int plan_adamw_launches(int n, const uint64_t *p, const uint64_t *m, const uint64_t *v, const uint64_t *g,
                        const uint64_t *pout, const size_t *counts, int gdtype, int odtype,
                        std::vector<AdamwLaunch> &out) {
  out.clear();
  const size_t gsz = adamw_esz(gdtype), osz = adamw_esz(odtype);
  if (!gsz || !osz) return BINE_ERR_ARG;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!p || !m || !v || !g || !counts)) return BINE_ERR_ARG;
  std::vector<SegLaunch> ls;
  if (const int rc = plan_norm_launches(n, p, counts, BINE_FLOAT, ls, nullptr)) return rc;
  if (adamw_list(n, m, counts, 4) || adamw_list(n, v, counts, 4) || adamw_list(n, g, counts, gsz)) return BINE_ERR_ARG;
  if (pout && adamw_list(n, pout, counts, osz)) return BINE_ERR_ARG;
  for (const SegLaunch &L : ls)
    for (int s0 = 0; s0 < L.nseg; s0 += kAdamwSegsPerLaunch) {
      out.emplace_back();
      AdamwLaunch &A = out.back();
      A.nseg = std::min(kAdamwSegsPerLaunch, L.nseg - s0);
      for (int s = 0; s < A.nseg; s++) {
        const int k = L.seg[s0 + s];
        A.seg[s] = k;
        A.tile0[s] = L.tile0[s0 + s] - L.tile0[s0];
        // h: the elements before p's first 16-B boundary (seg_head of a span that
        // reaches it: the flag is the addresses', whatever the count); the vector body
        // needs every other operand on a boundary of its own 4-element vector there
        const uint64_t h = seg_head(p[k], 16) / 4;
        const bool vec = (m[k] + 4 * h) % 16 == 0 && (v[k] + 4 * h) % 16 == 0 && (g[k] + gsz * h) % (4 * gsz) == 0 &&
                         (!pout || (pout[k] + osz * h) % (4 * osz) == 0);
        if (!vec) A.elem |= (uint64_t)1 << s;
      }
      A.tile0[A.nseg] = L.tile0[s0 + A.nseg] - L.tile0[s0];
    }
  return BINE_SUCCESS;
}

// the list checks of bine_adamw_segments (through pout) and the launches
static int adamw_list_args(int n, void *const *p, void *const *m, void *const *v, const void *const *g,
                           void *const *pout, const size_t *counts, int gdtype, int odtype,
                           std::vector<AdamwLaunch> *ls) {
  if (!adamw_esz(gdtype) || !adamw_esz(odtype)) return BINE_ERR_ARG;
  std::vector<uint64_t> a, o;  // p, m, v, g; the optional pout
  if (const int rc = seg_list_addrs(n, counts, {p, m, v, g}, a)) return rc;
  if (pout) seg_list_addrs(n, counts, {pout}, o);
  std::vector<AdamwLaunch> local;
  const uint64_t *pa = a.data();
  return plan_adamw_launches(n, pa, pa + n, pa + 2 * n, pa + 3 * n, pout ? o.data() : nullptr, counts, gdtype, odtype,
                             ls ? *ls : local);
}

int adamw_args(int n, void *const *p, void *const *m, void *const *v, const void *const *g, void *const *pout,
               const size_t *counts, int gdtype, int odtype, double lr, double beta1, double beta2, double eps,
               double weight_decay, int64_t step, const double *gcoef, double grad_mul, float consts[8],
               std::vector<AdamwLaunch> *ls) {
  if (const int rc = adamw_list_args(n, p, m, v, g, pout, counts, gdtype, odtype, ls)) return rc;
  if ((uintptr_t)gcoef & 7) return BINE_ERR_ARG;
  if (!(grad_mul >= 0.0) || std::isinf(grad_mul)) return BINE_ERR_ARG;  // NaN, negative or infinite
  float c[8];
  return bine_adamw_consts(lr, beta1, beta2, eps, weight_decay, step, consts ? consts : c);
}

int adamw_dyn_args(int n, void *const *p, void *const *m, void *const *v, const void *const *g, void *const *pout,
                   const size_t *counts, int gdtype, int odtype, const void *state, std::vector<AdamwLaunch> *ls) {
  if (const int rc = adamw_list_args(n, p, m, v, g, pout, counts, gdtype, odtype, ls)) return rc;
  return !state || ((uintptr_t)state & 7) ? BINE_ERR_ARG : BINE_SUCCESS;
}

int step_update_args(const void *state, const void *norm2, const bine_step_hyper *h) {
  if (!h) return BINE_ERR_ARG;
  float c[8];
  if (const int rc = bine_adamw_consts(h->lr, h->beta1, h->beta2, h->eps, h->weight_decay, 1, c)) return rc;
  if (!(h->max_norm >= 0.0) || !(h->clip_eps >= 0.0)) return BINE_ERR_ARG;  // negative or NaN
  if (!(h->growth_factor >= 1.0) || std::isinf(h->growth_factor)) return BINE_ERR_ARG;
  if (!(h->backoff_factor > 0.0 && h->backoff_factor <= 1.0)) return BINE_ERR_ARG;
  if (h->growth_interval < 1) return BINE_ERR_ARG;
  if (!(h->min_scale > 0.0 && h->min_scale <= h->max_scale) || std::isinf(h->max_scale)) return BINE_ERR_ARG;
  if (!state || ((uintptr_t)state & 7) || !norm2 || ((uintptr_t)norm2 & 7)) return BINE_ERR_ARG;
  return BINE_SUCCESS;
}

int plan_quant_launches(int n, const uint64_t *wide, const uint64_t *bytes8, const size_t *counts, int dtype,
                        std::vector<QuantLaunch> &out) {
  out.clear();
  const size_t esz = adamw_esz(dtype);
  if (!esz) return BINE_ERR_ARG;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!wide || !bytes8 || !counts)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++)
    if (counts[k] && (!wide[k] || !bytes8[k])) return BINE_ERR_ARG;
  std::vector<SegLaunch> ls;
  if (const int rc = plan_norm_launches(n, wide, counts, dtype, ls, nullptr)) return rc;
  for (const SegLaunch &L : ls) {
    out.emplace_back();
    static_cast<LaunchTable<kSegsPerLaunch> &>(out.back()) = L;
  }
  for (QuantLaunch &Q : out)
    for (int s = 0; s < Q.nseg; s++) {
      const int k = Q.seg[s];
      // h: the elements before wide's first 16-B boundary (the addresses' flag,
      // whatever the count); there bytes8 must stand on a boundary of the 16 / esz
      // bytes one wide vector holds
      const uint64_t h = seg_head(wide[k], 16) / esz;
      if ((bytes8[k] + h) % (16 / esz)) Q.elem[s >> 6] |= (uint64_t)1 << (s & 63);
    }
  return BINE_SUCCESS;
}

void quant_set_bodies(std::vector<QuantLaunch> &ls, const void *const *wide, const void *const *bytes8, int dtype) {
  const size_t esz = adamw_esz(dtype);
  for (QuantLaunch &Q : ls) {
    for (uint64_t &w : Q.elem) w = 0;
    for (int s = 0; s < Q.nseg; s++) {
      const int k = Q.seg[s];
      const uint64_t h = seg_head((uint64_t)(uintptr_t)wide[k], 16) / esz;
      if (((uint64_t)(uintptr_t)bytes8[k] + h) % (16 / esz)) Q.elem[s >> 6] |= (uint64_t)1 << (s & 63);
    }
  }
}

AmaxLaunch amax_launch_of(const LaunchTable<kSegsPerLaunch> &tiles) {
  AmaxLaunch A = tiles;
  uint32_t wgs = 0;
  for (int s = 0; s < tiles.nseg; s++) {
    A.tile0[s] = wgs;
    wgs += (tiles.tile0[s + 1] - tiles.tile0[s] + kAmaxTilesPerWg - 1) / kAmaxTilesPerWg;
  }
  A.tile0[tiles.nseg] = wgs;
  return A;
}

static int refuse(const char **why, const char *what) {
  if (why) *why = what;
  return BINE_ERR_ARG;
}

int amax_args(int n, const void *const *bufs, const size_t *counts, int dtype, const void *out, const char **why,
              std::vector<AmaxLaunch> *ls) {
  if (!adamw_esz(dtype)) return refuse(why, "dtype: float, float16 or bfloat16");
  std::vector<uint64_t> a;
  if (seg_list_addrs(n, counts, {bufs}, a)) return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  std::vector<SegLaunch> tiles;
  if (plan_norm_launches(n, a.data(), counts, dtype, tiles, nullptr))
    return refuse(why, "a NULL buffer with a non-zero count, or a buffer not aligned to its element");
  if (!out || ((uintptr_t)out & 3)) return refuse(why, "out NULL or not 4-byte aligned");
  if (ls) {
    ls->clear();
    for (const SegLaunch &L : tiles) ls->push_back(amax_launch_of(L));
  }
  return BINE_SUCCESS;
}

int fp8_scales_args(int n, const void *amax, int fmt, const void *scales, const char **why) {
  if (!fp8_fmt_ok(fmt)) return refuse(why, "fmt: BINE_FP8_E4M3 or BINE_FP8_E5M2");
  if (n < 0 || n > BINE_MULTI_MAX) return refuse(why, "n outside [0, BINE_MULTI_MAX]");
  if (!amax || ((uintptr_t)amax & 3)) return refuse(why, "amax NULL or not 4-byte aligned");
  if (!scales || ((uintptr_t)scales & 3)) return refuse(why, "scales NULL or not 4-byte aligned");
  return BINE_SUCCESS;
}

int quant_args(int n, const void *const *wide, const void *const *bytes8, const size_t *counts, int dtype, int fmt,
               const void *scales, const char **why, std::vector<QuantLaunch> *ls) {
  if (!adamw_esz(dtype)) return refuse(why, "dtype: float, float16 or bfloat16");
  if (!fp8_fmt_ok(fmt)) return refuse(why, "fmt: BINE_FP8_E4M3 or BINE_FP8_E5M2");
  std::vector<uint64_t> a;  // wide, bytes8
  if (seg_list_addrs(n, counts, {wide, bytes8}, a))
    return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  std::vector<QuantLaunch> local;
  if (plan_quant_launches(n, a.data(), a.data() + n, counts, dtype, ls ? *ls : local))
    return refuse(why, "a NULL buffer with a non-zero count, or a wide buffer not aligned to its element");
  if ((uintptr_t)scales & 3) return refuse(why, "scales not 4-byte aligned");
  return BINE_SUCCESS;
}

// The MX tile rule, called by plan_mx_launches (k_mx_segs, and through it
// plan_mx_sum_launches for k_mx_sum_segs) and by plan_mx_ef_launches: tiles
// of kCopyTileVecs * 16 bytes of esz-byte elements counted from the segment's
// first element, at least one per non-empty segment, at most N slots per
// launch; elem(k) = 1 where tensor k takes the element body.
template <int N, typename L, typename F>
static int mx_tiles(int n, const size_t *counts, size_t esz, std::vector<L> &out, F &&elem) {
  const uint64_t tile_elems = kCopyTileVecs * 16 / esz;  // whole blocks: a multiple of kMxBlock
  for (int k = 0; k < n; k++) {
    if (counts[k] == 0) continue;
    const uint64_t tiles = (counts[k] + tile_elems - 1) / tile_elems;
    if (tiles > kSegMaxWgs) return BINE_ERR_ARG;
    if (out.empty() || out.back().nseg == N || out.back().tile0[out.back().nseg] + tiles > kSegMaxWgs)
      out.emplace_back();
    L &l = out.back();
    const int s = l.nseg++;
    l.seg[s] = k;
    l.tile0[s + 1] = (uint32_t)(l.tile0[s] + tiles);
    if (elem(k)) l.elem[s >> 6] |= (uint64_t)1 << (s & 63);
  }
  return BINE_SUCCESS;
}

int plan_mx_launches(int n, const uint64_t *wide, const uint64_t *data8, const uint64_t *scl8, const size_t *counts,
                     int dtype, int fmt, std::vector<MxLaunch> &out) {
  out.clear();
  const size_t esz = adamw_esz(dtype);
  if (!esz || !mx_fmt_ok(fmt)) return BINE_ERR_ARG;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!wide || !data8 || !scl8 || !counts)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++)
    if (counts[k] && (!wide[k] || !data8[k] || !scl8[k])) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++) {
    if (counts[k] && wide[k] % esz) return BINE_ERR_ARG;
    if (counts[k] > ((size_t)1 << 56)) return BINE_ERR_ARG;  // keeps the byte count and every sum below 2^64
  }
  return mx_tiles<kMxSegsPerLaunch>(n, counts, esz, out, [&](int k) { return mx_body(wide[k], data8[k], esz, fmt); });
}

int plan_mx_ef_launches(int n, const uint64_t *src, const uint64_t *res, const uint64_t *data8, const uint64_t *scl8,
                        const size_t *counts, int dtype, int fmt, std::vector<MxEfLaunch> &out) {
  out.clear();
  const size_t esz = adamw_esz(dtype);
  if (!esz || !mx_fmt_ok(fmt)) return BINE_ERR_ARG;
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!src || !res || !data8 || !scl8 || !counts)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++)
    if (counts[k] && (!src[k] || !res[k] || !data8[k] || !scl8[k])) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++) {
    if (counts[k] && src[k] % esz) return BINE_ERR_ARG;
    if (counts[k] > ((size_t)1 << 56)) return BINE_ERR_ARG;  // keeps the byte count and every sum below 2^64
  }
  for (int k = 0; k < n; k++)
    if (counts[k] && res[k] % 4) return BINE_ERR_ARG;
  return mx_tiles<kMxEfSegsPerLaunch>(n, counts, esz, out,
                                      [&](int k) { return mx_ef_body(src[k], res[k], data8[k], esz, fmt); });
}

int mx_ef_args(int n, const void *const *src, const void *const *res, const void *const *data8,
               const void *const *scl8, const size_t *counts, int dtype, int fmt, const char **why,
               std::vector<MxEfLaunch> *ls) {
  if (!adamw_esz(dtype)) return refuse(why, "sdtype: float, float16 or bfloat16");
  if (!mx_fmt_ok(fmt)) return refuse(why, "fmt: BINE_MX_E4M3, BINE_MX_E5M2 or BINE_MX_E2M1");
  std::vector<uint64_t> a;  // src, res, data8, scl8
  if (seg_list_addrs(n, counts, {src, res, data8, scl8}, a))
    return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  std::vector<MxEfLaunch> local;
  const uint64_t *p = a.data();
  if (plan_mx_ef_launches(n, p, p + n, p + 2 * (size_t)n, p + 3 * (size_t)n, counts, dtype, fmt, ls ? *ls : local))
    return refuse(why, "a NULL buffer with a non-zero count, a source not aligned to its element, or a residual not "
                       "4-byte aligned");
  return BINE_SUCCESS;
}

void mx_set_bodies(std::vector<MxLaunch> &ls, const void *const *wide, const void *const *data8, int dtype, int fmt) {
  const size_t esz = adamw_esz(dtype);
  for (MxLaunch &L : ls) {
    for (uint64_t &w : L.elem) w = 0;
    for (int s = 0; s < L.nseg; s++) {
      const int k = L.seg[s];
      if (mx_body((uint64_t)(uintptr_t)wide[k], (uint64_t)(uintptr_t)data8[k], esz, fmt))
        L.elem[s >> 6] |= (uint64_t)1 << (s & 63);
    }
  }
}

int mx_args(int n, const void *const *wide, const void *const *data8, const void *const *scl8, const size_t *counts,
            int dtype, int fmt, const char **why, std::vector<MxLaunch> *ls) {
  if (!adamw_esz(dtype)) return refuse(why, "dtype: float, float16 or bfloat16");
  if (!mx_fmt_ok(fmt)) return refuse(why, "fmt: BINE_MX_E4M3, BINE_MX_E5M2 or BINE_MX_E2M1");
  std::vector<uint64_t> a;  // wide, data8, scl8
  if (seg_list_addrs(n, counts, {wide, data8, scl8}, a))
    return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  std::vector<MxLaunch> local;
  if (plan_mx_launches(n, a.data(), a.data() + n, a.data() + 2 * (size_t)n, counts, dtype, fmt, ls ? *ls : local))
    return refuse(why, "a NULL buffer with a non-zero count, or a wide buffer not aligned to its element");
  return BINE_SUCCESS;
}

int mx_multi_args(int n, void *const *params8, void *const *scales8, const void *const *src,
                  const size_t *shard_counts, int sdtype, int fmt, const char **why, std::vector<MxLaunch> *ls) {
  if (!adamw_esz(sdtype)) return refuse(why, "sdtype: float, float16 or bfloat16");
  if (!mx_fmt_ok(fmt)) return refuse(why, "fmt: BINE_MX_E4M3, BINE_MX_E5M2 or BINE_MX_E2M1");
  if (n < 0 || n > BINE_MULTI_MAX / 2) return refuse(why, "n outside [0, BINE_MULTI_MAX / 2]");
  if (const int rc = mx_args(n, src, params8, scales8, shard_counts, sdtype, fmt, why, ls)) return rc;
  for (int k = 0; k < n; k++)
    if (shard_counts[k] % kMxBlock || shard_counts[k] > (size_t)INT_MAX)
      return refuse(why, "a shard count not a multiple of 32, or above INT_MAX");
  return BINE_SUCCESS;
}

int mx_wire_layout(int n, const size_t *counts, int fmt, std::vector<uint64_t> *off, uint64_t *data_bytes,
                   uint64_t *block_bytes) {
  if (!mx_fmt_ok(fmt) || n < 0 || (n > 0 && !counts)) return BINE_ERR_ARG;
  if (off) off->assign(2 * (size_t)n, 0);
  uint64_t d = 0, s = 0;
  for (int k = 0; k < n; k++) {
    if (counts[k] % kMxBlock) return BINE_ERR_ARG;
    if (off) (*off)[k] = d, (*off)[(size_t)n + k] = s;
    // a multiple of 32: dbytes is a multiple of 16, and count + 1 does not wrap
    if (__builtin_add_overflow(d, mx_dbytes(counts[k], fmt), &d) ||
        __builtin_add_overflow(s, (uint64_t)counts[k] / kMxBlock, &s))
      return BINE_ERR_ARG;
  }
  uint64_t t;
  if (__builtin_add_overflow(d, s, &t) || __builtin_add_overflow(t, (uint64_t)15, &t)) return BINE_ERR_ARG;
  if (off)
    for (int k = 0; k < n; k++) (*off)[(size_t)n + k] += d;
  if (data_bytes) *data_bytes = d;
  if (block_bytes) *block_bytes = t & ~(uint64_t)15;
  return BINE_SUCCESS;
}

int plan_mx_sum_launches(int n, const uint64_t *dst, const size_t *counts, int ddtype, int fmt,
                         std::vector<MxLaunch> &out) {
  // the byte side stands on a 16-B boundary in every block: mx_body is dst's alone
  const std::vector<uint64_t> unit((size_t)(n > 0 ? n : 0), 16);
  if (const int rc = plan_mx_launches(n, dst, unit.data(), unit.data(), counts, ddtype, fmt, out)) return rc;
  for (int k = 0; k < n; k++)
    if (counts[k] % kMxBlock) {
      out.clear();
      return BINE_ERR_ARG;
    }
  return BINE_SUCCESS;
}

int mx_sum_args(int n, int nstreams, const void *packed, size_t block_bytes, void *const *dst, const size_t *counts,
                int ddtype, int fmt, const char **why, std::vector<MxLaunch> *ls, std::vector<uint64_t> *off) {
  if (!adamw_esz(ddtype)) return refuse(why, "ddtype: float, float16 or bfloat16");
  if (!mx_fmt_ok(fmt)) return refuse(why, "fmt: BINE_MX_E4M3, BINE_MX_E5M2 or BINE_MX_E2M1");
  std::vector<uint64_t> a;
  if (seg_list_addrs(n, counts, {dst}, a)) return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  std::vector<MxLaunch> local;
  std::vector<MxLaunch> &L = ls ? *ls : local;
  const std::vector<uint64_t> unit((size_t)n, 16);
  if (plan_mx_launches(n, a.data(), unit.data(), unit.data(), counts, ddtype, fmt, L))
    return refuse(why, "a NULL buffer with a non-zero count, or a destination not aligned to its element");
  uint64_t D = 0, B = 0;
  if (mx_wire_layout(n, counts, fmt, off, &D, &B)) {
    L.clear();
    return refuse(why, "a count not a multiple of 32, or the bucket's bytes overflow");
  }
  if (nstreams < 1 || nstreams > kMxSumMaxStreams) return refuse(why, "nstreams outside [1, 16]");
  if (B == 0) return BINE_SUCCESS;
  if (!packed || ((uintptr_t)packed & 15)) return refuse(why, "packed NULL or not 16-B aligned");
  if (block_bytes % 16 || block_bytes < B)
    return refuse(why, "block_bytes not a multiple of 16, or below the bucket's wire block");
  return BINE_SUCCESS;
}

// ef: res is a third list beside sbufs (binary32, 4-byte aligned); otherwise it is not looked at
static int mx_rs_args_of(bool ef, int P, int n, const void *const *sbufs, const void *const *res, void *const *rbufs,
                         const size_t *shard_counts, int sdtype, int rdtype, int fmt, const void *send_ws,
                         const void *recv_ws, size_t ws_bytes, const char **why, uint64_t *block,
                         std::vector<uint64_t> *off) {
  if (block) *block = 0;
  const size_t ssz = adamw_esz(sdtype), rsz = adamw_esz(rdtype);
  if (!ssz || !rsz) return refuse(why, "sdtype, rdtype: float, float16 or bfloat16");
  if (!mx_fmt_ok(fmt)) return refuse(why, "fmt: BINE_MX_E4M3, BINE_MX_E5M2 or BINE_MX_E2M1");
  std::vector<uint64_t> a, ar;  // sbufs, rbufs; res where ef
  if (seg_list_addrs(n, shard_counts, {sbufs, rbufs}, a) || (ef && seg_list_addrs(n, shard_counts, {res}, ar)))
    return refuse(why, "n outside [0, BINE_MULTI_MAX], or a NULL array");
  for (int k = 0; k < n; k++)
    if (shard_counts[k] && (!a[k] || !a[(size_t)n + k] || (ef && !ar[k])))
      return refuse(why, "a NULL buffer with a non-zero count");
  for (int k = 0; k < n; k++)
    if (shard_counts[k] && (a[k] % ssz || a[(size_t)n + k] % rsz))
      return refuse(why, "a source or destination not aligned to its element");
  for (int k = 0; k < n; k++)
    if (ef && shard_counts[k] && ar[k] % 4) return refuse(why, "a residual not 4-byte aligned");
  for (int k = 0; k < n; k++)
    if (shard_counts[k] % kMxBlock || shard_counts[k] > (size_t)INT_MAX)
      return refuse(why, "a shard count not a multiple of 32, or above INT_MAX");
  uint64_t D = 0, B = 0;
  if (mx_wire_layout(n, shard_counts, fmt, off, &D, &B)) return refuse(why, "the bucket's bytes overflow");
  if (block) *block = B;
  if (B == 0) return BINE_SUCCESS;
  if (!send_ws || !recv_ws || ((uintptr_t)send_ws & 15) || ((uintptr_t)recv_ws & 15))
    return refuse(why, "send_ws or recv_ws NULL or not 16-B aligned");
  const uint64_t s0 = (uint64_t)(uintptr_t)send_ws, r0 = (uint64_t)(uintptr_t)recv_ws;
  if (s0 < r0 ? r0 - s0 < ws_bytes : s0 - r0 < ws_bytes) return refuse(why, "send_ws and recv_ws overlap");
  if (ws_bytes / (uint64_t)(P > 0 ? P : 1) < B) return refuse(why, "ws_bytes below comm size * block bytes");
  return BINE_SUCCESS;
}

int mx_rs_args(int P, int n, const void *const *sbufs, void *const *rbufs, const size_t *shard_counts, int sdtype,
               int rdtype, int fmt, const void *send_ws, const void *recv_ws, size_t ws_bytes, const char **why,
               uint64_t *block, std::vector<uint64_t> *off) {
  return mx_rs_args_of(false, P, n, sbufs, nullptr, rbufs, shard_counts, sdtype, rdtype, fmt, send_ws, recv_ws,
                       ws_bytes, why, block, off);
}

int mx_ef_rs_args(int P, int n, const void *const *sbufs, const void *const *res, void *const *rbufs,
                  const size_t *shard_counts, int sdtype, int rdtype, int fmt, const void *send_ws,
                  const void *recv_ws, size_t ws_bytes, const char **why, uint64_t *block,
                  std::vector<uint64_t> *off) {
  return mx_rs_args_of(true, P, n, sbufs, res, rbufs, shard_counts, sdtype, rdtype, fmt, send_ws, recv_ws, ws_bytes,
                       why, block, off);
}

}  // namespace bine

extern "C" int bine_mx_wire_bytes(int n, const size_t *shard_counts, int fmt, size_t *data_bytes,
                                  size_t *block_bytes) {
  if (!data_bytes || !block_bytes) return BINE_ERR_ARG;
  uint64_t D = 0, B = 0;
  if (const int rc = bine::mx_wire_layout(n, shard_counts, fmt, nullptr, &D, &B)) return rc;
  *data_bytes = (size_t)D, *block_bytes = (size_t)B;
  return BINE_SUCCESS;
}

extern "C" int64_t bine_plan_mx_sum(int n, const uint64_t *dst, const size_t *counts, int ddtype, int fmt,
                                    uint64_t *out, int64_t cap) {
  std::vector<bine::MxLaunch> ls;
  const int rc = bine::plan_mx_sum_launches(n, dst, counts, ddtype, fmt, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::MxLaunch &L = ls[l];
    for (int s = 0; s < L.nseg; s++, nt++)
      if (out && nt < cap) {
        uint64_t *e = out + 5 * nt;
        e[0] = l, e[1] = (uint64_t)L.seg[s], e[2] = L.tile0[s], e[3] = L.tile0[s + 1] - L.tile0[s];
        e[4] = (L.elem[s >> 6] >> (s & 63)) & 1;
      }
  }
  return nt;
}

extern "C" int bine_fp8_scale_host(uint32_t amax_bits, int fmt, float *scale, float *inv) {
  if (!bine::fp8_fmt_ok(fmt) || !scale || !inv) return BINE_ERR_ARG;
  bine::fp8_scale_rule(amax_bits, fmt, scale, inv);
  return BINE_SUCCESS;
}

extern "C" int64_t bine_plan_quant(int n, const uint64_t *wide, const uint64_t *bytes8, const size_t *counts,
                                   int dtype, uint64_t *out, int64_t cap) {
  std::vector<bine::QuantLaunch> ls;
  const int rc = bine::plan_quant_launches(n, wide, bytes8, counts, dtype, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::QuantLaunch &Q = ls[l];
    for (int s = 0; s < Q.nseg; s++, nt++)
      if (out && nt < cap) {
        uint64_t *e = out + 5 * nt;
        e[0] = l, e[1] = (uint64_t)Q.seg[s], e[2] = Q.tile0[s], e[3] = Q.tile0[s + 1] - Q.tile0[s];
        e[4] = (Q.elem[s >> 6] >> (s & 63)) & 1;
      }
  }
  return nt;
}

extern "C" int bine_mx_scale_host(uint32_t amax_bits, int fmt, uint8_t *s) {
  if (!bine::mx_fmt_ok(fmt) || !s) return BINE_ERR_ARG;
  *s = bine::mx_scale_rule(amax_bits, fmt);
  return BINE_SUCCESS;
}

extern "C" int64_t bine_plan_mx(int n, const uint64_t *wide, const uint64_t *data8, const uint64_t *scl8,
                                const size_t *counts, int dtype, int fmt, uint64_t *out, int64_t cap) {
  std::vector<bine::MxLaunch> ls;
  const int rc = bine::plan_mx_launches(n, wide, data8, scl8, counts, dtype, fmt, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::MxLaunch &L = ls[l];
    for (int s = 0; s < L.nseg; s++, nt++)
      if (out && nt < cap) {
        uint64_t *e = out + 5 * nt;
        e[0] = l, e[1] = (uint64_t)L.seg[s], e[2] = L.tile0[s], e[3] = L.tile0[s + 1] - L.tile0[s];
        e[4] = (L.elem[s >> 6] >> (s & 63)) & 1;
      }
  }
  return nt;
}

extern "C" int64_t bine_plan_mx_ef(int n, const uint64_t *src, const uint64_t *res, const uint64_t *data8,
                                   const uint64_t *scl8, const size_t *counts, int dtype, int fmt, uint64_t *out,
                                   int64_t cap) {
  std::vector<bine::MxEfLaunch> ls;
  const int rc = bine::plan_mx_ef_launches(n, src, res, data8, scl8, counts, dtype, fmt, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::MxEfLaunch &L = ls[l];
    for (int s = 0; s < L.nseg; s++, nt++)
      if (out && nt < cap) {
        uint64_t *e = out + 5 * nt;
        e[0] = l, e[1] = (uint64_t)L.seg[s], e[2] = L.tile0[s], e[3] = L.tile0[s + 1] - L.tile0[s];
        e[4] = (L.elem[s >> 6] >> (s & 63)) & 1;
      }
  }
  return nt;
}

extern "C" int bine_step_state_init(void *host_state, double scale, int64_t step, double beta1, double beta2) {
  if (!host_state || ((uintptr_t)host_state & 7)) return BINE_ERR_ARG;
  if (!(scale > 0.0) || std::isinf(scale)) return BINE_ERR_ARG;  // NaN, zero, negative or infinite
  if (step < 0) return BINE_ERR_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return BINE_ERR_ARG;
  bine::StepState *s = static_cast<bine::StepState *>(host_state);
  double pw1 = 1.0, pw2 = 1.0;
  for (int64_t t = 0; t < step; t++) {
    const double a = pw1 * beta1, b = pw2 * beta2;
    if (a == pw1 && b == pw2) break;  // zero, or a subnormal the product rounds back to: nothing changes any more
    pw1 = a, pw2 = b;
  }
  *s = bine::StepState{{scale, 0.0, (double)step, pw1, pw2, 0.0, 0.0, 0.0}, {0, 0, 0, 0, 0, 0, 0, 0}};
  return BINE_SUCCESS;
}

extern "C" int bine_step_update_host(void *host_state, double norm2, const bine_step_hyper *hyper) {
  if (const int rc = bine::step_update_args(host_state, &norm2, hyper)) return rc;
  bine::step_update_rule(static_cast<bine::StepState *>(host_state), norm2, *hyper);
  return BINE_SUCCESS;
}

extern "C" int bine_adamw_consts(double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                 float out[8]) {
  // negative or NaN; a beta outside [0, 1) or NaN
  if (!(lr >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return BINE_ERR_ARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return BINE_ERR_ARG;
  if (step < 1 || !out) return BINE_ERR_ARG;
  // binary64 throughout, one rounding (nearest even) to binary32 each
  out[0] = (float)(1.0 - lr * weight_decay);
  out[1] = (float)beta1;
  out[2] = (float)(1.0 - beta1);
  out[3] = (float)beta2;
  out[4] = (float)(1.0 - beta2);
  out[5] = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)step)));
  out[6] = (float)eps;
  out[7] = (float)(lr / (1.0 - std::pow(beta1, (double)step)));
  return BINE_SUCCESS;
}

extern "C" int64_t bine_plan_adamw(int n, const uint64_t *p, const uint64_t *m, const uint64_t *v, const uint64_t *g,
                                   const uint64_t *pout, const size_t *counts, int gdtype, int odtype, uint64_t *out,
                                   int64_t cap) {
  std::vector<bine::AdamwLaunch> ls;
  const int rc = bine::plan_adamw_launches(n, p, m, v, g, pout, counts, gdtype, odtype, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::AdamwLaunch &A = ls[l];
    for (int s = 0; s < A.nseg; s++, nt++)
      if (out && nt < cap) {
        uint64_t *e = out + 5 * nt;
        e[0] = l, e[1] = (uint64_t)A.seg[s], e[2] = A.tile0[s], e[3] = A.tile0[s + 1] - A.tile0[s];
        e[4] = (A.elem >> s) & 1;
      }
  }
  return nt;
}

extern "C" int64_t bine_plan_sumsq(int n, const uint64_t *addrs, const size_t *counts, int dtype) {
  std::vector<bine::SegLaunch> ls;
  uint64_t tiles = 0;
  const int rc = bine::plan_norm_launches(n, addrs, counts, dtype, ls, &tiles);
  return rc ? -(int64_t)rc : (int64_t)tiles;
}

extern "C" int64_t bine_plan_shards(int n, int nranks, int dir, uint64_t packed_addr, const uint64_t *flat_addr,
                                    const size_t *shard_bytes, uint64_t *out, int64_t cap) {
  std::vector<bine::ShardLaunch> ls;
  uint64_t block = 0;
  const int rc = bine::plan_shard_launches(n, nranks, dir, packed_addr, flat_addr, shard_bytes, ls, &block);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  auto put = [&](uint64_t launch, uint64_t ten, uint64_t shard, uint64_t off, uint64_t len, uint64_t kind) {
    if (out && nt < cap) {
      uint64_t *e = out + 6 * nt;
      e[0] = launch, e[1] = ten, e[2] = shard, e[3] = off, e[4] = len, e[5] = kind;
    }
    nt++;
  };
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::ShardLaunch &L = ls[l];
    for (int s = 0; s < L.nseg; s++) {
      const uint64_t k = (uint64_t)L.seg[s], b = shard_bytes[k];
      for (uint64_t j = 0; j < (uint64_t)nranks; j++) {
        const uint64_t head =
            bine::seg_head(bine::shard_dst(dir, packed_addr, block, L.poff[s], flat_addr[k], b, j), b);
        const uint64_t nvec = bine::seg_nvec(b, head), tail = b - head - 16 * nvec;
        if (head) put(l, k, j, 0, head, 1);
        for (uint64_t v = 0; v < nvec; v += bine::kCopyTileVecs)
          put(l, k, j, head + 16 * v, 16 * std::min<uint64_t>(bine::kCopyTileVecs, nvec - v), 0);
        if (tail) put(l, k, j, head + 16 * nvec, tail, 1);
      }
    }
  }
  return nt;
}

extern "C" int64_t bine_plan_segments(int n, const uint64_t *dst_addr, const uint64_t *src_addr, const size_t *bytes,
                                      uint64_t *out, int64_t cap) {
  std::vector<bine::SegLaunch> ls;
  const int rc = bine::plan_seg_launches(n, dst_addr, src_addr, bytes, ls);
  if (rc) return -(int64_t)rc;
  int64_t nt = 0;
  auto put = [&](uint64_t launch, uint64_t seg, uint64_t off, uint64_t len, uint64_t kind) {
    if (out && nt < cap) {
      uint64_t *e = out + 5 * nt;
      e[0] = launch, e[1] = seg, e[2] = off, e[3] = len, e[4] = kind;
    }
    nt++;
  };
  for (size_t l = 0; l < ls.size(); l++) {
    const bine::SegLaunch &L = ls[l];
    for (int s = 0; s < L.nseg; s++) {
      const uint64_t k = (uint64_t)L.seg[s], head = L.head[s], nvec = L.nvec[s];
      const uint64_t tail = bytes[k] - head - 16 * nvec;
      if (head) put(l, k, 0, head, 1);
      for (uint64_t v = 0; v < nvec; v += bine::kCopyTileVecs)
        put(l, k, head + 16 * v, 16 * std::min<uint64_t>(bine::kCopyTileVecs, nvec - v), 0);
      if (tail) put(l, k, head + 16 * nvec, tail, 1);
    }
  }
  return nt;
}
