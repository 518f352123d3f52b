// bine_internal.h -- shared declarations of libbine_amd.so (not installed).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "bine_amd.h"

// what the host planners and the kernels both evaluate (kernels.hip is HIP, every other unit plain C++)
#if defined(__HIPCC__)
#define BINE_HOST_DEVICE __attribute__((host)) __attribute__((device))
#else
#define BINE_HOST_DEVICE
#endif

namespace bine {

// ---- schedule (schedule.cpp) ------------------------------------------------

// One primitive of a per-rank plan (same layout as bine_prim_t).
using Prim = bine_prim_t;

struct Plan {
  std::vector<Prim> prims;
  uint64_t tmp_elems[3] = {0, 0, 0};  // workspace per TMP buffer, elements
  int status = BINE_SUCCESS;          // non-success: the reference's error return
  bool scale_fused = false;           // scaled call: the flagged trees scale, no trailing SCALE
  bool wide_a = false;                // wide call without covering trees: status UNSUPPORTED, take path A
};

struct PlanArgs {
  int algo = -1;
  int P = 1, rank = 0;
  size_t count = 0;                 // allreduce / reduce
  std::vector<int> rcounts;         // reduce_scatter
  int root = 0;                     // reduce
  size_t esz = 4;
  size_t segsize = 0;               // bytes; segmented variant's segment
  bool in_place = false;
  // allreduce (remap / static / rabenseifner, power-of-two P): replace the
  // mirrored allgather by one exchange in which every rank sends its reduced
  // block to every other rank (one hop on every link of a fully connected
  // node); reduce_bine_bdw: the gather tree becomes one step into the root.
  // Pure data movement: result bits unchanged.
  bool flat_ag = false;
  // allreduce remap / static / segmented (power-of-two P), reduce_scatter
  // bine_{permute,send}_remap / bine_static, reduce_bine_bdw, 2 <= P <= 16:
  // replace the log2(P) reduce-scatter steps by one all-peers exchange in which
  // every rank sends each block straight to the rank that computes it, which
  // then evaluates the reference's reduction tree for that block over the P
  // contributions in one REDUCE_TREE (same operands, same association, same
  // operand order: result bits unchanged).  flat_chunk = pipelining chunk in
  // elements (0: one chunk): chunk k's transfer overlaps chunk k-1's tree.
  bool flat_rs = false;
  size_t flat_chunk = 0;
  // with flat_rs and flat_ag (allreduce): the allgather exchange cut with the
  // reduce-scatter's chunks, chunk k's results sent right after chunk k+1's
  // reduce-scatter exchange, so the outputs complete chunk by chunk (the staged
  // host-buffer pipeline copies each chunk back as soon as it is final).  Pure
  // data movement: result bits unchanged.
  bool flat_ag_chunked = false;
  // scaled call (bine_allreduce_scaled / bine_reduce_scatter_scaled): every
  // element of this rank's output is multiplied by the call's scale exactly
  // once.  Where the flat reduce-scatter's trees produce the final values
  // (flat_rs(): the per-block trees of the bandwidth allreduces and of the
  // reduce-scatters, the one-shot trees of allreduce_bine_lat /
  // _recursivedoubling) they carry BINE_PRIM_SCALED and scale in registers
  // before their store; whatever moves their output afterwards (the allgather
  // phase, the in-place copy) moves scaled data.  Everywhere else -- literal
  // schedules, the rings' folded chain, non-power-of-two P, multi-tree mode,
  // P = 1 -- the plan ends with one BINE_PRIM_SCALE over the rank's output.
  // Which of the two a call gets depends on (algorithm, P, counts, forms)
  // alone, never on the rank: no element is scaled twice or not at all.
  bool scaled = false;
  // wide call (bine_allreduce_wide / bine_reduce_scatter_wide), planned with
  // the 16-bit element size: the trees `scaled` would flag carry
  // BINE_PRIM_WIDE instead (binary32 in registers, the call's scale, one
  // narrowing) and Plan::scale_fused says that they cover the output -- path
  // B.  A plan without them is no wide plan: the caller takes path A.
  bool wide = false;
};

Plan make_plan(const PlanArgs &a);
void append_scale(Plan &p, const PlanArgs &a);  // the trailing SCALE of a scaled call (unless p.scale_fused)
void wide_or_path_a(Plan &p);  // a wide call's plan without covering trees: UNSUPPORTED + Plan::wide_a

// multi-tree mode (trees.cpp): P-1 relabelled instances on P-1 slices; status
// BINE_ERR_UNSUPPORTED when not applicable (only allreduce, P = 4 or 8)
int tree_count(int P);
const int *tree_relabel(int P, int k);  // virtual -> physical rank of instance k
Plan make_tree_plan(const PlanArgs &a);

// schedule math (libbine_utils.h restated for the planner)
int pi(int rank, int step, int P);
uint32_t remap_rank(uint32_t P, uint32_t rank);
uint32_t get_nu(uint32_t rank, uint32_t size);
int log2_ceil(int v);
bool is_pow2(int v);
void static_perm(int P, std::vector<int> &perm);

// ---- issue schedule (schedule.cpp) -------------------------------------------
// A plan turned into device work for two streams: exchange groups go to the
// comm stream, local primitives to the compute stream.  PIPELINE exchanges are
// cut into `chunk` element pieces, each feeding the matching piece of the
// following reduction.  `wait` = index of the op of the OTHER stream this op
// must wait for (the newest one touching overlapping memory), -1 = none; ops of
// one stream are ordered by the stream.

struct SOp {
  bool xchg;
  std::vector<Prim> prims;
  int64_t wait;
};

struct Schedule {
  std::vector<SOp> ops;
  bool c_join = false;        // comm stream waits for the caller's prior work
  int64_t final_wait = -1;    // op of the comm stream the caller's stream waits for at the end
  uint64_t stage_elems = 0;   // BINE_BUF_STAGE workspace (relay mode)
  int relayed_steps = 0;
  std::vector<char> signals;  // op i is waited on (by an op's `wait` or final_wait): record its event
};

struct SchedCfg {
  size_t chunk = 0;       // pipelining chunk, elements (0: none)
  bool in_place = false;
  size_t relay_min = 0;   // relay mode: smallest relayed part, elements (0: off)
};

// Host staging of a schedule (bine_allreduce_staged / bine_reduce_scatter_staged):
// the input buffer (SBUF, or RBUF in place) is copied host -> device piece by
// piece just before the first op that touches each piece, and the output
// (RBUF) device -> host piece by piece right after the op that writes it last.
// h2d[i] = input element ranges first touched by op i (copied before it);
// h2d_wait[i] = the newest op whose h2d batch op i must wait for (-1: none);
// d2h[i] = output element ranges op i writes last (copied after it).
using Ivl = std::pair<uint64_t, uint64_t>;  // [lo, hi) in elements
struct StageRanges {
  std::vector<std::vector<Ivl>> h2d, d2h;
  std::vector<int64_t> h2d_wait;
};
void stage_ranges(const Schedule &sc, bool in_place, StageRanges &out);

// issue.cpp.  `all` = the plans of every rank (same arguments, rank varied);
// needed only for relay mode (null: no relay).
void make_schedule(const Plan &plan, const std::vector<Plan> *all, int rank, const SchedCfg &cfg, Schedule &out);
void make_schedule(const Plan &plan, size_t chunk, bool in_place, Schedule &out);

// ---- transports (executor.cpp, direct.cpp) -------------------------------------
struct XSend { int peer; const void *ptr; size_t bytes; };
struct XRecv { int peer; void *ptr; size_t bytes; };

// ---- kernels (kernels.hip) ----------------------------------------------------
int launch_reduce(const void *a, const void *b, void *out, size_t count, int dtype, int op,
                  void *stream);   // out = b (op) a
// up to kMaxBatch windows in one launch; BINE_ERR_ARG if a window is not
// co-aligned mod 16 B (then launch them one by one)
constexpr int kMaxBatch = 8;
int launch_reduce_batch(int n, const void *const *a, const void *const *b, void *const *out, const size_t *count,
                        int dtype, int op, void *stream);
// out = the reduction tree over nl (2..kMaxLeaves, power of two) leaves in
// tree order:
// level by level (w = 1, 2, 4, ...) v[i] = v[i] (op) v[i + w] for i % 2w == 0
// (v[i + w] (op) v[i] at the levels whose bit is set in `swap`)
constexpr int kMaxLeaves = 16;
int launch_reduce_tree(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op, void *stream,
                       unsigned swap = 0);
// kernels.hip is compiled three times; the entry points above live in the
// BINE_OPSET=0 object and forward a (dtype, op) another object holds
// (kernels.hip owner_opset) to that object's twin below.  Each object picks
// its instantiation through the same with_dtype / with_op / with_nl
// dispatchers; a dtype an object does not hold is BINE_ERR_UNSUPPORTED there.
// BINE_OPSET=1: the logical / bitwise / loc ops and the pair and complex types
int launch_reduce_logic(const void *a, const void *b, void *out, size_t count, int dtype, int op, void *stream);
int launch_reduce_batch_logic(int n, const void *const *a, const void *const *b, void *const *out,
                              const size_t *count, int dtype, int op, void *stream);
int launch_reduce_tree_logic(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                             void *stream, unsigned swap);
// BINE_OPSET=2: BINE_FLOAT16 / BINE_BFLOAT16
int launch_reduce_h16(const void *a, const void *b, void *out, size_t count, int dtype, int op, void *stream);
int launch_reduce_batch_h16(int n, const void *const *a, const void *const *b, void *const *out,
                            const size_t *count, int dtype, int op, void *stream);
int launch_reduce_tree_h16(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                           void *stream, unsigned swap);
// out[i] = S(in[i]) (k_scale; in == out allowed) and the tree with S applied
// to its result in the same launch (k_reduce_tree_sc): float / double in the
// opset-0 compilation, float16 / bfloat16 in opset 2.  BINE_ERR_ARG unless
// bine_scale_valid(dtype, op).
int launch_scale(const void *in, void *out, size_t count, int dtype, double scale, void *stream);
int launch_scale_h16(const void *in, void *out, size_t count, int dtype, double scale, void *stream);
int launch_reduce_tree_scaled(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                              void *stream, unsigned swap, double scale);
int launch_reduce_tree_scaled_h16(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                                  void *stream, unsigned swap, double scale);
// wide (binary32-accumulating) reductions of float16 / bfloat16, opset 2 only:
// out32[i] = in16[i] exactly (k_widen), out16[i] = nearest-even(in32[i])
// (k_narrow), and the tree evaluated in binary32 with one multiplication by
// (float)scale and one narrowing before the store (k_reduce_tree_wide).
// BINE_ERR_ARG unless bine_wide_valid(dtype, op).
int launch_widen_h16(const void *in16, void *out32, size_t count, int dtype, void *stream);
int launch_narrow_h16(const void *in32, void *out16, size_t count, int dtype, void *stream);
int launch_reduce_tree_wide_h16(int nl, const void *const *leaf, void *out, size_t count, int dtype, int op,
                                void *stream, unsigned swap, double scale);
// copy_buffer on the device (k_copy); hipMemcpyAsync when src / dst are not
// co-aligned mod 16 B
int launch_copy(void *dst, const void *src, size_t bytes, void *stream);
// k_copy's cache policy: copies of at least min_bytes load their first
// keep_bytes with the default policy (they may stay in the Infinity Cache for
// the next copy of the same source), everything else non-temporally.
struct CopyKeep {
  uint64_t keep_bytes, min_bytes;
};
// the policy with BINE_COPY_KEEP_MIB = env (NULL: unset): a number of MiB >= 0,
// fractions allowed, replaces def_keep and applies to copies of every size
// (0: every load non-temporal); unset or not such a number: the defaults
inline CopyKeep copy_keep_policy(const char *env, uint64_t def_keep, uint64_t def_min) {
  if (!env || !*env) return {def_keep, def_min};
  char *end = nullptr;
  const double mib = strtod(env, &end);
  if (end == env || *end || !(mib >= 0.0)) return {def_keep, def_min};
  const double cap = 1099511627776.0;  // 2^40 MiB = 2^60 bytes: the conversion below stays in range
  return {(uint64_t)((mib < cap ? mib : cap) * 1048576.0), 0};
}
// k_copy's keep_vecs for a copy of `bytes` bytes with nvec whole vectors: never
// above nvec, 0 below the policy's size threshold
inline uint64_t copy_keep_vecs(uint64_t bytes, uint64_t nvec, const CopyKeep &p) {
  if (bytes < p.min_bytes) return 0;
  const uint64_t k = p.keep_bytes / 16;
  return k < nvec ? k : nvec;
}
// ---- the segment family (segments.cpp, kernels.hip: TileTable) ------------------
// Every call that walks a list of buffers is planned on the host (segments.cpp,
// no HIP) as LaunchTables -- up to N non-empty segments, one workgroup per tile
// of kCopyTileVecs 16-B vectors, at least one per segment -- and issued by
// kernels.hip, one launch each (the dispatch: TileTable's comment there).
constexpr int kSegsPerLaunch = BINE_COPY_SEGS_PER_LAUNCH;
constexpr uint64_t kCopyTileVecs = 2048;           // kBlock * kCopyU (kernels.hip asserts it)
constexpr uint64_t kSegMaxWgs = (1u << 24) - 1;    // workgroups of one launch (256 lanes each: below 2^32 lanes)
// A segment's split, the ONE definition planners and kernels share: the bytes
// before the first 16-B boundary at or after addr (all of them, if the segment
// ends first) and the whole vectors after those.
BINE_HOST_DEVICE inline uint64_t seg_head(uint64_t addr, uint64_t bytes) {
  const uint64_t h = (16 - (addr & 15)) & 15;
  return h < bytes ? h : bytes;
}
BINE_HOST_DEVICE inline uint64_t seg_nvec(uint64_t bytes, uint64_t head) { return (bytes - head) / 16; }
// one launch as a planner leaves it
template <int N>
struct LaunchTable {
  int nseg = 0;
  int seg[N];                  // the caller's segment (tensor) index per slot
  uint32_t tile0[N + 1] = {};  // first tile per slot; [nseg] = their number
};
// The preamble of every list entry: BINE_ERR_ARG if n is outside [0,
// BINE_MULTI_MAX] or, with n > 0, `sizes` or one of `lists` is NULL; otherwise
// the lists' pointers as the addresses the planners take, list i at addr[i * n].
inline int seg_list_addrs(int n, const size_t *sizes, std::initializer_list<const void *const *> lists,
                          std::vector<uint64_t> &addr) {
  if (n < 0 || n > BINE_MULTI_MAX || (n > 0 && !sizes)) return BINE_ERR_ARG;
  addr.clear();
  for (const void *const *l : lists) {
    if (n > 0 && !l) return BINE_ERR_ARG;
    for (int k = 0; k < n; k++) addr.push_back((uint64_t)(uintptr_t)l[k]);
  }
  return BINE_SUCCESS;
}
// segmented copy (bine_copy_segments): plan_seg_launches' launches, issued as
// k_copy_segs by launch_copy_segments
struct SegLaunch : LaunchTable<kSegsPerLaunch> {
  uint64_t head[kSegsPerLaunch];  // seg_head of the destination
  uint64_t nvec[kSegsPerLaunch];  // seg_nvec after it
};
// BINE_SUCCESS, or BINE_ERR_ARG (n out of range, a NULL array, a zero address
// with a non-zero size, more than kSegMaxWgs workgroups in one launch)
int plan_seg_launches(int n, const uint64_t *dst_addr, const uint64_t *src_addr, const size_t *bytes,
                      std::vector<SegLaunch> &out);
int launch_copy_segments(int n, void *const *dsts, const void *const *srcs, const size_t *bytes, void *stream);
// sharded copy (bine_copy_shards): all P shards of up to kSegsPerLaunch
// non-empty tensors per launch of k_copy_shards, between the flat layout
// (shard j of tensor k at flat[k] + j * bytes[k]) and the packed one (at
// packed + j * block_bytes + poff[k], poff = the prefix sum of bytes over the
// non-empty tensors).  Every shard of a tensor gets tps tiles, tps = what the
// shard with the most destination vectors needs (at least one); with T = the
// sum of tps over the launch's tensors the grid is P * T workgroups, shard
// major: workgroup t is tile t % T (of the tensors' concatenated tiles) of
// shard t / T, and copies nothing where that shard has fewer tiles.
constexpr int kShardMaxRanks = 64;  // the library's peer limit (dm::kMaxPeers)
struct ShardLaunch : LaunchTable<kSegsPerLaunch> {  // seg: tensors; tile0: tiles within one shard's T
  uint64_t poff[kSegsPerLaunch];                    // the tensor's shards' offset in a packed block
};
// the destination of shard j of a tensor (dir 0: packed, dir 1: flat), the
// expression k_copy_shards evaluates too; its split is seg_head / seg_nvec
inline uint64_t shard_dst(int dir, uint64_t packed, uint64_t block_bytes, uint64_t poff, uint64_t flat,
                          uint64_t bytes, uint64_t j) {
  return dir ? flat + j * bytes : packed + j * block_bytes + poff;
}
// BINE_SUCCESS, or BINE_ERR_ARG (n, nranks or dir out of range, a NULL array, a
// zero address with a non-zero size, a tensor that alone exceeds kSegMaxWgs
// workgroups); a launch ends early where the next tensor would pass kSegMaxWgs
int plan_shard_launches(int n, int nranks, int dir, uint64_t packed_addr, const uint64_t *flat_addr,
                        const size_t *bytes, std::vector<ShardLaunch> &out, uint64_t *block_bytes);
int launch_copy_shards(int n, int nranks, int dir, void *packed, void *const *flat, const size_t *bytes,
                       void *stream);
// segmented sum of squares and segmented scale (bine_sumsq_segments /
// bine_clip_segments): both walk the segmented copy's tile table with
// destination = source = the buffer (whole elements per vector).
// norm_esz: the element size of the four types the two calls take, 0 otherwise.
size_t norm_esz(int dtype);
// The checks of a list that need no device, in the header's order (dtype, n, a
// NULL array, a NULL buffer with a non-zero count, a buffer not aligned to its
// element), then the launches and their workgroups summed over the launches
// (`tiles`: the doubles of scratch bine_sumsq_segments needs).  BINE_SUCCESS or
// BINE_ERR_ARG.
int plan_norm_launches(int n, const uint64_t *addrs, const size_t *counts, int dtype, std::vector<SegLaunch> &out,
                       uint64_t *tiles);
// k_sumsq_segs per launch of `ls` (one double per workgroup into `scratch`, the
// launches' workgroups one after another); the opset-0 entry forwards the
// 16-bit types.  nt: non-temporal loads.
int launch_sumsq_tiles(const std::vector<SegLaunch> &ls, const void *const *bufs, const size_t *counts, int dtype,
                       double *scratch, bool nt, void *stream);
int launch_sumsq_tiles_h16(const std::vector<SegLaunch> &ls, const void *const *bufs, const size_t *counts,
                           int dtype, double *scratch, bool nt, void *stream);
// bine_sumsq_segments: the checks, launch_sumsq_tiles, then k_sumsq_fold per
// launch (a segment's partials -> out[k]) and one k_sumsq_total (the empty
// segments' zeros and out[n])
int launch_sumsq_segments(int n, const void *const *bufs, const size_t *counts, int dtype, double *out,
                          double *scratch, size_t scratch_doubles, void *stream);
// bine_clip_segments: k_scale_segs per launch of the same table, in place
int launch_clip_segments(int n, void *const *bufs, const size_t *counts, int dtype, const double *norm2,
                         double max_norm, double eps, double *coef_out, void *stream);
int launch_clip_segments_h16(int n, void *const *bufs, const size_t *counts, int dtype, const double *norm2,
                             double max_norm, double eps, double *coef_out, void *stream);
// fused AdamW step over a list of shards (bine_adamw_segments, k_adamw_segs):
// plan_norm_launches' table over p as BINE_FLOAT -- the same tiles, the same
// first-workgroup rule -- cut into launches of at most kAdamwSegsPerLaunch
// descriptors (five pointers and a count each: 128 would not fit the 4 KiB of
// by-value arguments), tile0 rebased to each launch's first segment.
constexpr int kAdamwSegsPerLaunch = BINE_ADAMW_SEGS_PER_LAUNCH;
static_assert(kSegsPerLaunch % kAdamwSegsPerLaunch == 0 && kAdamwSegsPerLaunch <= 64,
              "a SegLaunch splits into whole AdamW launches; AdamwLaunch::elem has one bit per slot");
struct AdamwLaunch : LaunchTable<kAdamwSegsPerLaunch> {
  uint64_t elem = 0;  // bit s: slot s takes the element body
};
// the element size of the three types g and pout take (float, float16,
// bfloat16), 0 otherwise
size_t adamw_esz(int dtype);
// The checks of the five lists that need no device, in the header's order, then
// the launches.  pout NULL: no 16-bit copy.  BINE_SUCCESS or BINE_ERR_ARG.
int plan_adamw_launches(int n, const uint64_t *p, const uint64_t *m, const uint64_t *v, const uint64_t *g,
                        const uint64_t *pout, const size_t *counts, int gdtype, int odtype,
                        std::vector<AdamwLaunch> &out);
// every check of bine_adamw_segments, nothing launched (bine_adamw_multi runs
// it before it looks at its communicator)
int adamw_args(int n, void *const *p, void *const *m, void *const *v, const void *const *g, void *const *pout,
               const size_t *counts, int gdtype, int odtype, double lr, double beta1, double beta2, double eps,
               double weight_decay, int64_t step, const double *gcoef, double grad_mul, float consts[8],
               std::vector<AdamwLaunch> *ls);
// bine_adamw_segments: adamw_args, then k_adamw_segs per launch (kernels_h16.o:
// the compilation that holds the 16-bit conversions)
int launch_adamw_segments_h16(int n, void *const *p, void *const *m, void *const *v, const void *const *g,
                              void *const *pout, const size_t *counts, int gdtype, int odtype, double lr,
                              double beta1, double beta2, double eps, double weight_decay, int64_t step,
                              const double *gcoef, double grad_mul, void *stream);

// dynamic loss scaling (bine_step_update, bine_adamw_segments_dyn): the state
// block of bine_amd.h as a struct, and its update rule -- ONE statement for the
// host twin (segments.cpp: plain C++) and for k_step_update (kernels.hip:
// thread 0).  Every operation is binary64 and correctly rounded, one per
// expression node; both compilations pass -ffp-contract=off, so no product
// folds into a sum.  tests/step_sim.py restates it in numpy.
struct StepState {
  double d[8];  // scale, good, step, pw1, pw2, skip, gm, skipped
  float c[8];   // bine_adamw_consts' order
};
static_assert(sizeof(StepState) == BINE_STEP_STATE_BYTES && alignof(StepState) == 8, "bine_amd.h's layout");
BINE_HOST_DEVICE inline void step_update_rule(StepState *s, double n2, const bine_step_hyper &h) {
  double scale = s->d[0];
  if (!(n2 <= 1.7976931348623157e308)) {  // +inf or NaN: some element on some rank was not finite
    s->d[5] = 1.0;
    s->d[6] = 0.0;
    s->d[7] = s->d[7] + 1.0;
    s->d[1] = 0.0;
    scale = scale * h.backoff_factor;
    s->d[0] = scale > h.min_scale ? scale : h.min_scale;
    return;
  }
  const double inv = 1.0 / scale;
  const double nrm = __builtin_sqrt(n2) * inv;
  const double r = h.max_norm / (nrm + h.clip_eps);
  const double cc = r < 1.0 ? r : 1.0;  // a NaN r gives 1.0, as bine_clip_segments
  s->d[6] = cc * inv;
  s->d[2] = s->d[2] + 1.0;
  const double pw1 = s->d[3] * h.beta1, pw2 = s->d[4] * h.beta2;
  s->d[3] = pw1;
  s->d[4] = pw2;
  s->c[0] = (float)(1.0 - h.lr * h.weight_decay);
  s->c[1] = (float)h.beta1;
  s->c[2] = (float)(1.0 - h.beta1);
  s->c[3] = (float)h.beta2;
  s->c[4] = (float)(1.0 - h.beta2);
  s->c[5] = (float)(1.0 / __builtin_sqrt(1.0 - pw2));
  s->c[6] = (float)h.eps;
  s->c[7] = (float)(h.lr / (1.0 - pw1));
  s->d[5] = 0.0;
  const double good = s->d[1] + 1.0;
  if (good >= (double)h.growth_interval) {
    scale = scale * h.growth_factor;
    s->d[0] = scale < h.max_scale ? scale : h.max_scale;
    s->d[1] = 0.0;
  } else {
    s->d[1] = good;
  }
}
// the hyper-parameters' refusals, then state / norm2 NULL or not 8-byte aligned
// (bine_step_update_host: norm2 is a value, pass any aligned non-NULL address)
int step_update_args(const void *state, const void *norm2, const bine_step_hyper *h);
// bine_step_update: step_update_args, then one launch of k_step_update
int launch_step_update_h16(void *state, const double *norm2, const bine_step_hyper *h, void *stream);
// bine_adamw_segments_dyn's checks: adamw_args' list checks, then the state
// pointer (NULL or not 8-byte aligned)
int adamw_dyn_args(int n, void *const *p, void *const *m, void *const *v, const void *const *g, void *const *pout,
                   const size_t *counts, int gdtype, int odtype, const void *state, std::vector<AdamwLaunch> *ls);
// bine_adamw_segments_dyn: adamw_dyn_args, then k_adamw_segs' DYN form per launch
int launch_adamw_segments_dyn_h16(int n, void *const *p, void *const *m, void *const *v, const void *const *g,
                                  void *const *pout, const size_t *counts, int gdtype, int odtype, const void *state,
                                  void *stream);

// FP8 quantization of a list of tensors (bine_amax_segments, bine_fp8_scales,
// bine_quant_segments, bine_dequant_segments; kernels_h16.o).
// The scale rule of bine_amd.h -- ONE statement for the host twin
// (bine_fp8_scale_host, segments.cpp) and for k_fp8_scales (kernels.hip), in
// integer arithmetic on the pattern; tests/fp8_sim.py restates it with frexp.
constexpr int fp8_fe(int fmt) { return fmt == BINE_FP8_E4M3 ? 9 : 16; }  // FMAX = 0.875 * 2^fe
inline bool fp8_fmt_ok(int fmt) { return fmt == BINE_FP8_E4M3 || fmt == BINE_FP8_E5M2; }
BINE_HOST_DEVICE inline void fp8_scale_rule(uint32_t bits, int fmt, float *scale, float *inv) {
  int e = 0;
  if (bits != 0 && bits < 0x7f800000u) {
    // the value as f * 2^x, f = 1.frac / 2 in [0.5, 1)
    const uint32_t ex = bits >> 23, man = bits & 0x7fffffu;
    int x;
    uint32_t frac;
    if (ex) {
      x = (int)ex - 126;
      frac = man;
    } else {  // subnormal: man * 2^-149 with its leading one at bit p
      const int p = 31 - __builtin_clz(man);
      x = p - 148;
      frac = (man << (23 - p)) & 0x7fffffu;
    }
    e = fp8_fe(fmt) - x - (frac > 0x600000u ? 1 : 0);  // f > 0.875
    e = e < -126 ? -126 : e > 126 ? 126 : e;
  }
  const uint32_t sb = (uint32_t)(127 + e) << 23, ib = (uint32_t)(127 - e) << 23;
  __builtin_memcpy(scale, &sb, 4);
  __builtin_memcpy(inv, &ib, 4);
}
// k_quant_segs, both directions: plan_norm_launches' table over the WIDE side
// (the source of a quantization, the destination of a dequantization) -- the
// same tiles, the same first-workgroup rule -- with one flag per slot
struct QuantLaunch : LaunchTable<kSegsPerLaunch> {
  uint64_t elem[(kSegsPerLaunch + 63) / 64] = {};  // bit s: slot s takes the element body
};
// k_amax_segs: the same table with kAmaxTilesPerWg consecutive tiles of a slot
// per workgroup (tile0 counts workgroups: ceil(tiles / kAmaxTilesPerWg) per
// slot).  Every workgroup ends in a look at out[k] and, where it holds a new
// maximum, an atomic on that one address; atomics on one address serialise,
// and with a workgroup per tile the thousands that end together before any
// maximum is visible cost 20 us on a 256 MiB tensor (tools/amax_variants.hip,
// DESIGN.md 6.9).
constexpr uint32_t kAmaxTilesPerWg = BINE_AMAX_TILES_PER_WG;
using AmaxLaunch = LaunchTable<kSegsPerLaunch>;
AmaxLaunch amax_launch_of(const LaunchTable<kSegsPerLaunch> &tiles);
// the body flags of `ls` (plan_quant_launches' tables of `wide`) for another byte side
void quant_set_bodies(std::vector<QuantLaunch> &ls, const void *const *wide, const void *const *bytes8, int dtype);
// The checks of the two lists that need no device, in the header's order (dtype
// through the source's alignment), then the launches.  With h = the elements
// before wide's first 16-B boundary a slot takes the vector body where bytes8
// + h is aligned to 16 / esz bytes (what one wide vector holds in FP8).
int plan_quant_launches(int n, const uint64_t *wide, const uint64_t *bytes8, const size_t *counts, int dtype,
                        std::vector<QuantLaunch> &out);
// Every check of the four entry points, nothing launched; BINE_SUCCESS or
// BINE_ERR_ARG with *why = what was refused.  ls: the launches, where given.
int amax_args(int n, const void *const *bufs, const size_t *counts, int dtype, const void *out, const char **why,
              std::vector<AmaxLaunch> *ls);
int fp8_scales_args(int n, const void *amax, int fmt, const void *scales, const char **why);
// wide / bytes8: src / dst8 of bine_quant_segments, dst / src8 of bine_dequant_segments
int quant_args(int n, const void *const *wide, const void *const *bytes8, const size_t *counts, int dtype, int fmt,
               const void *scales, const char **why, std::vector<QuantLaunch> *ls);
// the launches themselves (arguments checked by the functions above)
int launch_amax_segments_h16(const std::vector<AmaxLaunch> &ls, int n, const void *const *bufs, const size_t *counts,
                             int dtype, uint32_t *out, void *stream);
int launch_fp8_scales_h16(int n, const uint32_t *amax, int fmt, float *scales, void *stream);
int launch_quant_segments_h16(const std::vector<QuantLaunch> &ls, const void *const *src, void *const *dst8,
                              const size_t *counts, int sdtype, int fmt, const float *scales, void *stream);
int launch_dequant_segments_h16(const std::vector<QuantLaunch> &ls, const void *const *src8, void *const *dst,
                                const size_t *counts, int ddtype, int fmt, const float *inv_scales, void *stream);

// MX block-scaled quantization of a list of tensors (bine_mx_quant_segments,
// bine_mx_dequant_segments; kernels_h16.o): 32 elements share one E8M0 byte.
// The scale rule of bine_amd.h -- ONE statement for the host twin
// (bine_mx_scale_host, segments.cpp) and for k_mx_segs (kernels.hip), in
// integer arithmetic on the pattern; tests/mx_sim.py restates it with frexp.
constexpr int kMxBlock = 32;
BINE_HOST_DEVICE constexpr int mx_emax(int fmt) { return fmt == BINE_MX_E4M3 ? 8 : fmt == BINE_MX_E5M2 ? 15 : 2; }
inline bool mx_fmt_ok(int fmt) { return fmt == BINE_MX_E4M3 || fmt == BINE_MX_E5M2 || fmt == BINE_MX_E2M1; }
// the data bytes of `count` elements: one each, or two per byte for E2M1
BINE_HOST_DEVICE inline uint64_t mx_dbytes(uint64_t count, int fmt) {
  return fmt == BINE_MX_E2M1 ? (count + 1) / 2 : count;
}
// A: the block's largest bits(widen(x)) & 0x7fffffff
BINE_HOST_DEVICE inline uint8_t mx_scale_rule(uint32_t A, int fmt) {
  if (A >= 0x7f800000u) return 0xff;  // an inf or a NaN in the block
  if (A == 0) return 0;
  // E = floor(log2 |max|); a subnormal is man * 2^-149 with its leading one at bit p
  const int E = (A >> 23) ? (int)(A >> 23) - 127 : (31 - __builtin_clz(A)) - 149;
  const int S = E - mx_emax(fmt) + 127;
  return (uint8_t)(S < 0 ? 0 : S);
}
// k_mx_segs, both directions: tiles of kCopyTileVecs * 16 bytes of the WIDE
// side counted from the segment's FIRST ELEMENT (blocks are, so a tile is whole
// blocks), at least one per non-empty segment, with one body flag per slot.
constexpr int kMxSegsPerLaunch = BINE_MX_SEGS_PER_LAUNCH;
struct MxLaunch : LaunchTable<kMxSegsPerLaunch> {
  uint64_t elem[(kMxSegsPerLaunch + 63) / 64] = {};  // bit s: slot s takes the element body
};
// the body of one segment: 0 vector -- wide on a 16-B boundary and data8 on a
// boundary of the bytes one wide vector yields -- or 1 element
inline int mx_body(uint64_t wide, uint64_t data8, size_t esz, int fmt) {
  return wide % 16 || data8 % mx_dbytes(16 / esz, fmt) ? 1 : 0;
}
// the body flags of `ls` for other addresses of the same counts
void mx_set_bodies(std::vector<MxLaunch> &ls, const void *const *wide, const void *const *data8, int dtype, int fmt);
// The checks of the three lists that need no device, in the header's order
// (dtype and fmt through the wide side's alignment), then the launches.
int plan_mx_launches(int n, const uint64_t *wide, const uint64_t *data8, const uint64_t *scl8, const size_t *counts,
                     int dtype, int fmt, std::vector<MxLaunch> &out);
// Every check of the two entry points, nothing launched; BINE_SUCCESS or
// BINE_ERR_ARG with *why = what was refused.  wide / data8: src / dst8 of
// bine_mx_quant_segments, dst / src8 of bine_mx_dequant_segments.
int mx_args(int n, const void *const *wide, const void *const *data8, const void *const *scl8, const size_t *counts,
            int dtype, int fmt, const char **why, std::vector<MxLaunch> *ls);
// bine_mx_quant_multi's checks that need no communicator and no algorithm id:
// mx_args with params8 / scales8 standing for the slots, then the shard counts
int mx_multi_args(int n, void *const *params8, void *const *scales8, const void *const *src,
                  const size_t *shard_counts, int sdtype, int fmt, const char **why, std::vector<MxLaunch> *ls);
int launch_mx_quant_segments_h16(const std::vector<MxLaunch> &ls, const void *const *src, void *const *dst8,
                                 void *const *scl8, const size_t *counts, int sdtype, int fmt, void *stream);
int launch_mx_dequant_segments_h16(const std::vector<MxLaunch> &ls, const void *const *src8, const void *const *scl8,
                                   void *const *dst, const size_t *counts, int ddtype, int fmt, void *stream);
// The wire layout of a bucket (bine_mx_wire_bytes): per tensor its data offset
// in a block and its scale offset (D + the prefix sum of counts / 32), then D
// and B.  BINE_ERR_ARG for fmt, n < 0, counts NULL with n > 0, a count not a
// multiple of 32, a sum that overflows.  off: 2n entries (data, then scale), or NULL.
int mx_wire_layout(int n, const size_t *counts, int fmt, std::vector<uint64_t> *off, uint64_t *data_bytes,
                   uint64_t *block_bytes);
// k_mx_sum_segs: plan_mx_launches' table over the DESTINATION (the same tiles,
// whole blocks from the segment's first element) with the body flag of dst
// alone -- a block's data offsets are multiples of 16 and `packed` is 16-B
// aligned -- then the counts' multiples of 32.
constexpr int kMxSumMaxStreams = BINE_MX_SUM_MAX_STREAMS;
int plan_mx_sum_launches(int n, const uint64_t *dst, const size_t *counts, int ddtype, int fmt,
                         std::vector<MxLaunch> &out);
// Every check of bine_mx_sum_segments in the header's order, nothing launched;
// ls: the launches, off: mx_wire_layout's offsets, where given.
int mx_sum_args(int n, int nstreams, const void *packed, size_t block_bytes, void *const *dst, const size_t *counts,
                int ddtype, int fmt, const char **why, std::vector<MxLaunch> *ls, std::vector<uint64_t> *off);
// bine_mx_reduce_scatter_multi's checks that need no communicator and no
// algorithm id, in the header's order, for a communicator of P ranks; *block =
// B (0: every count is 0, the workspaces were not looked at)
int mx_rs_args(int P, int n, const void *const *sbufs, void *const *rbufs, const size_t *shard_counts, int sdtype,
               int rdtype, int fmt, const void *send_ws, const void *recv_ws, size_t ws_bytes, const char **why,
               uint64_t *block, std::vector<uint64_t> *off);
int launch_mx_sum_segments_h16(const std::vector<MxLaunch> &ls, const std::vector<uint64_t> &off, int n, int nstreams,
                               const void *packed, size_t block_bytes, void *const *dst, const size_t *counts,
                               int ddtype, int fmt, float scale, void *stream);
// k_mx_ef_segs (bine_mx_quant_ef_segments): plan_mx_launches' table over the
// source -- the same tiles -- cut at kMxEfSegsPerLaunch descriptors (four
// pointers and a count: 112 would not fit the 4 KiB of by-value arguments).
// The vector body needs what mx_body asks of the source and data8, and res on
// a 16-B boundary.
constexpr int kMxEfSegsPerLaunch = BINE_MX_EF_SEGS_PER_LAUNCH;
struct MxEfLaunch : LaunchTable<kMxEfSegsPerLaunch> {
  uint64_t elem[(kMxEfSegsPerLaunch + 63) / 64] = {};  // bit s: slot s takes the element body
};
inline int mx_ef_body(uint64_t src, uint64_t res, uint64_t data8, size_t esz, int fmt) {
  return mx_body(src, data8, esz, fmt) || res % 16 ? 1 : 0;
}
// The checks of the four lists that need no device, in the header's order
// (dtype and fmt through the residual's alignment), then the launches.
int plan_mx_ef_launches(int n, const uint64_t *src, const uint64_t *res, const uint64_t *data8, const uint64_t *scl8,
                        const size_t *counts, int dtype, int fmt, std::vector<MxEfLaunch> &out);
// Every check of bine_mx_quant_ef_segments, nothing launched; ls: the launches, where given.
int mx_ef_args(int n, const void *const *src, const void *const *res, const void *const *data8,
               const void *const *scl8, const size_t *counts, int dtype, int fmt, const char **why,
               std::vector<MxEfLaunch> *ls);
// bine_mx_reduce_scatter_multi_ef's checks that need no communicator and no
// algorithm id: mx_rs_args' in its order, with res beside sbufs
int mx_ef_rs_args(int P, int n, const void *const *sbufs, const void *const *res, void *const *rbufs,
                  const size_t *shard_counts, int sdtype, int rdtype, int fmt, const void *send_ws,
                  const void *recv_ws, size_t ws_bytes, const char **why, uint64_t *block,
                  std::vector<uint64_t> *off);
int launch_mx_quant_ef_segments_h16(const std::vector<MxEfLaunch> &ls, const void *const *src, void *const *res,
                                    void *const *dst8, void *const *scl8, const size_t *counts, int sdtype, int fmt,
                                    void *stream);
int launch_fill_pico(void *buf, size_t count, int dtype, uint32_t seed, void *stream);

// direct peer-memory transport (direct.cpp): one launch moves up to kMaxDm
// messages, `wgs` workgroups each (k_dm_move).  Sequence numbers live in the
// device (per peer and direction, in the rank's own inbox) and every address
// and flag is derived from them in the kernel, so launches carry no host-side
// state and can be captured into a graph and replayed.
constexpr int kMaxDm = 32;
// the inbox layout (bytes from its base): flags region, then the data slots
namespace dm {
constexpr size_t kFlagStride = 128;  // one flag / counter per 128-B line
constexpr size_t kReadyOff = 0, kAckOff = 64 << 10, kCntPushOff = 128 << 10, kCntPullOff = 192 << 10,
                 kPoisonOff = 256 << 10, kBaseSendOff = 260 << 10, kBaseRecvOff = 264 << 10,
                 kLaunchCntOff = 268 << 10, kPeerTabOff = 272 << 10, kPingOff = 288 << 10,
                 kGeomOff = 296 << 10;
// Slice flags of k_dm_fused (round 6): workgroup w of a launch of `wgs`
// workgroups owns slice w of every message (slice(): [n w / wgs, n (w+1) / wgs)
// of its n vectors), so a receiver's workgroup w needs only the SENDER's
// workgroup w to be done with slice w, not the whole message.  Per (ordered
// pair, slot, slice) a ready flag (in the receiver's inbox, set by the sender's
// workgroup w after its stores of slice w were acknowledged) and an ack flag
// (in the sender's inbox, set by the receiver's workgroup w after its reads of
// slice w completed); value = seq << kSliceWgsBits | wgs of the setter's launch
// -- a slice flag stands for slice w only when both ends cut the message with
// the same wgs (the message sizes match by construction).  The whole-message
// flags are still published (the last arriver), so a peer issuing another
// form waits on those.  kGeomOff: per (peer, slot) the sequence number and
// vector count of this rank's last k_dm_fused push into that slot (local), so
// a push can tell whether the receiver's slice acks of the slot's previous use
// cover the bytes it is about to overwrite.
// Layout [w][x][k]: one 128-B line per (slice w, pair x) holds that pair's
// kSlots flags of slice w -- written only by one sender workgroup, polled
// only by one receiver workgroup (flags of different workgroups in one line
// made the phases contend for it: C3 at P = 2 0.385 -> 0.412 ms).
constexpr int kSliceMax = 1024, kSliceWgsBits = 12;
constexpr size_t kSliceLine = 128;
constexpr size_t kSliceReadyOff = 320 << 10,
                 kSliceAckOff = kSliceReadyOff + (size_t)kSliceMax * 64 * kSliceLine,   // x kMaxPeers
                 kFlagsBytes = kSliceAckOff + (size_t)kSliceMax * 64 * kSliceLine;
// the slice flag of (slice w, pair x, slot k) from a region's base
constexpr size_t slice_off(size_t w, size_t x, size_t k) { return (w * 64 + x) * kSliceLine + k * 8; }
constexpr int kSlots = 4;      // slots per ordered pair
constexpr int kMaxPeers = 64;  // P limit of the layout (flag regions: P * kSlots * 128 B <= 64 KiB)
static_assert(kSliceAckOff - kSliceReadyOff == (size_t)kMaxPeers * kSliceMax * kSliceLine &&
                  kFlagsBytes - kSliceAckOff == (size_t)kMaxPeers * kSliceMax * kSliceLine &&
                  kSlots * 8 <= kSliceLine &&
                  kGeomOff + (size_t)kMaxPeers * kSlots * 16 <= kSliceReadyOff && kFlagsBytes % 4096 == 0,
              "inbox layout");
}  // namespace dm
struct DmMsg {
  const uint8_t *src;  // push: the data to send (pull: unused -- the slot)
  uint8_t *dst;        // pull: where the data goes (push: unused -- the peer's slot)
  uint64_t bytes;
  int push;            // 1: into the peer's inbox, 0: out of our own
  int peer;
  int j;               // this launch's j-th message of this kind to / from `peer`: seq = base[peer] + j + 1
  int leaf = -1;       // k_dm_move_tree: >= 0 -- a pull whose slot is a leaf of the launch's tree (read in
                       // place, never copied); -1 -- copied by its own workgroups
  int grp = -1;        // a push of the same bytes to several peers: index in m of the group's leader, whose
                       // workgroups read the source once and store it into every member's slot; -1: alone
};
// Residency: every workgroup of a direct-transport launch
// may wait on a flag that a workgroup of a peer's launch sets.  A launch whose
// workgroups cannot all be resident at once -- together with the launches of
// the other `share` ranks on the same GPU -- can fill the chip with waiters
// whose producers never get a slot: a residency stall (the hardware
// scheduler's time slicing resolves it slowly, or a wait times out).  So every
// launch is cut to fit: its workgroups (each copy entry's cwgs, the tree's
// twgs, the fused kernel's wgs) are scaled so that they sum to at most
// cap = CUs x (resident blocks per CU of the kernel (hipOccupancy...) - margin)
// / share (dm_residency_cap).  The margin (one workgroup per CU,
// BINE_DIRECT_RESIDENCY_MARGIN) is what any other wave on the GPU may hold
// while the spinning ones hold theirs: with 8 ranks on one GPU at the exact
// cap (8 x 160 = 1,280 = 256 CUs x 5) a producer's last workgroups got a slot
// only after the first waiter timed out.
// dm_fit_residency: scale `cw[0..n)` and *tw (null: none) proportionally,
// each >= 1, to sum <= cap.  0: unchanged (already fits or cap <= 0),
// 1: scaled, -1: n parts (+ the tree) alone exceed cap (left unchanged).
int dm_fit_residency(int *cw, int n, int *tw, int cap);
// the cap from the device's CUs, the kernel's resident blocks per CU, the
// margin (blocks per CU left free; never below one resident block per CU)
// and the ranks sharing the GPU; 0 when unknown (cus or per_cu <= 0)
inline int dm_residency_cap(int cus, int per_cu, int margin, int share) {
  if (cus <= 0 || per_cu <= 0) return 0;
  const int per = per_cu - margin >= 1 ? per_cu - margin : 1;
  return cus * per / (share >= 1 ? share : 1);
}
// the cap itself on the current device: kind 0 k_dm_move, 1 k_dm_move_tree for
// (dtype, op, nl), 2 k_dm_fused for (dtype, op); -1: no such kernel, 0: unknown
int dm_launch_cap(int kind, int dtype, int op, int nl, int share);
struct DmArgs {
  int nmsg = 0;
  int wgs = 1;
  int rank = 0;
  int share = 1;                   // ranks of this transport on this GPU (the residency cap's divisor)
  uint64_t slot = 0;               // bytes per slot
  uint8_t *own = nullptr;          // this rank's inbox (flags, counters, sequence bases, peer table)
  uint32_t *poison_host = nullptr; // mapped host word set together with the inbox's poison word
  uint64_t timeout_ticks = 0;      // wall_clock64 ticks
  DmMsg m[kMaxDm];
  int ncopy = 0;                   // messages with workgroups of their own (standalone copies, group leaders):
  int cidx[kMaxDm] = {};           // indices into m, in dispatch order,
  int cwgs[kMaxDm] = {};           // and their workgroups (wgs; wgs x members for a group)
  int ncw = 0;                     // sum of cwgs: the copy workgroups of the launch
  // diagnostics (BINE_DIRECT_STAMPS): per-workgroup wall_clock64 stamps of
  // entry / wait done / copy done, appended to `stamps` (dm::Stamp layout);
  // null: off
  uint64_t *stamps = nullptr;
  uint32_t serial = 0;             // the launch's number (host-side count)
};
namespace dm {
// stamps buffer: [0] records written (atomic), [1] capacity (records), then
// records of 4 words: tag = serial << 32 | kind << 24 | msg << 16 | wg, and the
// workgroup's wall_clock64 at entry, when its wait ended, when its copy (or
// tree) ended.  kind: 0 push, 1 pull, 2 tree, 3 push group
constexpr int kStampHdr = 8, kStampWords = 4;
// The mapped host words (DirectState::hpoison, kHostBytes): word 0's low half
// is the poison flag; 64-bit words kRecFirst .. kRecFirst + kRecWords - 1 hold
// the first timed-out waiter's record (dm_time_out, kernels.hip): kind << 8 |
// phase, rank, peer, slot, sequence number wanted, flag value last seen,
// launch serial, workgroup << 16 | thread, wall_clock64 ticks waited
constexpr int kRecFirst = 1, kRecWords = 9;
constexpr size_t kHostBytes = 128;
// what the waiter was: a push waits for the receiver's acknowledgement of the
// slot's previous use, a pull / leaf for the sender's ready mark
enum WaitKind : uint32_t {
  kWaitMovePush = 1,   // k_dm_move push
  kWaitMovePull = 2,   // k_dm_move pull
  kWaitGroupPush = 3,  // k_dm_move push group (BINE_DIRECT_MCAST)
  kWaitTreeLeaf = 4,   // k_dm_move_tree leaf
  kWaitFusedPush = 5,  // k_dm_fused push (phase 0: A, 1 + c: the allgather pieces of tree c)
  kWaitFusedPull = 6,  // k_dm_fused leaf (phase 1 + c) or allgather pull (phase 15: D)
  kWaitPing = 7,       // k_dm_ping (bine_comm_direct_ping): the peer's answer
};
}  // namespace dm
int launch_dm_move(const DmArgs &a, void *stream);

// The flag latency probe (k_dm_ping, bine_comm_direct_ping): ping flags at
// dm::kPingOff + x * kFlagStride of the inbox of rank y, written by rank x
// (monotonic: sequence numbers base + 1 .. base + iters, base = the pair's
// earlier pings, counted on the host by both ranks alike)
struct DmPingArgs {
  uint8_t *own = nullptr;
  uint32_t *poison_host = nullptr;
  uint64_t timeout_ticks = 0;
  uint64_t base = 0;
  uint64_t *out = nullptr;  // device word: wall_clock64 ticks of round trips 2 .. iters (0: timed out)
  int rank = 0, peer = 0, iters = 0, initiator = 0;
  uint32_t serial = 0;
};
int launch_dm_ping(const DmPingArgs &a, void *stream);

// The flat reduce-scatter's tree evaluated INSIDE the exchange launch that
// receives its leaves (k_dm_move_tree<T, OP, NL>): the launch's copy messages
// (pushes, and pulls that are not leaves) run as in k_dm_move on their
// `wgs` workgroups each; `twgs` further workgroups wait for the leaf pulls'
// ready marks, evaluate the reference's tree (own leaf at `pos`, per-level
// swap bits) reading the received leaves in place in the inbox slots, write
// `out`, and acknowledge every leaf slot -- the pull copy into a staging area
// and the separate tree launch of the unfused form are gone (one HBM pass
// over every received byte less).  Slots, flags, counters and sequence bases
// are k_dm_move's; a leaf pull is counted and acknowledged like a copied one,
// so both ends see the same protocol.
struct DmTree {
  int nl = 0, pos = 0;
  unsigned swap = 0;
  int twgs = 0;                 // tree workgroups (dispatched after the copy workgroups, DmArgs::cidx)
  int leaf_msg[kMaxLeaves] = {};  // tree position -> DmArgs::m index (-1 at pos)
  const void *own_leaf = nullptr;
  void *out = nullptr;
  uint64_t nvec = 0;            // 16-B vectors per leaf and of `out`
};
// BINE_ERR_UNSUPPORTED: no instantiation for (dtype, op, nl) -- the caller
// issues the unfused form
int launch_dm_move_tree(const DmArgs &a, const DmTree &t, int dtype, int op, void *stream);
bool dm_tree_supported(int dtype, int op, int nl);

// A whole flat-form collective in ONE launch over the direct transport
// (k_dm_fused): phase A pushes this rank's blocks (every chunk) into the
// peers' inboxes; then for each chunk c, phase B_c waits for the peers' blocks
// of that chunk and evaluates the reference's reduction tree (the
// REDUCE_TREE primitive: own leaf at `pos`, the received blocks read straight
// out of the inbox slots, `swap` per level) into its `out`, pushing each
// result vector from registers into the peers' slots (the flat allgather's
// piece c); phase D copies the peers' results out of the inbox (absent for
// the one-shot latency form and for reduce-scatters).  Workgroup w handles
// the same 1/wgs slice of every message in every phase, so a workgroup only
// ever reads back what it wrote itself: no grid-wide barrier.  Every wait
// is for a flag that a peer sets in an EARLIER phase, and every workgroup of
// every rank's launch is resident (the residency cut), so the phases
// complete in order.  Messages use the same slots, flags, counters and
// device-side sequence bases as k_dm_move (j = the message's index among
// this launch's messages of its kind to / from its peer, < kSlots: no slot
// is used twice in one launch).
constexpr int kMaxFusedPeers = 15;  // P <= 16
constexpr int kMaxFusedTrees = 4;   // chunks of the tree phase
constexpr int kMaxFusedMsgs = 4 * kMaxFusedPeers;
struct DmFusedTree {
  const void *own_leaf = nullptr;
  void *out = nullptr;
  uint64_t nvec = 0;                   // 16-B vectors per leaf / of out
  int b0 = 0, nb = 0, nc = 0;          // leaves m[b0, b0 + nb), then the pushes of out m[b0 + nb, b0 + nb + nc)
  int8_t leaf[kMaxLeaves] = {};        // leaf j != pos: index in m of the pull carrying it
};
struct DmFusedArgs {
  int wgs = 1, rank = 0;
  int share = 1;                       // as DmArgs::share (wgs is cut to the residency cap)
  uint64_t slot = 0;
  uint8_t *own = nullptr;
  uint32_t *poison_host = nullptr;
  uint64_t timeout_ticks = 0;
  int na = 0, nt = 0, d0 = 0, nd = 0;  // phase A pushes m[0, na); trees t[0, nt); phase D pulls m[d0, d0 + nd)
  DmMsg m[kMaxFusedMsgs];
  int nl = 0, pos = 0;
  unsigned swap = 0;
  DmFusedTree t[kMaxFusedTrees];
  uint64_t *stamps = nullptr;          // DmArgs::stamps: one record per workgroup (kind 4: entry, end of the
  uint32_t serial = 0;                 // first wait, end)
  int slices = 1;                      // per-slice flags (dm::kSliceReadyOff; BINE_DIRECT_SLICE_FLAGS=0: off)
};
// BINE_ERR_UNSUPPORTED: (dtype, op) has no fused instantiation (the caller
// issues the primitives one by one)
int launch_dm_fused(const DmFusedArgs &a, int dtype, int op, void *stream);
int dm_fused_check(const DmFusedArgs &a, int dtype, int op);  // launch_dm_fused's argument check alone
bool dm_fused_supported(int dtype, int op);
int launch_checksum(const void *buf, size_t count, int dtype, uint64_t *out, void *stream);

}  // namespace bine
