// segments.cpp -- the tile table of the segmented copy (bine_copy_segments).
//
// Host only, no HIP: plain C++ over addresses and sizes, so the CPU suite can
// check the cover (bine_plan_segments) and a stand-alone program can run it
// under the host sanitizers (tools/segments_check.cpp).  launch_copy_segments
// (kernels.hip) issues exactly the launches plan_seg_launches returns, and
// k_copy_segs derives a segment's head and vector count from the same two
// expressions (seg_head / seg_nvec) over the same descriptor.
#include <algorithm>

#include "bine_internal.h"

namespace bine {

static uint64_t seg_head(uint64_t dst, uint64_t bytes) {
  const uint64_t h = (16 - (dst & 15)) & 15;
  return h < bytes ? h : bytes;
}
static uint64_t seg_nvec(uint64_t bytes, uint64_t head) { return (bytes - head) / 16; }

int plan_seg_launches(int n, const uint64_t *dst_addr, const uint64_t *src_addr, const size_t *bytes,
                      std::vector<SegLaunch> &out) {
  out.clear();
  if (n < 0 || n > BINE_MULTI_MAX) return BINE_ERR_ARG;
  if (n > 0 && (!dst_addr || !src_addr || !bytes)) return BINE_ERR_ARG;
  for (int k = 0; k < n; k++) {
    if (bytes[k] == 0) continue;
    if (!dst_addr[k] || !src_addr[k]) return BINE_ERR_ARG;
    if (out.empty() || out.back().nseg == kSegsPerLaunch) {
      out.emplace_back();
      out.back().tile0[0] = 0;
    }
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

}  // namespace bine

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
