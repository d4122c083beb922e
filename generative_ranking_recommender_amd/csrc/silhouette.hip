// silhouette.hip — exact silhouette sums of scored rows against every cluster (rqsid_silhouette).
//
// For every query i and every cluster c the sum S(i, c) of the TRUE pairwise distances from i to the members of c,
// from which a (own cluster), b (nearest other cluster by mean distance) and s = (b - a) / max(a, b) follow.  No
// centroid identity exists for unsquared distances, so this is m x n x dim matrix work plus a segmented reduction.
//
// Shape.  The base rows are walked in the bucketed order (row_index) in fixed tiles of 128 positions that straddle
// segments; a block owns 128 queries and one chunk of consecutive tiles, and is tile_rows.h's block
// (row_tile_sweep: the staging, the MFMAs, the park and the barriers).  This file supplies its policy: the value
// parked for a pair is d = sqrt(max(0, |q|^2 + |x|^2 - 2 D)), zero for the self row and for rows that do not
// exist; the walk goes through the tile's positions with the segment boundaries as wave-uniform control flow: an
// fp32 sum per (tile, segment) piece, added in fp64 to the running segment sum; a segment that ends becomes the
// own-cluster sum or competes for b.  Per (query, chunk) the block writes one record; a second kernel folds a
// query's records in chunk order.  No float atomics: the result is a pure function of the arguments (the per-piece
// fp32 sums do not even depend on chunk_rows).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "assign_common.h"
#include "tile_rows.h"

namespace rqsid {
namespace {

// what a block knows about one query after its chunk
struct SilRecord {
  double first_sum;   // the piece of first_seg, a segment that began before the chunk
  double last_sum;    // the piece of last_seg, a segment that began in the chunk and runs past its end
  double own_sum;     // the own cluster's sum when it lies wholly inside the chunk, else 0
  double best;        // min mean over the other segments wholly inside the chunk
  int32_t first_seg, last_seg, best_seg;  // -1: none
  int32_t bad;        // a non-finite piece sum
};
static_assert(sizeof(SilRecord) == 48, "record layout");

struct SilParams : RowPairParams {  // xn, qn: |row|^2 (kNormSq)
  SilRecord* rec;  // [n_chunks][qtiles * kRowQ]
  float* out_a;
  float* out_b;
  int32_t* out_b_seg;
  float* out_s;
};

// row_tile_sweep's policy: distances, and per query the chunk's running segment sums
struct SilPolicy {
  const SilParams& p;
  const int64_t c0, c1;
  // MFMA role: lane (r, h) of wave wv holds query q0 + 32 wv + r
  float qn;
  int self;
  // walking role (threads 0..127): query q0 + t and the chunk's running state
  int my_seg;
  int seg;         // the first segment that ends after the walk's position (block-uniform)
  double cur;      // the open segment's sum inside this chunk
  bool open;
  SilRecord rec;

  __device__ __forceinline__ void tile_row(int, int&, float&) {}

  __device__ __forceinline__ float value(int64_t, int, float dot, float xn, int rw) const {
    float tt = fmaf(-2.0f, dot, qn + xn);
    // the self row is excluded by INDEX and a position without a row adds nothing: their argument is zeroed
    // (sqrt(0) = 0) rather than their root branched around; a NaN stays a NaN
    const bool skip = (rw < 0) | (rw == self);
    tt = (skip | (tt < 0.f)) ? 0.f : tt;
    return sqrtf(tt);
  }

  // one thread per query, the tile's positions in order, segment boundaries as uniform branches
  __device__ __forceinline__ void walk(int64_t pos0, const float* s_d, const int*) {
    const int t = threadIdx.x;
    int64_t pos = pos0;
    const int64_t tend = pos0 + kRowTile < c1 ? pos0 + kRowTile : c1;
    while (pos < tend && seg < p.n_seg) {
      const int64_t shi = off_at(p, seg + 1), slo = off_at(p, seg);  // (both scalar loads in flight together)
      if (shi <= pos) {  // an empty segment
        ++seg;
        continue;
      }
      if (slo > pos) {  // (only a broken table leaves positions between two segments)
        pos = slo < tend ? slo : tend;
        continue;
      }
      const int64_t end = shi < tend ? shi : tend;
      // the piece's distances in position order; eight LDS reads in flight at a time, the adds still one by one
      float ps = 0.f;
      int j = (int)(pos - pos0);
      const int je = (int)(end - pos0);
      for (; j + 8 <= je; j += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s_d[(j + u) * kRowDStride + t];
#pragma unroll
        for (int u = 0; u < 8; ++u) ps += v[u];
      }
      for (; j < je; ++j) ps += s_d[j * kRowDStride + t];
      cur += (double)ps;
      if (!(fabsf(ps) <= FLT_MAX)) rec.bad = 1;
      open = true;
      pos = end;
      if (end == shi) {  // the segment ends here
        if (slo < c0) {
          rec.first_seg = seg;
          rec.first_sum = cur;
        } else if (seg == my_seg) {
          rec.own_sum = cur;
        } else {
          const double mean = cur / (double)(shi - slo);
          if (mean < rec.best) {
            rec.best = mean;
            rec.best_seg = seg;
          }
        }
        cur = 0.0;
        open = false;
        ++seg;
      }
    }
  }
};

template <int XF>
__global__ __launch_bounds__(256, 2) void silhouette_kernel(SilParams p) {
  const RowTileLds lds = row_tile_lds();
  const int t = threadIdx.x;
  const int qtile = (int)(blockIdx.x % (unsigned)p.qtiles), chunk = (int)(blockIdx.x / (unsigned)p.qtiles);
  const int q0 = qtile * kRowQ;
  const int64_t c0 = (int64_t)chunk * p.chunk_rows;
  const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;
  const int ntile = (int)((c1 - c0 + kRowTile - 1) / kRowTile);

  const int myq = q0 + (t >> 6) * 32 + (t & 31), wq = q0 + t;
  SilPolicy w{p, c0, c1};
  w.qn = myq < p.nq ? p.qn[myq] : 0.f;
  w.self = myq < p.nq ? clean_self(p, myq) : -1;
  w.my_seg = (t < kRowQ && wq < p.nq) ? clean_seg(p, wq) : -1;
  {
    int lo = 0, hi = p.n_seg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (off_at(p, mid + 1) > c0) hi = mid;
      else lo = mid + 1;
    }
    w.seg = lo;
  }
  w.cur = 0.0;
  w.open = false;
  w.rec.first_sum = w.rec.last_sum = w.rec.own_sum = 0.0;
  w.rec.best = INFINITY;
  w.rec.first_seg = w.rec.last_seg = w.rec.best_seg = -1;
  w.rec.bad = 0;

  row_tile_sweep<XF>(p, q0, c0, c1, 0, ntile, lds, w);

  if (t < kRowQ) {
    if (w.open) {  // a segment that runs past the chunk's end
      if (off_at(p, w.seg) < c0) {
        w.rec.first_seg = w.seg;
        w.rec.first_sum = w.cur;
      } else {
        w.rec.last_seg = w.seg;
        w.rec.last_sum = w.cur;
      }
    }
    p.rec[(int64_t)chunk * p.qtiles * kRowQ + wq] = w.rec;
  }
}

// a query's records in chunk order -> a, b, b_seg, s
__global__ __launch_bounds__(256) void sil_fold_kernel(SilParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nq) return;
  const int my_seg = clean_seg(p, i);
  const int self = clean_self(p, i);
  const int64_t nqp = (int64_t)p.qtiles * kRowQ;
  double a_sum = 0.0, best = INFINITY, carry_sum = 0.0;
  int best_seg = -1, carry_seg = -1, bad = 0;
  auto close = [&](int s, double sum) {  // a segment whose pieces are all in
    if (s == my_seg) {
      a_sum += sum;
    } else {
      const double mean = sum / (double)(off_at(p, s + 1) - off_at(p, s));
      if (mean < best) {
        best = mean;
        best_seg = s;
      }
    }
  };
  for (int k = 0; k < p.n_chunks; ++k) {
    const SilRecord rc = p.rec[k * nqp + i];
    const int64_t c1 = ((int64_t)k + 1) * p.chunk_rows;
    bad |= rc.bad;
    if (rc.first_seg >= 0) {
      if (carry_seg == rc.first_seg) {
        carry_sum += rc.first_sum;
      } else {
        carry_seg = rc.first_seg;
        carry_sum = rc.first_sum;
      }
      if (off_at(p, carry_seg + 1) <= c1) {
        close(carry_seg, carry_sum);
        carry_seg = -1;
      }
    }
    a_sum += rc.own_sum;
    if (rc.best_seg >= 0 && rc.best < best) {
      best = rc.best;
      best_seg = rc.best_seg;
    }
    if (rc.last_seg >= 0) {
      carry_seg = rc.last_seg;
      carry_sum = rc.last_sum;
    }
  }
  const int64_t n_o = my_seg >= 0 ? off_at(p, my_seg + 1) - off_at(p, my_seg) : 0;
  const int64_t den = self >= 0 ? n_o - 1 : n_o;
  double a = den > 0 ? a_sum / (double)den : 0.0;
  double b = best, s;
  if (self >= 0 && my_seg >= 0 && n_o <= 1) {
    s = 0.0;
  } else {
    const double m = a > b ? a : b;
    s = m == 0.0 ? 0.0 : (b - a) / m;  // b = +inf (no other cluster): NaN
  }
  if (bad) {
    a = b = s = __longlong_as_double(0x7FF8000000000000LL);
    best_seg = -1;
  }
  p.out_a[i] = (float)a;
  p.out_b[i] = (float)b;
  p.out_b_seg[i] = best_seg;
  p.out_s[i] = (float)s;
}

template <int XF>
int sil_launch(const SilParams& p, hipStream_t st) {
  int rc;
  if ((rc = row_pair_prepare<XF, kNormSq, 0>("rqsid_silhouette", p, st))) return rc;
  hipLaunchKernelGGL((silhouette_kernel<XF>), dim3((unsigned)((int64_t)p.qtiles * p.n_chunks)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_silhouette"))) return rc;
  hipLaunchKernelGGL(sil_fold_kernel, dim3((unsigned)cdiv(p.nq, 256)), dim3(256), 0, st, p);
  return check_launch("rqsid_silhouette (fold)");
}

// the workspace after the shared areas: the records
int64_t sil_bytes(const RowPairPlan& pl) {
  return pl.off_own + pl.n_chunks * pl.qtiles * kRowQ * (int64_t)sizeof(SilRecord);
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int32_t rqsid_silhouette_tile_rows(void) { return kRowTile; }

int64_t rqsid_silhouette_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t chunk_rows) {
  const char* const who = "rqsid_silhouette_workspace_bytes";
  int rc;
  if ((rc = row_pair_check_counts(who, n_rows, n_queries)) || (rc = row_pair_check_chunks(who, chunk_rows))) return rc;
  RowPairPlan pl;
  if (!row_pair_plan(n_rows, n_queries, chunk_rows, pl)) return row_pair_fail_blocks(who, pl);
  return sil_bytes(pl);
}

int rqsid_silhouette(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                     int32_t n_segments, const int32_t* seg_row_off, const void* q, int32_t n_queries,
                     const int32_t* query_self, const int32_t* query_seg, int32_t chunk_rows, float* out_a,
                     float* out_b, int32_t* out_b_seg, float* out_s, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  const char* const who = "rqsid_silhouette";
  int rc;
  if ((rc = row_pair_check_format(who, x_format, dim)) || (rc = row_pair_check_counts(who, n_rows, n_queries)) ||
      (rc = row_pair_check_chunks(who, chunk_rows, n_segments)))
    return rc;
  if (n_rows == 0 || n_queries == 0) return RQSID_OK;
  if (n_segments < 1 || !seg_row_off)
    return fail(RQSID_E_ARG, "%s: n_segments = %d and seg_row_off are required", who, n_segments);
  if ((rc = row_pair_check_rows(who, x, q))) return rc;
  if (!out_a || !out_b || !out_b_seg || !out_s)
    return fail(RQSID_E_ARG, "%s: out_a, out_b, out_b_seg and out_s are required", who);
  RowPairPlan pl;
  if (!row_pair_plan(n_rows, n_queries, chunk_rows, pl)) return row_pair_fail_blocks(who, pl);
  if (!workspace || workspace_bytes < sil_bytes(pl))
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes,
                (long long)sil_bytes(pl));
  SilParams p;
  row_pair_fill(p, x, n_rows, dim, row_index, n_segments, seg_row_off, q, n_queries, query_self, query_seg, workspace,
                pl);
  p.rec = reinterpret_cast<SilRecord*>(static_cast<char*>(workspace) + pl.off_own);
  p.out_a = out_a;
  p.out_b = out_b;
  p.out_b_seg = out_b_seg;
  p.out_s = out_s;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_xf(x_format, [&](auto xf) { return sil_launch<decltype(xf)::value>(p, st); });
}

}  // extern "C"
