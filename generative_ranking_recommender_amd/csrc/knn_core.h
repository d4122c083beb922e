// knn_core.h — what rqsid_row_knn (row_knn.hip) and rqsid_probe_knn (probe_knn.hip) share.
// Not ABI.
//
// Both entries screen in fp32 on tile_rows.h's block, keep the k + 8 smallest screen values of a LIST (row_knn: one
// per (query, chunk of the order); probe_knn: one per (query, probe) item), fold a query's lists into U, certify
// each list and rank in fp64 what can still place.  Here once: the record and the parameters, the interval e, the
// screen's policy (KnnPolicy), the fold of one query (knn_fold_query) and the exact pass of one query
// (knn_exact_query).  What the entries differ in reaches the last two as a small accessor:
//   n()             the number of lists of the query
//   meta_at(c)      the index of list c's record in KnnParams::meta
//   entry_at(c, j)  the index of entry j of list c in KnnParams::ls / lr
//   range(c, a, b)  the positions [a, b) of the order that list c stands for (the all-rows pass)
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "assign_common.h"
#include "exact_row.h"
#include "tile_rows.h"

namespace rqsid {

// (the header's words [4, 16) are the three counters of the fold)
constexpr int kKnnSlack = 8;       // list entries beyond k
constexpr int kKnnMV = kMaxDim / 4 / 64;  // float4 pieces of a row per lane of the exact pass
constexpr int kKnnFull = 1, kKnnBad = 2, kKnnAllRows = 4;  // KnnMeta::flags

// what a block knows about one list after its sweep, beside the list itself
struct KnnMeta {
  float max_s;    // the largest kept s (meaningful when full)
  float xn_max;   // the largest |x|^2 among the rows the block met (L2: the worst-case e of the list)
  int32_t count;  // list entries
  int32_t flags;  // kKnnFull, kKnnBad (a non-finite s), kKnnAllRows (set by the fold: not certified)
};
static_assert(sizeof(KnnMeta) == 16, "record layout");

// xn, qn: L2 fl32(|x|^2) (kNormSqFinite), cosine fl32(1 / |x|) (kNormInv); -1: never a neighbour / a query without
// an answer
struct KnnParams : RowPairParams {
  double* U;      // [queries]
  KnnMeta* meta;  // one per list
  float* ls;      // [..][C][nqp]: entry j of a list is nqp floats after entry j - 1
  int32_t* lr;    // likewise: row numbers
  int32_t* out_row;
  float* out_val;
  int64_t nqp;    // the stride between a list's entries
  int32_t k, C;
};

// e >= |s - t|, in fp64 from the stored fp32 norms: L2 (|q|^2 + |x|^2) R + dim 2^-120, cosine
// R + 2^-50, R = 1.01 (dim + 8) 2^-24
template <int METRIC>
__device__ __forceinline__ double knn_err(int dim, float qn, float xn) {
  const double R = 1.01 * (double)(dim + 8) * 0x1p-24;
  if constexpr (METRIC == RQSID_KNN_L2) return ((double)qn + (double)xn) * R + (double)dim * 0x1p-120;
  return R + 0x1p-50;
}

// row_tile_sweep's policy: screen values, and per column of the block the C smallest of what it sweeps
template <int METRIC>
struct KnnPolicy {
  const KnnParams& p;
  // MFMA role: lane (r, h) of wave wv holds column 32 wv + r: its query's norm term, self row and range
  float qn;
  int self;
  int64_t qlo, qhi;
  // walking role (threads 0..127): column t and its list in the workspace
  float* ls;
  int32_t* lr;
  int cnt, bad;
  float thr;  // what a value has to stay below to enter: +inf until the list is full, then its largest
  float mx;
  float xmax;  // L2: the largest |x|^2 this thread met

  __device__ __forceinline__ void tile_row(int, int& row, float& xn) {
    if (xn < 0.f) row = -1;  // a row without a key is never a neighbour
    if (METRIC == RQSID_KNN_L2 && row >= 0) xmax = fmaxf(xmax, xn);
  }

  __device__ __forceinline__ float value(int64_t pos0, int j, float dot, float xn, int rw) const {
    // the column's range in positions of this tile
    const int jlo = qlo - pos0 > 0 ? (qlo - pos0 < kRowTile ? (int)(qlo - pos0) : kRowTile) : 0;
    const int jhi = qhi - pos0 > 0 ? (qhi - pos0 < kRowTile ? (int)(qhi - pos0) : kRowTile) : 0;
    float s;
    if constexpr (METRIC == RQSID_KNN_L2) s = fmaf(-2.0f, dot, qn + xn);
    else s = -((dot * qn) * xn);
    // a value the interval does not cover becomes -inf: it reaches the walk, which flags the list
    s = fabsf(s) <= FLT_MAX ? s : -INFINITY;
    const bool skip = (rw < 0) | (rw == self) | (j < jlo) | (j >= jhi);
    return skip ? INFINITY : s;
  }

  __device__ __forceinline__ void walk(int64_t, const float* s_d, const int* s_row) {
    const int t = threadIdx.x;
    for (int j = 0; j < kRowTile; j += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = s_d[(j + u) * kRowDStride + t];
      bool any = false;
#pragma unroll
      for (int u = 0; u < 8; ++u) any |= v[u] < thr;
      if (any) {
#pragma unroll 1
        for (int u = 0; u < 8; ++u) {
          const float w = s_d[(j + u) * kRowDStride + t];
          if (!(w < thr)) continue;
          if (w == -INFINITY) {
            bad = 1;
            continue;
          }
          const int row = s_row[j + u];
          if (cnt < p.C) {
            ls[cnt * p.nqp] = w;
            lr[cnt * p.nqp] = row;
            mx = fmaxf(mx, w);
            if (++cnt == p.C) thr = mx;
          } else {  // replace the largest; the new largest is the second largest or the newcomer
            int im = 0;
            float m1 = -INFINITY, m2 = -INFINITY;
            for (int i = 0; i < p.C; ++i) {
              const float a = ls[i * p.nqp];
              if (a > m1) {
                m2 = m1;
                m1 = a;
                im = i;
              } else if (a > m2) {
                m2 = a;
              }
            }
            ls[im * p.nqp] = w;
            lr[im * p.nqp] = row;
            thr = fmaxf(m2, w);
          }
        }
      }
    }
  }
};

// One query's lists -> U and the lists' certificates (one thread).  U = the k-th smallest s + e over every kept
// entry of every list: the lists hold pairwise different rows, so k of them have a key <= U.  A list is certified
// when it is not full (it holds every eligible row), or when its largest kept s - its worst e > U (a row it let go
// has a key > U).  Counters: header word 1 = queries ranked from their lists alone, 2 = lists sent to the all-rows
// pass, 3 = queries without an answer.
template <int METRIC, class Lists>
__device__ __forceinline__ void knn_fold_query(const KnnParams& p, int i, const Lists& L) {
  const float qn = p.qn[i];
  if (qn < 0.f) {  // no answer: the exact pass writes -1 / NaN
    atomicAdd(reinterpret_cast<int*>(p.err) + 3, 1);
    return;
  }
  // the k smallest s + e, unsorted slots k .. 15 held at -inf so that they never take part
  double top[RQSID_KNN_MAX];
#pragma unroll
  for (int j = 0; j < RQSID_KNN_MAX; ++j) top[j] = j < p.k ? INFINITY : -INFINITY;
  const int nl = L.n();
  for (int c = 0; c < nl; ++c) {
    const int cnt = p.meta[L.meta_at(c)].count;
    for (int j = 0; j < cnt; ++j) {
      const int64_t at = L.entry_at(c, j);
      const float s = p.ls[at];
      double v = (double)s + knn_err<METRIC>(p.dim, qn, METRIC == RQSID_KNN_L2 ? p.xn[p.lr[at]] : 0.f);
#pragma unroll
      for (int jj = 0; jj < RQSID_KNN_MAX; ++jj) {
        const double o = top[jj];
        const bool lt = v < o;
        top[jj] = lt ? v : o;
        v = lt ? o : v;
      }
    }
  }
  double U = -INFINITY;
#pragma unroll
  for (int j = 0; j < RQSID_KNN_MAX; ++j) U = top[j] > U ? top[j] : U;
  p.U[i] = U;
  int all_rows = 0;
  for (int c = 0; c < nl; ++c) {
    KnnMeta* const m = p.meta + L.meta_at(c);
    const int fl = m->flags;
    const bool beyond = (double)m->max_s - knn_err<METRIC>(p.dim, qn, m->xn_max) > U;
    if ((fl & kKnnBad) || ((fl & kKnnFull) && !beyond)) {
      m->flags = fl | kKnnAllRows;
      ++all_rows;
    }
  }
  if (all_rows) atomicAdd(reinterpret_cast<int*>(p.err) + 2, all_rows);
  else atomicAdd(reinterpret_cast<int*>(p.err) + 1, 1);
}

// One query, one wave (lanes over dims): fp64 keys, eight rows at a time with the re-score's halving reduction, of
// the listed rows with s - e <= U and of every row of an uncertified list's range; ranked by (key, row number) in
// lanes 0 .. k-1 and written to out_row / out_val.
template <int XF, int METRIC, class Lists>
__device__ __forceinline__ void knn_exact_query(const KnnParams& p, int i, int lane, const Lists& L) {
  const float qn = p.qn[i];
  if (qn < 0.f) {
    if (lane < p.k) {
      p.out_row[(int64_t)i * p.k + lane] = -1;
      p.out_val[(int64_t)i * p.k + lane] = __uint_as_float(0x7FC00000u);
    }
    return;
  }
  const int nv = p.dim / 4;
  const float* const xf = static_cast<const float*>(p.x);
  float4 v[kKnnMV];
  double qq = 0.0;
#pragma unroll
  for (int m = 0; m < kKnnMV; ++m) {
    const int e = lane + 64 * m;
    v[m] = e < nv ? load_row4<XF>(static_cast<const float*>(p.q), i, p.dim, e) : make_float4(0.f, 0.f, 0.f, 0.f);
    qq += sq4(v[m]);
  }
  const double sqq = sqrt(wave_sum(qq));
  const double U = p.U[i];
  const int self = clean_self(p, i);

  double hk = INFINITY;  // lane j < k: the j-th place so far
  int hr = INT_MAX;
  // the fp64 keys of up to eight rows (rr < 0: none), each offered to the ranking
  const auto batch = [&](const int (&rr)[kBatch]) __attribute__((always_inline)) {
    double a0[kBatch], a1[kBatch];
#pragma unroll
    for (int jj = 0; jj < kBatch; ++jj) {
      a0[jj] = a1[jj] = 0.0;
#pragma unroll
      for (int m = 0; m < kKnnMV; ++m) {
        const int e = lane + 64 * m;
        if (rr[jj] < 0 || e >= nv) continue;
        const float4 c = load_row4<XF>(xf, rr[jj], p.dim, e);
        if constexpr (METRIC == RQSID_KNN_L2) {
          const double d0 = (double)v[m].x - c.x, d1 = (double)v[m].y - c.y, d2 = (double)v[m].z - c.z,
                       d3 = (double)v[m].w - c.w;
          a0[jj] = fma(d3, d3, fma(d2, d2, fma(d1, d1, fma(d0, d0, a0[jj]))));
        } else {
          a0[jj] = fma((double)v[m].w, (double)c.w, fma((double)v[m].z, (double)c.z,
                   fma((double)v[m].y, (double)c.y, fma((double)v[m].x, (double)c.x, a0[jj]))));
          a1[jj] = fma((double)c.w, (double)c.w, fma((double)c.z, (double)c.z,
                   fma((double)c.y, (double)c.y, fma((double)c.x, (double)c.x, a1[jj]))));
        }
      }
    }
    double key = batch_reduce<64>(a0, lane);
    if constexpr (METRIC == RQSID_KNN_COSINE) key = -(key / (sqq * sqrt(batch_reduce<64>(a1, lane))));
#pragma unroll
    for (int jj = 0; jj < kBatch; ++jj) {
      if (rr[jj] < 0) continue;
      const double ck = __shfl(key, batch_lane<64>(jj));
      const int cr = rr[jj];
      if (!(fabs(ck) <= DBL_MAX)) continue;  // a row with a non-finite key is never a neighbour
      const bool before = lane < p.k && (hk < ck || (hk == ck && hr < cr));
      const int at = __popcll(__ballot(before));  // (the places are sorted: the better ones are lanes 0 .. at-1)
      if (at >= p.k) continue;
      const double uk = __shfl_up(hk, 1);
      const int ur = __shfl_up(hr, 1);
      if (lane == at) {
        hk = ck;
        hr = cr;
      } else if (lane > at && lane < p.k) {
        hk = uk;
        hr = ur;
      }
    }
  };
  // the rows of the lanes named in mask (wave-uniform), eight at a time
  const auto offer = [&](uint64_t mask, int row) __attribute__((always_inline)) {
    while (mask) {
      int rr[kBatch];
#pragma unroll
      for (int jj = 0; jj < kBatch; ++jj) {
        rr[jj] = -1;
        if (mask) {
          rr[jj] = __shfl(row, __builtin_ctzll(mask));
          mask &= mask - 1;
        }
      }
      batch(rr);
    }
  };

  const int nl = L.n();
  for (int c = 0; c < nl; ++c) {
    const KnnMeta m = p.meta[L.meta_at(c)];
    if (!(m.flags & kKnnAllRows)) {
      for (int j0 = 0; j0 < m.count; j0 += 64) {
        const int j = j0 + lane;
        bool ok = j < m.count;
        int row = -1;
        if (ok) {
          const int64_t at = L.entry_at(c, j);
          row = p.lr[at];
          ok = (double)p.ls[at] - knn_err<METRIC>(p.dim, qn, METRIC == RQSID_KNN_L2 ? p.xn[row] : 0.f) <= U;
        }
        offer(__ballot(ok), row);
      }
    } else {
      int64_t a, b;
      L.range(c, a, b);
      for (int64_t pos = a; pos < b; pos += 64) {
        const int64_t pp = pos + lane;
        int row = -1;
        if (pp < b) row = p.row_index ? p.row_index[pp] : (int)pp;
        const bool ok = pp < b && (int64_t)(uint32_t)row < p.n_rows && row != self;
        offer(__ballot(ok), row);
      }
    }
  }
  if (lane < p.k) {
    const bool none = hr == INT_MAX;
    p.out_row[(int64_t)i * p.k + lane] = none ? -1 : hr;
    p.out_val[(int64_t)i * p.k + lane] =
        none ? INFINITY : (METRIC == RQSID_KNN_L2 ? (float)sqrt(hk) : (float)(-hk));
  }
}

inline int knn_check_k(const char* who, int32_t k) {
  if (k < 1 || k > RQSID_KNN_MAX) return fail(RQSID_E_ARG, "%s: k = %d (1 .. %d)", who, k, RQSID_KNN_MAX);
  return RQSID_OK;
}
inline int knn_check_metric(const char* who, int32_t metric) {
  if (metric != RQSID_KNN_L2 && metric != RQSID_KNN_COSINE)
    return fail(RQSID_E_ARG, "%s: unknown metric %d", who, metric);
  return RQSID_OK;
}

}  // namespace rqsid
