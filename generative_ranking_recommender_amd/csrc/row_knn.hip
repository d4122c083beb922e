// row_knn.hip — the exact k nearest rows of every query, over all rows or inside one segment (rqsid_row_knn;
// DESIGN.md §3.3c).
//
// Three kernels after the norms and the table check:
//  1. knn_screen_kernel: tile_rows.h's block (row_tile_sweep: 128 queries x one chunk of 128-position tiles of the
//     bucketed order), over the tiles that the union of the block's query ranges touches.  Its policy parks the
//     metric's fp32 screen value s (L2: |q|^2 + |x|^2 - 2 D, cosine: -D / (|q| |x|)), +inf for a position that is
//     missing, outside the query's range, the self row or a row that can never be a neighbour; one thread per query
//     walks the tile's positions and keeps the C = k + 8 smallest (s, row) of the chunk.  The kept list lives in the
//     workspace record of the (query, chunk) pair: the walk holds only its length and its largest value in
//     registers, so a position costs one LDS read and one compare, and the list is touched (through L2) only by
//     the O(C log(chunk / C)) positions that enter it.  LDS stays at the silhouette's 74.7 KB: two blocks per CU.
//  2. knn_fold_kernel: one thread per query; U = the k-th smallest s + e over the chunks' lists (e >= |s - t|, the
//     derived interval), and per chunk the certificate "not full, or largest kept s - worst e of the chunk > U".
//  3. knn_exact_kernel: one wave per query, lanes over dims; fp64 keys, eight rows at a time with the re-score's
//     halving reduction, of the listed rows with s - e <= U and of every row of an uncertified chunk; ranked by
//     (key, row number) in lanes 0 .. k-1.
// The result is a function of the row set alone: e, the slack and chunk_rows move only the amount of fp64 work.
// No float atomics, no write positioned by a device counter.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "assign_common.h"
#include "exact_row.h"
#include "tile_rows.h"

namespace rqsid {
namespace {

// (the header's words [4, 16) are this entry's three counters)
constexpr int kKnnSlack = 8;       // list entries beyond k
constexpr int kKnnMV = kMaxDim / 4 / 64;  // float4 pieces of a row per lane of the exact pass
constexpr int kKnnFull = 1, kKnnBad = 2, kKnnAllRows = 4;  // KnnMeta::flags

// what a block knows about one query after its chunk, beside the list itself
struct KnnMeta {
  float max_s;    // the largest kept s (meaningful when full)
  float xn_max;   // the largest |x|^2 among the chunk's rows the block met (L2: the worst-case e of the chunk)
  int32_t count;  // list entries
  int32_t flags;  // kKnnFull, kKnnBad (a non-finite s), kKnnAllRows (set by the fold: not certified)
};
static_assert(sizeof(KnnMeta) == 16, "record layout");

// xn, qn: L2 fl32(|x|^2) (kNormSqFinite), cosine fl32(1 / |x|) (kNormInv); -1: never a neighbour / a query without
// an answer
struct KnnParams : RowPairParams {
  double* U;      // [qtiles * kRowQ]
  KnnMeta* meta;  // [n_chunks][qtiles * kRowQ]
  float* ls;      // [n_chunks][C][qtiles * kRowQ]
  int32_t* lr;    // likewise: row numbers
  int32_t* out_row;
  float* out_val;
  int64_t nqp;    // qtiles * kRowQ
  int32_t k, C;
};

// the positions query i searches
__device__ __forceinline__ void query_range(const KnnParams& p, int i, int64_t& lo, int64_t& hi) {
  const int s = clean_seg(p, i);
  lo = s >= 0 ? off_at(p, s) : 0;
  hi = s >= 0 ? off_at(p, s + 1) : p.n_rows;
}

// e >= |s - t|, in fp64 from the stored fp32 norms: L2 (|q|^2 + |x|^2) R + dim 2^-120, cosine
// R + 2^-50, R = 1.01 (dim + 8) 2^-24
template <int METRIC>
__device__ __forceinline__ double knn_err(int dim, float qn, float xn) {
  const double R = 1.01 * (double)(dim + 8) * 0x1p-24;
  if constexpr (METRIC == RQSID_KNN_L2) return ((double)qn + (double)xn) * R + (double)dim * 0x1p-120;
  return R + 0x1p-50;
}

// row_tile_sweep's policy: screen values, and per query the C smallest of the chunk
template <int METRIC>
struct KnnPolicy {
  const KnnParams& p;
  // MFMA role: lane (r, h) of wave wv holds query q0 + 32 wv + r, its norm term, self row and range
  float qn;
  int self;
  int64_t qlo, qhi;
  // walking role (threads 0..127): query q0 + t and its list in the workspace
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
    // the query's range in positions of this tile
    const int jlo = qlo - pos0 > 0 ? (qlo - pos0 < kRowTile ? (int)(qlo - pos0) : kRowTile) : 0;
    const int jhi = qhi - pos0 > 0 ? (qhi - pos0 < kRowTile ? (int)(qhi - pos0) : kRowTile) : 0;
    float s;
    if constexpr (METRIC == RQSID_KNN_L2) s = fmaf(-2.0f, dot, qn + xn);
    else s = -((dot * qn) * xn);
    // a value the interval does not cover becomes -inf: it reaches the walk, which flags the chunk
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

template <int XF, int METRIC>
__global__ __launch_bounds__(256, 2) void knn_screen_kernel(KnnParams p) {
  const RowTileLds lds = row_tile_lds();
  __shared__ int s_lo, s_hi, s_xmax;

  const int t = threadIdx.x;
  const int qtile = (int)(blockIdx.x % (unsigned)p.qtiles), chunk = (int)(blockIdx.x / (unsigned)p.qtiles);
  const int q0 = qtile * kRowQ;
  const int64_t c0 = (int64_t)chunk * p.chunk_rows;
  const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;

  const int myq = q0 + (t >> 6) * 32 + (t & 31);
  const int64_t wq = q0 + t;
  KnnPolicy<METRIC> w{p};
  w.qn = myq < p.nq ? p.qn[myq] : -1.0f;
  w.self = myq < p.nq ? clean_self(p, myq) : -1;
  w.qlo = w.qhi = 0;  // (a query without an answer searches nothing)
  if (myq < p.nq && !(w.qn < 0.f)) query_range(p, myq, w.qlo, w.qhi);
  w.ls = p.ls + (int64_t)chunk * p.C * p.nqp + wq;
  w.lr = p.lr + (int64_t)chunk * p.C * p.nqp + wq;
  w.cnt = w.bad = 0;
  w.thr = INFINITY;
  w.mx = -INFINITY;
  w.xmax = 0.f;

  // the union of the block's ranges: tiles outside it are skipped
  if (t == 0) {
    s_lo = INT_MAX;
    s_hi = 0;
    s_xmax = 0;
  }
  __syncthreads();
  if ((t & 32) == 0 && w.qlo < w.qhi) {
    atomicMin(&s_lo, (int)w.qlo);
    atomicMax(&s_hi, (int)w.qhi);
  }
  __syncthreads();
  const int64_t ulo = s_lo, uhi = s_hi;
  const int ntile = (int)((c1 - c0 + kRowTile - 1) / kRowTile);
  const int tile0 = ulo > c0 ? (int)((ulo - c0) / kRowTile < ntile ? (ulo - c0) / kRowTile : ntile) : 0;
  int tile1 = uhi > c0 ? (int)((uhi - c0 + kRowTile - 1) / kRowTile) : 0;
  tile1 = tile1 < ntile ? tile1 : ntile;

  row_tile_sweep<XF>(p, q0, c0, c1, tile0, tile1, lds, w);

  if (METRIC == RQSID_KNN_L2 && t < kRowTile) atomicMax(&s_xmax, __float_as_int(w.xmax));  // (xmax >= 0: int order)
  __syncthreads();
  if (t < kRowQ) {
    KnnMeta m;
    m.max_s = w.thr;
    m.xn_max = __int_as_float(s_xmax);
    m.count = w.cnt;
    m.flags = (w.cnt == p.C ? kKnnFull : 0) | (w.bad ? kKnnBad : 0);
    p.meta[(int64_t)chunk * p.nqp + wq] = m;
  }
}

// a query's lists -> U and the chunks' certificates
template <int METRIC>
__global__ __launch_bounds__(256) void knn_fold_kernel(KnnParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nq) return;
  const float qn = p.qn[i];
  if (qn < 0.f) {  // no answer: the exact pass writes -1 / NaN
    atomicAdd(reinterpret_cast<int*>(p.err) + 3, 1);
    return;
  }
  // the k smallest s + e, unsorted slots k .. 15 held at -inf so that they never take part
  double top[RQSID_KNN_MAX];
#pragma unroll
  for (int j = 0; j < RQSID_KNN_MAX; ++j) top[j] = j < p.k ? INFINITY : -INFINITY;
  for (int c = 0; c < p.n_chunks; ++c) {
    const int cnt = p.meta[(int64_t)c * p.nqp + i].count;
    for (int j = 0; j < cnt; ++j) {
      const int64_t at = ((int64_t)c * p.C + j) * p.nqp + i;
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
  for (int c = 0; c < p.n_chunks; ++c) {
    KnnMeta* const m = p.meta + (int64_t)c * p.nqp + i;
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

// one wave per query: fp64 keys of the rows that can still place, ranked by (key, row) in lanes 0 .. k-1
template <int XF, int METRIC>
__global__ __launch_bounds__(256) void knn_exact_kernel(KnnParams p) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= p.nq) return;
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
  int64_t qlo, qhi;
  query_range(p, i, qlo, qhi);

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

  for (int c = 0; c < p.n_chunks; ++c) {
    const KnnMeta m = p.meta[(int64_t)c * p.nqp + i];
    if (!(m.flags & kKnnAllRows)) {
      for (int j0 = 0; j0 < m.count; j0 += 64) {
        const int j = j0 + lane;
        bool ok = j < m.count;
        int row = -1;
        if (ok) {
          const int64_t at = ((int64_t)c * p.C + j) * p.nqp + i;
          row = p.lr[at];
          ok = (double)p.ls[at] - knn_err<METRIC>(p.dim, qn, METRIC == RQSID_KNN_L2 ? p.xn[row] : 0.f) <= U;
        }
        offer(__ballot(ok), row);
      }
    } else {
      const int64_t c0 = (int64_t)c * p.chunk_rows;
      const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;
      const int64_t a = c0 > qlo ? c0 : qlo, b = c1 < qhi ? c1 : qhi;
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

struct KnnPlan : RowPairPlan {
  int64_t nqp, off_U, off_meta, off_ls, off_lr, bytes;
  int32_t C;
};

bool knn_plan(int64_t n_rows, int32_t nq, int32_t k, int32_t chunk_rows, KnnPlan& pl) {
  const bool ok = row_pair_plan(n_rows, nq, chunk_rows, pl);
  pl.nqp = pl.qtiles * kRowQ;
  pl.C = k + kKnnSlack;
  pl.off_U = pl.off_own;
  pl.off_meta = pl.off_U + up256(pl.nqp * 8);
  pl.off_ls = pl.off_meta + up256(pl.n_chunks * pl.nqp * (int64_t)sizeof(KnnMeta));
  pl.off_lr = pl.off_ls + up256(pl.n_chunks * pl.nqp * pl.C * 4);
  pl.bytes = pl.off_lr + up256(pl.n_chunks * pl.nqp * pl.C * 4);
  return ok;
}

int knn_check_k(const char* who, int32_t k) {
  if (k < 1 || k > RQSID_KNN_MAX) return fail(RQSID_E_ARG, "%s: k = %d (1 .. %d)", who, k, RQSID_KNN_MAX);
  return RQSID_OK;
}

template <int XF, int METRIC>
int knn_launch(const KnnParams& p, hipStream_t st) {
  int rc;
  constexpr int RULE = METRIC == RQSID_KNN_L2 ? kNormSqFinite : kNormInv;
  if ((rc = row_pair_prepare<XF, RULE, 3>("rqsid_row_knn", p, st))) return rc;
  hipLaunchKernelGGL((knn_screen_kernel<XF, METRIC>), dim3((unsigned)((int64_t)p.qtiles * p.n_chunks)), dim3(256), 0,
                     st, p);
  if ((rc = check_launch("rqsid_row_knn (screen)"))) return rc;
  hipLaunchKernelGGL(knn_fold_kernel<METRIC>, dim3((unsigned)cdiv(p.nq, 256)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_row_knn (fold)"))) return rc;
  hipLaunchKernelGGL((knn_exact_kernel<XF, METRIC>), dim3((unsigned)cdiv(p.nq, 4)), dim3(256), 0, st, p);
  return check_launch("rqsid_row_knn (exact)");
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int32_t rqsid_row_knn_tile_rows(void) { return kRowTile; }

int64_t rqsid_row_knn_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k, int32_t chunk_rows) {
  const char* const who = "rqsid_row_knn_workspace_bytes";
  int rc;
  if ((rc = row_pair_check_counts(who, n_rows, n_queries)) || (rc = knn_check_k(who, k)) ||
      (rc = row_pair_check_chunks(who, chunk_rows)))
    return rc;
  KnnPlan pl;
  if (!knn_plan(n_rows, n_queries, k, chunk_rows, pl)) return row_pair_fail_blocks(who, pl);
  return pl.bytes;
}

int rqsid_row_knn(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                  int32_t n_segments, const int32_t* seg_row_off, const void* q, int32_t n_queries,
                  const int32_t* query_self, const int32_t* query_seg, int32_t metric, int32_t k, int32_t chunk_rows,
                  int32_t* out_row, float* out_val, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "rqsid_row_knn";
  int rc;
  if ((rc = row_pair_check_format(who, x_format, dim))) return rc;
  if (metric != RQSID_KNN_L2 && metric != RQSID_KNN_COSINE)
    return fail(RQSID_E_ARG, "%s: unknown metric %d", who, metric);
  if ((rc = row_pair_check_counts(who, n_rows, n_queries)) || (rc = knn_check_k(who, k)) ||
      (rc = row_pair_check_chunks(who, chunk_rows, n_segments)))
    return rc;
  if (n_rows == 0 || n_queries == 0) return RQSID_OK;
  if (n_segments > 0 && !seg_row_off)
    return fail(RQSID_E_ARG, "%s: n_segments = %d needs seg_row_off", who, n_segments);
  if (query_seg && !seg_row_off) return fail(RQSID_E_ARG, "%s: query_seg needs seg_row_off", who);
  if ((rc = row_pair_check_rows(who, x, q))) return rc;
  if (!out_row || !out_val) return fail(RQSID_E_ARG, "%s: out_row and out_val are required", who);
  KnnPlan pl;
  if (!knn_plan(n_rows, n_queries, k, chunk_rows, pl)) return row_pair_fail_blocks(who, pl);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes,
                (long long)pl.bytes);
  char* ws = static_cast<char*>(workspace);
  KnnParams p;
  row_pair_fill(p, x, n_rows, dim, row_index, n_segments, n_segments > 0 ? seg_row_off : nullptr, q, n_queries,
                query_self, query_seg, workspace, pl);
  p.U = reinterpret_cast<double*>(ws + pl.off_U);
  p.meta = reinterpret_cast<KnnMeta*>(ws + pl.off_meta);
  p.ls = reinterpret_cast<float*>(ws + pl.off_ls);
  p.lr = reinterpret_cast<int32_t*>(ws + pl.off_lr);
  p.out_row = out_row;
  p.out_val = out_val;
  p.nqp = pl.nqp;
  p.k = k;
  p.C = pl.C;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_xf(x_format, [&](auto xf) {
    constexpr int XF = decltype(xf)::value;
    return metric == RQSID_KNN_L2 ? knn_launch<XF, RQSID_KNN_L2>(p, st) : knn_launch<XF, RQSID_KNN_COSINE>(p, st);
  });
}

}  // extern "C"
