// row_knn.hip — the exact k nearest rows of every query, over all rows or inside one segment (rqsid_row_knn;
// DESIGN.md §3.3c).
//
// Three kernels after the norms and the table check:
//  1. knn_screen_kernel: silhouette_kernel's block (128 queries x one chunk of 128-position tiles of the bucketed
//     order, fp32 images in LDS with the next chunk's loads in flight, v_mfma_f32_32x32x2_f32 with the base rows on
//     the A side).  The epilogue forms the metric's fp32 screen value s (L2: |q|^2 + |x|^2 - 2 D, cosine:
//     -D / (|q| |x|)), +inf for a position that is missing, outside the query's range, the self row or a row that
//     can never be a neighbour, and parks the tile in the idle operand images; one thread per query walks the
//     tile's positions and keeps the C = k + 8 smallest (s, row) of the chunk.  The kept list lives in the
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

constexpr int kKnnTile = 128;      // base positions per tile (4 MFMA blocks of 32)
constexpr int kKnnQ = 128;         // queries per block (32 per wave)
constexpr int kKnnStride = 36;     // floats per row of a chunk image: 32 + 4 of padding
constexpr int kKnnOp = kKnnTile * kKnnStride;  // floats per operand image
constexpr int kKnnDStride = 132;   // floats per position of the parked screen values (128 queries + 4)
constexpr int kKnnHeader = 256;    // workspace [0, 4): sticky error word, [4, 16): three counters
constexpr int kKnnTargetBlocks = 2048;  // chunk_rows = 0: at least this many blocks
constexpr int kKnnSlack = 8;       // list entries beyond k
constexpr int kKnnMV = kMaxDim / 4 / 64;  // float4 pieces of a row per lane of the exact pass
constexpr uint32_t kKnnErrRow = 1u;  // a row_index / query_self entry outside [0, n_rows)
constexpr uint32_t kKnnErrSeg = 2u;  // a query_seg entry outside [-1, n_segments)
constexpr uint32_t kKnnErrOff = 4u;  // a seg_row_off entry outside [0, n_rows] or decreasing
constexpr int kKnnFull = 1, kKnnBad = 2, kKnnAllRows = 4;  // KnnMeta::flags
static_assert(4 * kKnnOp >= kKnnTile * kKnnDStride, "the parked values fit in the operand images");

// what a block knows about one query after its chunk, beside the list itself
struct KnnMeta {
  float max_s;    // the largest kept s (meaningful when full)
  float xn_max;   // the largest |x|^2 among the chunk's rows the block met (L2: the worst-case e of the chunk)
  int32_t count;  // list entries
  int32_t flags;  // kKnnFull, kKnnBad (a non-finite s), kKnnAllRows (set by the fold: not certified)
};
static_assert(sizeof(KnnMeta) == 16, "record layout");

struct KnnParams {
  const void* x;
  const void* q;
  const int32_t* row_index;
  const int32_t* seg_off;
  const int32_t* query_self;
  const int32_t* query_seg;
  float* xn;      // [n_rows] L2: fl32(|x|^2); cosine: fl32(1 / |x|), NaN outside the screened range; -1: never a neighbour
  float* qn;      // [qtiles * kKnnQ] likewise; -1: a query without an answer
  double* U;      // [qtiles * kKnnQ]
  KnnMeta* meta;  // [n_chunks][qtiles * kKnnQ]
  float* ls;      // [n_chunks][C][qtiles * kKnnQ]
  int32_t* lr;    // likewise: row numbers
  uint32_t* err;  // the header: error word, then the three counters
  int32_t* out_row;
  float* out_val;
  int64_t n_rows;
  int64_t chunk_rows;
  int64_t nqp;    // qtiles * kKnnQ
  int32_t dim, n_seg, nq, qtiles, n_chunks, k, C;
};

__device__ __forceinline__ int64_t off_at(const KnnParams& p, int s) {
  const int64_t v = p.seg_off[s];
  return v < 0 ? 0 : (v > p.n_rows ? p.n_rows : v);
}
__device__ __forceinline__ int clean_seg(const KnnParams& p, int i) {
  const int v = p.query_seg ? p.query_seg[i] : -1;
  return (unsigned)v < (unsigned)p.n_seg ? v : -1;
}
__device__ __forceinline__ int clean_self(const KnnParams& p, int i) {
  const int v = p.query_self ? p.query_self[i] : -1;
  return (int64_t)(uint32_t)v < p.n_rows ? v : -1;
}
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

// per row: the norm term of the screen value, or -1 for a row that has no key (a non-finite element; cosine: |x| = 0)
template <int XF, int METRIC>
__global__ __launch_bounds__(256) void knn_norm_kernel(const void* __restrict__ src, int64_t n, int dim,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = dim / 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < n; row += (int64_t)gridDim.x * 4) {
    double s = 0.0;
    bool nf = false;
    for (int i = lane; i < nv; i += 64) {
      const float4 a = load_row4<XF>(static_cast<const float*>(src), row, dim, i);
      s += sq4(a);
      nf |= !(fabsf(a.x) <= FLT_MAX) | !(fabsf(a.y) <= FLT_MAX) | !(fabsf(a.z) <= FLT_MAX) | !(fabsf(a.w) <= FLT_MAX);
    }
    s = wave_sum(s);
    nf = __any(nf);
    float v;
    if constexpr (METRIC == RQSID_KNN_L2) {
      v = (float)s;
    } else {
      // the screen's interval is proven for 2^-30 <= |x| <= 2^30; outside, the NaN sends the pair to the exact pass
      v = (s >= 0x1p-60 && s <= 0x1p60) ? (float)(1.0 / sqrt(s)) : __uint_as_float(0x7FC00000u);
      nf |= s == 0.0;
    }
    if (lane == 0) out[row] = nf ? -1.0f : v;
  }
}

// the sticky error bits of the tables the kernels clamp instead of follow; block 0 zeroes the call's counters
__global__ __launch_bounds__(256) void knn_check_kernel(KnnParams p) {
  uint32_t errs = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 < 3) p.err[1 + i0] = 0u;
  if (p.seg_off)
    for (int64_t i = i0; i <= p.n_seg; i += stride) {
      const int64_t v = p.seg_off[i];
      if (v < 0 || v > p.n_rows || (i > 0 && v < (int64_t)p.seg_off[i - 1])) errs |= kKnnErrOff;
    }
  if (p.row_index)
    for (int64_t i = i0; i < p.n_rows; i += stride)
      if ((int64_t)(uint32_t)p.row_index[i] >= p.n_rows) errs |= kKnnErrRow;
  for (int64_t i = i0; i < p.nq; i += stride) {
    if (p.query_self) {
      const int v = p.query_self[i];
      if (v != -1 && (int64_t)(uint32_t)v >= p.n_rows) errs |= kKnnErrRow;
    }
    if (p.query_seg) {
      const int v = p.query_seg[i];
      if (v != -1 && (unsigned)v >= (unsigned)p.n_seg) errs |= kKnnErrSeg;
    }
  }
  if (errs) atomicOr(p.err, errs);
}

template <int XF, int METRIC>
__global__ __launch_bounds__(256, 2) void knn_screen_kernel(KnnParams p) {
  __shared__ __attribute__((aligned(16))) float s_buf[4 * kKnnOp];  // two (query, base) image pairs / the values
  __shared__ __attribute__((aligned(16))) int s_row[kKnnTile];
  __shared__ __attribute__((aligned(16))) float s_xn[kKnnTile];
  __shared__ int s_lo, s_hi, s_xmax;

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int qtile = (int)(blockIdx.x % (unsigned)p.qtiles), chunk = (int)(blockIdx.x / (unsigned)p.qtiles);
  const int q0 = qtile * kKnnQ;
  const int64_t c0 = (int64_t)chunk * p.chunk_rows;
  const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;
  const int nch = p.dim / kChunk;

  // staging role: thread t moves 16 B (f4 = t & 7) of base rows / queries (t >> 3) + 32 i of every chunk
  const int f4 = t & 7, srow = t >> 3;
  int my_q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) my_q[i] = q0 + srow + 32 * i < p.nq ? q0 + srow + 32 * i : -1;
  // the base row at a position of this chunk, or -1 (no address is formed from an entry outside [0, n_rows))
  auto row_at = [&](int64_t pos) {
    int row = -1;
    if (pos < c1) {
      row = p.row_index ? p.row_index[pos] : (int)pos;
      if ((int64_t)(uint32_t)row >= p.n_rows) row = -1;
    }
    return row;
  };
  uint4 xr[4], qr[4];
  auto load_chunk = [&](int r0, int r1, int r2, int r3, int ch) {  // (rows by value: nothing indexed in memory)
    const int i4 = ch * (kChunk / 4) + f4;
    const int rw[4] = {r0, r1, r2, r3};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xr[i] = rw[i] >= 0 ? load_raw<XF>(p.x, rw[i], p.dim, i4) : make_uint4(0u, 0u, 0u, 0u);
      qr[i] = my_q[i] >= 0 ? load_raw<XF>(p.q, my_q[i], p.dim, i4) : make_uint4(0u, 0u, 0u, 0u);
    }
  };

  // MFMA role: lane (r, h) of wave wv holds query q0 + 32 wv + r, its norm term, self row and range
  const int qcol = wv * 32 + r;
  const int myq = q0 + qcol;
  const float qn = myq < p.nq ? p.qn[myq] : -1.0f;
  const int self = myq < p.nq ? clean_self(p, myq) : -1;
  int64_t qlo = 0, qhi = 0;  // (a query without an answer searches nothing)
  if (myq < p.nq && !(qn < 0.f)) query_range(p, myq, qlo, qhi);

  // the union of the block's ranges: tiles outside it are skipped
  if (t == 0) {
    s_lo = INT_MAX;
    s_hi = 0;
    s_xmax = 0;
  }
  __syncthreads();
  if (h == 0 && qlo < qhi) {
    atomicMin(&s_lo, (int)qlo);
    atomicMax(&s_hi, (int)qhi);
  }
  __syncthreads();
  const int64_t ulo = s_lo, uhi = s_hi;
  const int ntile = (int)((c1 - c0 + kKnnTile - 1) / kKnnTile);
  const int tile0 = ulo > c0 ? (int)((ulo - c0) / kKnnTile < ntile ? (ulo - c0) / kKnnTile : ntile) : 0;
  int tile1 = uhi > c0 ? (int)((uhi - c0 + kKnnTile - 1) / kKnnTile) : 0;
  tile1 = tile1 < ntile ? tile1 : ntile;

  // walking role (threads 0..127): query q0 + t and its list in the workspace
  const int64_t wq = q0 + t;
  float* const ls = p.ls + (int64_t)chunk * p.C * p.nqp + wq;
  int32_t* const lr = p.lr + (int64_t)chunk * p.C * p.nqp + wq;
  int cnt = 0, bad = 0;
  float thr = INFINITY;  // what a value has to stay below to enter: +inf until the list is full, then its largest
  float mx = -INFINITY, xmax = 0.f;

  int rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows[i] = -1;
  if (tile0 < tile1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = row_at(c0 + (int64_t)tile0 * kKnnTile + srow + 32 * i);
    load_chunk(rows[0], rows[1], rows[2], rows[3], 0);
  }

  for (int tile = tile0; tile < tile1; ++tile) {
    const int64_t pos0 = c0 + (int64_t)tile * kKnnTile;
    // this tile's row numbers and norm terms for the epilogue, and the next tile's rows for the staging role
    int e_row = -1;
    float e_xn = 0.f;
    if (t < kKnnTile) {
      e_row = row_at(pos0 + t);
      e_xn = e_row >= 0 ? p.xn[e_row] : 0.f;
      if (e_xn < 0.f) e_row = -1;  // a row without a key is never a neighbour
      if (METRIC == RQSID_KNN_L2 && e_row >= 0) xmax = fmaxf(xmax, e_xn);
    }
    int nrows[4] = {-1, -1, -1, -1};
    if (tile + 1 < tile1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) nrows[i] = row_at(pos0 + kKnnTile + srow + 32 * i);
    }

    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

    for (int ch = 0; ch < nch; ++ch) {
      float* const sq = s_buf + (ch & 1) * 2 * kKnnOp;
      float* const sx = sq + kKnnOp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(sx + (srow + 32 * i) * kKnnStride + 4 * f4) = widen_raw<XF>(xr[i]);
        *reinterpret_cast<float4*>(sq + (srow + 32 * i) * kKnnStride + 4 * f4) = widen_raw<XF>(qr[i]);
      }
      // one barrier per chunk: the pair written here was last read two chunks ago, before the previous barrier
      __syncthreads();
      {  // the next chunk's loads (the next tile's first chunk after the last), in flight during the MFMAs
        const bool last = ch + 1 == nch;
        if (!last || tile + 1 < tile1)
          load_chunk(last ? nrows[0] : rows[0], last ? nrows[1] : rows[1], last ? nrows[2] : rows[2],
                     last ? nrows[3] : rows[3], last ? 0 : ch + 1);
      }
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        // lane half h takes dims 8 qd + 4 h .. + 3 of the chunk for its four k-steps (A and B alike)
        const float4 bv = *reinterpret_cast<const float4*>(sq + qcol * kKnnStride + 8 * qd + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float4 av = *reinterpret_cast<const float4*>(sx + (32 * b + r) * kKnnStride + 8 * qd + 4 * h);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[b], 0, 0, 0);
        }
      }
    }

    // ---- epilogue: screen values into the idle operand images ----
    if (t < kKnnTile) {
      s_row[t] = e_row;
      s_xn[t] = e_xn;
    }
    __syncthreads();  // every wave has finished the tile's MFMAs; s_row / s_xn are visible
    float* const s_d = s_buf;
    // the query's range in positions of this tile
    const int jlo = qlo - pos0 > 0 ? (qlo - pos0 < kKnnTile ? (int)(qlo - pos0) : kKnnTile) : 0;
    const int jhi = qhi - pos0 > 0 ? (qhi - pos0 < kKnnTile ? (int)(qhi - pos0) : kKnnTile) : 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // lane (r, h) holds base positions 32 b + 8 g + 4 h + k of the tile in acc[b][4 g + k]
        const int P = 32 * b + 8 * g + 4 * h;
        const float4 xn4 = *reinterpret_cast<const float4*>(s_xn + P);
        const int4 rw4 = *reinterpret_cast<const int4*>(s_row + P);
        const auto put = [&](int k, float dot, float xn, int rw) {
          float s;
          if constexpr (METRIC == RQSID_KNN_L2) s = fmaf(-2.0f, dot, qn + xn);
          else s = -((dot * qn) * xn);
          // a value the interval does not cover becomes -inf: it reaches the walk, which flags the chunk
          s = fabsf(s) <= FLT_MAX ? s : -INFINITY;
          const bool skip = (rw < 0) | (rw == self) | (P + k < jlo) | (P + k >= jhi);
          s_d[(P + k) * kKnnDStride + qcol] = skip ? INFINITY : s;
        };
        put(0, acc[b][4 * g + 0], xn4.x, rw4.x);
        put(1, acc[b][4 * g + 1], xn4.y, rw4.y);
        put(2, acc[b][4 * g + 2], xn4.z, rw4.z);
        put(3, acc[b][4 * g + 3], xn4.w, rw4.w);
      }
    __syncthreads();

    // ---- walk: one thread per query keeps the C smallest values of the chunk ----
    if (t < kKnnQ) {
      for (int j = 0; j < kKnnTile; j += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = s_d[(j + u) * kKnnDStride + t];
        bool any = false;
#pragma unroll
        for (int u = 0; u < 8; ++u) any |= v[u] < thr;
        if (any) {
#pragma unroll 1
          for (int u = 0; u < 8; ++u) {
            const float w = s_d[(j + u) * kKnnDStride + t];
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
    __syncthreads();  // the values are read before the next tile's images overwrite them
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = nrows[i];
  }

  if (METRIC == RQSID_KNN_L2 && t < kKnnTile) atomicMax(&s_xmax, __float_as_int(xmax));  // (xmax >= 0: int order)
  __syncthreads();
  if (t < kKnnQ) {
    KnnMeta m;
    m.max_s = thr;
    m.xn_max = __int_as_float(s_xmax);
    m.count = cnt;
    m.flags = (cnt == p.C ? kKnnFull : 0) | (bad ? kKnnBad : 0);
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

struct KnnPlan {
  int64_t chunk_rows, n_chunks, qtiles, nqp, off_xn, off_qn, off_U, off_meta, off_ls, off_lr, bytes;
  int32_t C;
};

// chunk_rows = 0: the fewest chunks that give kKnnTargetBlocks blocks (a fixed figure: the query needs no device)
bool knn_plan(int64_t n_rows, int32_t nq, int32_t k, int32_t chunk_rows, KnnPlan& pl) {
  const int64_t tiles = cdiv(n_rows, kKnnTile);
  pl.qtiles = cdiv(nq, kKnnQ);
  pl.nqp = pl.qtiles * kKnnQ;
  pl.C = k + kKnnSlack;
  if (chunk_rows == 0) {
    int64_t want = pl.qtiles > 0 ? cdiv(kKnnTargetBlocks, pl.qtiles) : 1;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    pl.chunk_rows = (tiles > 0 ? cdiv(tiles, want) : 1) * kKnnTile;
  } else {
    pl.chunk_rows = chunk_rows;
  }
  pl.n_chunks = cdiv(n_rows, pl.chunk_rows);
  const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
  pl.off_xn = kKnnHeader;
  pl.off_qn = pl.off_xn + up(n_rows * 4);
  pl.off_U = pl.off_qn + up(pl.nqp * 4);
  pl.off_meta = pl.off_U + up(pl.nqp * 8);
  pl.off_ls = pl.off_meta + up(pl.n_chunks * pl.nqp * (int64_t)sizeof(KnnMeta));
  pl.off_lr = pl.off_ls + up(pl.n_chunks * pl.nqp * pl.C * 4);
  pl.bytes = pl.off_lr + up(pl.n_chunks * pl.nqp * pl.C * 4);
  return pl.n_chunks * pl.qtiles <= INT32_MAX;
}

int knn_check_shape(const char* who, int64_t n_rows, int32_t nq, int32_t k, int32_t chunk_rows) {
  if (n_rows < 0 || n_rows > INT32_MAX) return fail(RQSID_E_ARG, "%s: n_rows = %lld", who, (long long)n_rows);
  if (nq < 0) return fail(RQSID_E_ARG, "%s: n_queries = %d", who, nq);
  if (k < 1 || k > RQSID_KNN_MAX) return fail(RQSID_E_ARG, "%s: k = %d (1 .. %d)", who, k, RQSID_KNN_MAX);
  if (chunk_rows < 0 || chunk_rows % kKnnTile)
    return fail(RQSID_E_ARG, "%s: chunk_rows = %d (0 or a positive multiple of %d)", who, chunk_rows, kKnnTile);
  return RQSID_OK;
}

template <int XF, int METRIC>
int knn_launch(const KnnParams& p, hipStream_t st) {
  int rc;
  const unsigned nb = grid_cap(cdiv(p.n_rows, 4), 16384), qb = grid_cap(cdiv(p.nq, 4), 16384);
  hipLaunchKernelGGL((knn_norm_kernel<XF, METRIC>), dim3(nb), dim3(256), 0, st, p.x, p.n_rows, p.dim, p.xn);
  if ((rc = check_launch("rqsid_row_knn (row norms)"))) return rc;
  hipLaunchKernelGGL((knn_norm_kernel<XF, METRIC>), dim3(qb), dim3(256), 0, st, p.q, (int64_t)p.nq, p.dim, p.qn);
  if ((rc = check_launch("rqsid_row_knn (query norms)"))) return rc;
  int64_t items = p.n_seg + 1 > p.nq ? p.n_seg + 1 : p.nq;
  if (p.row_index && p.n_rows > items) items = p.n_rows;
  hipLaunchKernelGGL(knn_check_kernel, dim3(grid_cap(cdiv(items, 256), 1024)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_row_knn (tables)"))) return rc;
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

int32_t rqsid_row_knn_tile_rows(void) { return kKnnTile; }

int64_t rqsid_row_knn_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k, int32_t chunk_rows) {
  int rc;
  if ((rc = knn_check_shape("rqsid_row_knn_workspace_bytes", n_rows, n_queries, k, chunk_rows))) return rc;
  KnnPlan pl;
  if (!knn_plan(n_rows, n_queries, k, chunk_rows, pl))
    return fail(RQSID_E_ARG, "rqsid_row_knn_workspace_bytes: %lld chunks x %lld query tiles exceed 2^31 - 1 blocks",
                (long long)pl.n_chunks, (long long)pl.qtiles);
  return pl.bytes;
}

int rqsid_row_knn(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                  int32_t n_segments, const int32_t* seg_row_off, const void* q, int32_t n_queries,
                  const int32_t* query_self, const int32_t* query_seg, int32_t metric, int32_t k, int32_t chunk_rows,
                  int32_t* out_row, float* out_val, void* workspace, int64_t workspace_bytes, void* stream) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "rqsid_row_knn: unknown x_format %d", x_format);
  if (dim <= 0 || dim % kChunk || dim > kMaxDim)
    return fail(RQSID_E_ARG, "rqsid_row_knn: dim = %d (a multiple of %d up to %d)", dim, kChunk, kMaxDim);
  if (metric != RQSID_KNN_L2 && metric != RQSID_KNN_COSINE)
    return fail(RQSID_E_ARG, "rqsid_row_knn: unknown metric %d", metric);
  int rc;
  if ((rc = knn_check_shape("rqsid_row_knn", n_rows, n_queries, k, chunk_rows))) return rc;
  if (n_segments < 0) return fail(RQSID_E_ARG, "rqsid_row_knn: n_segments = %d", n_segments);
  if (n_rows == 0 || n_queries == 0) return RQSID_OK;
  if (n_segments > 0 && !seg_row_off)
    return fail(RQSID_E_ARG, "rqsid_row_knn: n_segments = %d needs seg_row_off", n_segments);
  if (query_seg && !seg_row_off)
    return fail(RQSID_E_ARG, "rqsid_row_knn: query_seg needs seg_row_off");
  if (!x || !q || ((uintptr_t)x & 15) || ((uintptr_t)q & 15))
    return fail(RQSID_E_ARG, "rqsid_row_knn: x and q are required, 16-byte aligned");
  if (!out_row || !out_val) return fail(RQSID_E_ARG, "rqsid_row_knn: out_row and out_val are required");
  KnnPlan pl;
  if (!knn_plan(n_rows, n_queries, k, chunk_rows, pl))
    return fail(RQSID_E_ARG, "rqsid_row_knn: %lld chunks x %lld query tiles exceed 2^31 - 1 blocks",
                (long long)pl.n_chunks, (long long)pl.qtiles);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "rqsid_row_knn: workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)pl.bytes);
  char* ws = static_cast<char*>(workspace);
  KnnParams p;
  p.x = x;
  p.q = q;
  p.row_index = row_index;
  p.seg_off = n_segments > 0 ? seg_row_off : nullptr;
  p.query_self = query_self;
  p.query_seg = query_seg;
  p.xn = reinterpret_cast<float*>(ws + pl.off_xn);
  p.qn = reinterpret_cast<float*>(ws + pl.off_qn);
  p.U = reinterpret_cast<double*>(ws + pl.off_U);
  p.meta = reinterpret_cast<KnnMeta*>(ws + pl.off_meta);
  p.ls = reinterpret_cast<float*>(ws + pl.off_ls);
  p.lr = reinterpret_cast<int32_t*>(ws + pl.off_lr);
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.out_row = out_row;
  p.out_val = out_val;
  p.n_rows = n_rows;
  p.chunk_rows = pl.chunk_rows;
  p.nqp = pl.nqp;
  p.dim = dim;
  p.n_seg = n_segments;
  p.nq = n_queries;
  p.qtiles = (int32_t)pl.qtiles;
  p.n_chunks = (int32_t)pl.n_chunks;
  p.k = k;
  p.C = pl.C;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_xf(x_format, [&](auto xf) {
    constexpr int XF = decltype(xf)::value;
    return metric == RQSID_KNN_L2 ? knn_launch<XF, RQSID_KNN_L2>(p, st) : knn_launch<XF, RQSID_KNN_COSINE>(p, st);
  });
}

}  // extern "C"
