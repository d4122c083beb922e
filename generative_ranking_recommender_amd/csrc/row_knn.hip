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
// The record, the policy of the screen, the fold of one query and the exact pass of one query live in knn_core.h,
// which rqsid_probe_knn (probe_knn.hip) shares; here are the chunk geometry, the hull skip and the entry.
// The result is a function of the row set alone: e, the slack and chunk_rows move only the amount of fp64 work.
// No float atomics, no write positioned by a device counter.
#include "knn_core.h"

namespace rqsid {
namespace {

// the positions query i searches
__device__ __forceinline__ void query_range(const KnnParams& p, int i, int64_t& lo, int64_t& hi) {
  const int s = clean_seg(p, i);
  lo = s >= 0 ? off_at(p, s) : 0;
  hi = s >= 0 ? off_at(p, s + 1) : p.n_rows;
}

// knn_core.h's accessor: query i's lists are its chunks', [n_chunks][C][nqp]
struct ChunkLists {
  const KnnParams& p;
  int i;
  int64_t qlo, qhi;
  __device__ __forceinline__ int n() const { return p.n_chunks; }
  __device__ __forceinline__ int64_t meta_at(int c) const { return (int64_t)c * p.nqp + i; }
  __device__ __forceinline__ int64_t entry_at(int c, int j) const { return ((int64_t)c * p.C + j) * p.nqp + i; }
  __device__ __forceinline__ void range(int c, int64_t& a, int64_t& b) const {
    const int64_t c0 = (int64_t)c * p.chunk_rows;
    const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;
    a = c0 > qlo ? c0 : qlo;
    b = c1 < qhi ? c1 : qhi;
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
  knn_fold_query<METRIC>(p, i, ChunkLists{p, i, 0, 0});
}

// one wave per query: fp64 keys of the rows that can still place, ranked by (key, row) in lanes 0 .. k-1
template <int XF, int METRIC>
__global__ __launch_bounds__(256) void knn_exact_kernel(KnnParams p) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= p.nq) return;
  ChunkLists L{p, i, 0, 0};
  query_range(p, i, L.qlo, L.qhi);
  knn_exact_query<XF, METRIC>(p, i, lane, L);
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
  if ((rc = row_pair_check_format(who, x_format, dim)) || (rc = knn_check_metric(who, metric))) return rc;
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
