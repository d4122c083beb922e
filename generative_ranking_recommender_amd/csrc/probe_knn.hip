// probe_knn.hip — the exact k nearest rows of every query among the rows of a few position ranges of the order: the
// search through the ID index (rqsid_probe_knn).
//
// An ITEM is one (query, probe) pair, item = query * n_probes + probe; nothing is replicated: an item reads row
// item / n_probes of q in place.  After the norms and the table check of tile_rows.h:
//  1. probe_clean_kernel: one thread per query cleans its ranges (clamped into [0, n_rows], lo > hi and a range
//     that overlaps an earlier kept one made empty), writes out_scanned and each item's sort key, the tile number
//     of its range's start (the last key for an empty item); every list record starts out "uncertified".
//  2. rqsid_bucket over the keys: the items ordered by where their range starts.  The order only decides which
//     items share a block; probe_slots_kernel turns it into the block columns' item and query-row tables.
//  3. probe_screen_kernel: a block takes G consecutive items of that order (G = 128, fewer when the items are few, so
//     that their runs spread over the device) as the first G columns of tile_rows.h's block.
//     It sorts their (first tile, last tile) intervals in LDS, merges those that touch into runs and sweeps run
//     after run with row_tile_sweep and knn_core.h's KnnPolicy, each column limited to its item's range: no tile is
//     visited twice, and tiles between far-apart items are not visited at all.  A column keeps the k + 8 smallest
//     screen values of its item in the workspace list of that item.
//  4. probe_fold_kernel (one thread per query, knn_fold_query over its n_probes lists) and probe_exact_kernel (one
//     wave per query, knn_exact_query): U over every kept entry of the query, the certificate per item, fp64 keys
//     of what can still place and of every row of an uncertified item's range.
// The result is a function of the row set alone.  No float atomics; the only writes placed through a counter are
// rqsid_bucket's, whose result no output depends on.
#include "knn_core.h"

namespace rqsid {
namespace {

constexpr uint32_t kProbeErrRange = 4u;    // a range end outside [0, n_rows], or lo > hi
constexpr uint32_t kProbeErrOverlap = 8u;  // two ranges of one query overlap: the later one is dropped
constexpr int kProbeMaxKeys = 65536;       // segments of the item sort; more tiles share keys

struct ProbeParams : KnnParams {
  const int32_t* probe_lo;
  const int32_t* probe_hi;
  int32_t* clo;        // [nip] the cleaned ranges, by item
  int32_t* chi;
  int32_t* key;        // [nip] sort keys
  int32_t* perm;       // [nip] rqsid_bucket's row_index over the items
  int32_t* slot_item;  // [n_blocks * kRowQ] column -> item, -1: none
  int32_t* slot_q;     // likewise: column -> row of q, -1: none (RowPairParams::q_row)
  int32_t* out_scanned;
  int32_t* bucket_err;  // rqsid_bucket's error word inside this workspace
  int64_t n_items, n_slots;
  int32_t P, S, shift, G;  // G: items per block
};

__global__ __launch_bounds__(256) void probe_clean_kernel(ProbeParams p) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g == 0) *p.bucket_err = 0;
  if (g < p.nqp) {
    p.perm[g] = -1;
    // a list no block writes (the item missing from the order) is walked row by row
    KnnMeta m;
    m.max_s = m.xn_max = 0.f;
    m.count = 0;
    m.flags = kKnnBad;
    p.meta[g] = m;
  }
  if (g >= p.nq) return;
  const int i = (int)g;
  const bool answer = !(p.qn[i] < 0.f);
  uint32_t errs = 0;
  int64_t scanned = 0;
  for (int c = 0; c < p.P; ++c) {
    const int64_t item = (int64_t)i * p.P + c;
    int64_t lo = p.probe_lo[item], hi = p.probe_hi[item];
    if (lo < 0 || lo > p.n_rows || hi < 0 || hi > p.n_rows || lo > hi) errs |= kProbeErrRange;
    lo = lo < 0 ? 0 : (lo > p.n_rows ? p.n_rows : lo);
    hi = hi < 0 ? 0 : (hi > p.n_rows ? p.n_rows : hi);
    if (lo > hi) hi = lo;
    for (int b = 0; b < c && lo < hi; ++b) {
      const int64_t blo = p.clo[item - c + b], bhi = p.chi[item - c + b];
      if (blo < bhi && lo < bhi && blo < hi) {
        errs |= kProbeErrOverlap;
        hi = lo;
      }
    }
    p.clo[item] = (int32_t)lo;
    p.chi[item] = (int32_t)hi;
    scanned += hi - lo;
    p.key[item] = (lo < hi && answer) ? (int32_t)((lo / kRowTile) >> p.shift) : p.S - 1;
  }
  if (p.out_scanned) p.out_scanned[i] = (int32_t)scanned;
  if (errs) atomicOr(p.err, errs);
}

__global__ __launch_bounds__(256) void probe_slots_kernel(ProbeParams p) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= p.n_slots) return;
  // column col of block s / kRowQ is place (s / kRowQ) G + col of the order, for col < G
  const int col = (int)(s % kRowQ);
  const int64_t at = s / kRowQ * p.G + col;
  int item = col < p.G && at < p.n_items ? p.perm[at] : -1;
  if ((int64_t)(uint32_t)item >= p.n_items) item = -1;
  p.slot_item[s] = item;
  p.slot_q[s] = item >= 0 ? item / p.P : -1;
}

template <int XF, int METRIC>
__global__ __launch_bounds__(256, 2) void probe_screen_kernel(ProbeParams p) {
  const RowTileLds lds = row_tile_lds();
  __shared__ int s_a[kRowQ], s_b[kRowQ];  // the sorted intervals, then the runs: first and last tile
  __shared__ int s_nrun, s_xmax;

  const int t = threadIdx.x;
  const int q0 = blockIdx.x * kRowQ;

  const int mitem = p.slot_item[q0 + (t >> 6) * 32 + (t & 31)];
  const int mq = mitem >= 0 ? mitem / p.P : -1;
  KnnPolicy<METRIC> w{p};
  w.qn = mq >= 0 ? p.qn[mq] : -1.0f;
  w.self = mq >= 0 ? clean_self(p, mq) : -1;
  w.qlo = w.qhi = 0;  // (a query without an answer searches nothing)
  if (mq >= 0 && !(w.qn < 0.f)) {
    w.qlo = p.clo[mitem];
    w.qhi = p.chi[mitem];
  }
  const int witem = t < kRowQ ? p.slot_item[q0 + t] : -1;
  w.ls = p.ls + (witem >= 0 ? witem : 0);
  w.lr = p.lr + (witem >= 0 ? witem : 0);
  w.cnt = w.bad = 0;
  w.thr = INFINITY;
  w.mx = -INFINITY;
  w.xmax = 0.f;

  // the columns' tile intervals, sorted by (first tile, column) and merged into runs of tiles
  int* const s_first = reinterpret_cast<int*>(lds.s_buf);  // (idle until the sweep)
  int first = INT_MAX, last = -1;
  if (witem >= 0 && !(p.qn[witem / p.P] < 0.f)) {
    const int lo = p.clo[witem], hi = p.chi[witem];
    if (lo < hi) {
      first = lo / kRowTile;
      last = (hi - 1) / kRowTile;
    }
  }
  if (t < kRowQ) s_first[t] = first;
  if (t == 0) s_xmax = 0;
  __syncthreads();
  if (t < kRowQ) {
    int rank = 0;
    for (int u = 0; u < kRowQ; ++u) {
      const int f = s_first[u];
      rank += (f < first) | ((f == first) & (u < t));
    }
    s_a[rank] = first;
    s_b[rank] = last;
  }
  __syncthreads();
  if (t == 0) {
    int nrun = 0, visits = 0;
    for (int j = 0; j < kRowQ; ++j) {
      const int f = s_a[j], l = s_b[j];
      if (f == INT_MAX) break;
      if (nrun > 0 && f <= s_b[nrun - 1] + 1) {  // shares a tile with the run, or continues it
        if (l > s_b[nrun - 1]) s_b[nrun - 1] = l;
      } else {
        s_a[nrun] = f;
        s_b[nrun] = l;
        ++nrun;
      }
    }
    for (int r = 0; r < nrun; ++r) visits += s_b[r] - s_a[r] + 1;
    s_nrun = nrun;
    if (visits) atomicAdd(reinterpret_cast<int*>(p.err) + 4, visits);
  }
  __syncthreads();

  const int nrun = s_nrun;
  for (int r = 0; r < nrun; ++r) {
    // (s_first, in the images the sweep writes, was last read before the barriers above)
    row_tile_sweep<XF>(p, q0, 0, p.n_rows, s_a[r], s_b[r] + 1, lds, w);
  }

  if (METRIC == RQSID_KNN_L2 && t < kRowTile) atomicMax(&s_xmax, __float_as_int(w.xmax));  // (xmax >= 0: int order)
  __syncthreads();
  if (witem >= 0) {
    KnnMeta m;
    m.max_s = w.thr;
    m.xn_max = __int_as_float(s_xmax);
    m.count = w.cnt;
    m.flags = (w.cnt == p.C ? kKnnFull : 0) | (w.bad ? kKnnBad : 0);
    p.meta[witem] = m;
  }
}

// knn_core.h's accessor: query i's lists are its items', [C][nip]
struct ItemLists {
  const ProbeParams& p;
  int i;
  __device__ __forceinline__ int n() const { return p.P; }
  __device__ __forceinline__ int64_t meta_at(int c) const { return (int64_t)i * p.P + c; }
  __device__ __forceinline__ int64_t entry_at(int c, int j) const { return (int64_t)j * p.nqp + (int64_t)i * p.P + c; }
  __device__ __forceinline__ void range(int c, int64_t& a, int64_t& b) const {
    a = p.clo[(int64_t)i * p.P + c];
    b = p.chi[(int64_t)i * p.P + c];
  }
};

template <int METRIC>
__global__ __launch_bounds__(256) void probe_fold_kernel(ProbeParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nq) return;
  knn_fold_query<METRIC>(p, i, ItemLists{p, i});
}

template <int XF, int METRIC>
__global__ __launch_bounds__(256) void probe_exact_kernel(ProbeParams p) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= p.nq) return;
  knn_exact_query<XF, METRIC>(p, i, lane, ItemLists{p, i});
}

constexpr int kProbeTargetBlocks = 1024;  // fewer items than 128 of these blocks' worth: fewer items per block

struct ProbePlan : RowPairPlan {
  int64_t n_items, nip, n_blocks, s_cap, bucket_bytes, bytes;
  int64_t off_U, off_meta, off_ls, off_lr, off_clo, off_chi, off_key, off_perm, off_sitem, off_sq, off_soff,
      off_toff, off_bucket;
  int32_t C, S, shift, G;
};

// every term grows with its argument: the size query is monotone (the bucket area is sized for the key count's
// cap and for the larger of rqsid_bucket's two layouts)
void probe_plan(int64_t n_rows, int32_t nq, int32_t n_probes, int32_t k, ProbePlan& pl) {
  row_pair_plan(n_rows, nq, 0, pl);
  pl.n_items = (int64_t)nq * n_probes;
  pl.nip = cdiv(pl.n_items, kRowQ) * kRowQ;
  pl.C = k + kKnnSlack;
  // items per block: 128 once that gives kProbeTargetBlocks blocks, else what gives about that many, at least 1.
  // Fewer than 2 kProbeTargetBlocks + 1 blocks whenever G < 128 (G >= items / (2 kProbeTargetBlocks) there), so the
  // column tables are sized for that or for G = 128, whichever is larger: monotone in the item count
  const int64_t g = pl.n_items / kProbeTargetBlocks;
  pl.G = (int32_t)(g < 1 ? 1 : (g > kRowQ ? kRowQ : g));
  pl.n_blocks = cdiv(pl.n_items, pl.G);
  const int64_t few = pl.n_items < 2 * kProbeTargetBlocks + 1 ? pl.n_items : 2 * kProbeTargetBlocks + 1;
  const int64_t cap_blocks = pl.nip / kRowQ > few ? pl.nip / kRowQ : few;
  const int64_t tiles = cdiv(n_rows, kRowTile);
  pl.shift = 0;
  while ((tiles >> pl.shift) + 2 > kProbeMaxKeys) ++pl.shift;
  pl.S = (int32_t)((tiles >> pl.shift) + 2);
  pl.s_cap = tiles + 2 < kProbeMaxKeys ? tiles + 2 : kProbeMaxKeys;
  pl.bucket_bytes = bucket_workspace_words_up_to(pl.s_cap) * 4;
  int64_t at = pl.off_own;
  const auto take = [&](int64_t bytes) {
    const int64_t o = at;
    at += up256(bytes);
    return o;
  };
  pl.off_U = take((int64_t)pl.qtiles * kRowQ * 8);
  pl.off_meta = take(pl.nip * (int64_t)sizeof(KnnMeta));
  pl.off_ls = take(pl.nip * pl.C * 4);
  pl.off_lr = take(pl.nip * pl.C * 4);
  pl.off_clo = take(pl.nip * 4);
  pl.off_chi = take(pl.nip * 4);
  pl.off_key = take(pl.nip * 4);
  pl.off_perm = take(pl.nip * 4);
  pl.off_sitem = take(cap_blocks * kRowQ * 4);
  pl.off_sq = take(cap_blocks * kRowQ * 4);
  pl.off_soff = take((pl.s_cap + 1) * 4);
  pl.off_toff = take((pl.s_cap + 1) * 4);
  pl.off_bucket = take(pl.bucket_bytes);
  pl.bytes = at;
}

int probe_check_counts(const char* who, int64_t n_rows, int32_t nq, int32_t n_probes, int32_t k) {
  int rc;
  if ((rc = row_pair_check_counts(who, n_rows, nq)) || (rc = knn_check_k(who, k))) return rc;
  if (n_probes < 1 || n_probes > RQSID_PROBE_MAX)
    return fail(RQSID_E_ARG, "%s: n_probes = %d (1 .. %d)", who, n_probes, RQSID_PROBE_MAX);
  if ((int64_t)nq * n_probes > INT32_MAX)
    return fail(RQSID_E_ARG, "%s: %d queries x %d probes exceed 2^31 - 1 items", who, nq, n_probes);
  return RQSID_OK;
}

template <int XF, int METRIC>
int probe_launch(const ProbeParams& p, const ProbePlan& pl, void* bucket_ws, int32_t* seg_off, int32_t* tile_off,
                 hipStream_t st) {
  const char* const who = "rqsid_probe_knn";
  int rc;
  constexpr int RULE = METRIC == RQSID_KNN_L2 ? kNormSqFinite : kNormInv;
  if ((rc = row_pair_prepare<XF, RULE, 4>(who, p, st))) return rc;
  const int64_t span = p.nqp > p.nq ? p.nqp : p.nq;
  hipLaunchKernelGGL(probe_clean_kernel, dim3((unsigned)cdiv(span, 256)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_probe_knn (ranges)"))) return rc;
  if ((rc = rqsid_bucket(p.key, p.n_items, p.S, 0, seg_off, tile_off, p.perm, bucket_ws, pl.bucket_bytes, st)))
    return rc;
  hipLaunchKernelGGL(probe_slots_kernel, dim3((unsigned)cdiv(p.n_slots, 256)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_probe_knn (order)"))) return rc;
  hipLaunchKernelGGL((probe_screen_kernel<XF, METRIC>), dim3((unsigned)(p.n_slots / kRowQ)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_probe_knn (screen)"))) return rc;
  hipLaunchKernelGGL(probe_fold_kernel<METRIC>, dim3((unsigned)cdiv(p.nq, 256)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_probe_knn (fold)"))) return rc;
  hipLaunchKernelGGL((probe_exact_kernel<XF, METRIC>), dim3((unsigned)cdiv(p.nq, 4)), dim3(256), 0, st, p);
  return check_launch("rqsid_probe_knn (exact)");
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int64_t rqsid_probe_knn_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t n_probes, int32_t k) {
  int rc;
  if ((rc = probe_check_counts("rqsid_probe_knn_workspace_bytes", n_rows, n_queries, n_probes, k))) return rc;
  ProbePlan pl;
  probe_plan(n_rows, n_queries, n_probes, k, pl);
  return pl.bytes;
}

int rqsid_probe_knn(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                    const void* q, int32_t n_queries, const int32_t* query_self, int32_t n_probes,
                    const int32_t* probe_lo, const int32_t* probe_hi, int32_t metric, int32_t k, int32_t* out_row,
                    float* out_val, int32_t* out_scanned, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "rqsid_probe_knn";
  int rc;
  if ((rc = row_pair_check_format(who, x_format, dim)) || (rc = knn_check_metric(who, metric)) ||
      (rc = probe_check_counts(who, n_rows, n_queries, n_probes, k)))
    return rc;
  if (n_rows == 0 || n_queries == 0) return RQSID_OK;
  if ((rc = row_pair_check_rows(who, x, q))) return rc;
  if (!probe_lo || !probe_hi) return fail(RQSID_E_ARG, "%s: probe_lo and probe_hi are required", who);
  if (!out_row || !out_val) return fail(RQSID_E_ARG, "%s: out_row and out_val are required", who);
  ProbePlan pl;
  probe_plan(n_rows, n_queries, n_probes, k, pl);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes,
                (long long)pl.bytes);
  if (rqsid_bucket_workspace_bytes(pl.n_items, pl.S) > pl.bucket_bytes)  // (before any launch, not inside the call)
    return fail(RQSID_E_WORKSPACE, "%s: the item sort needs more than the %lld bytes planned for it", who,
                (long long)pl.bucket_bytes);
  char* ws = static_cast<char*>(workspace);
  const auto i32 = [&](int64_t off) { return reinterpret_cast<int32_t*>(ws + off); };
  ProbeParams p;
  row_pair_fill(p, x, n_rows, dim, row_index, 0, nullptr, q, n_queries, query_self, nullptr, workspace, pl);
  p.U = reinterpret_cast<double*>(ws + pl.off_U);
  p.meta = reinterpret_cast<KnnMeta*>(ws + pl.off_meta);
  p.ls = reinterpret_cast<float*>(ws + pl.off_ls);
  p.lr = i32(pl.off_lr);
  p.out_row = out_row;
  p.out_val = out_val;
  p.nqp = pl.nip;
  p.k = k;
  p.C = pl.C;
  p.probe_lo = probe_lo;
  p.probe_hi = probe_hi;
  p.clo = i32(pl.off_clo);
  p.chi = i32(pl.off_chi);
  p.key = i32(pl.off_key);
  p.perm = i32(pl.off_perm);
  p.slot_item = i32(pl.off_sitem);
  p.slot_q = i32(pl.off_sq);
  p.q_row = p.slot_q;
  p.out_scanned = out_scanned;
  p.bucket_err = i32(pl.off_bucket) + bucket_error_word_at(pl.S);
  p.n_items = pl.n_items;
  p.n_slots = pl.n_blocks * kRowQ;
  p.G = pl.G;
  p.P = n_probes;
  p.S = pl.S;
  p.shift = pl.shift;
  hipStream_t st = (hipStream_t)stream;
  return dispatch_xf(x_format, [&](auto xf) {
    constexpr int XF = decltype(xf)::value;
    return metric == RQSID_KNN_L2
               ? probe_launch<XF, RQSID_KNN_L2>(p, pl, ws + pl.off_bucket, i32(pl.off_soff), i32(pl.off_toff), st)
               : probe_launch<XF, RQSID_KNN_COSINE>(p, pl, ws + pl.off_bucket, i32(pl.off_soff), i32(pl.off_toff),
                                                    st);
  });
}

}  // extern "C"
