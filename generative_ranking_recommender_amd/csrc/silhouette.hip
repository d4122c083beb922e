// silhouette.hip — exact silhouette sums of scored rows against every cluster (rqsid_silhouette).
//
// For every query i and every cluster c the sum S(i, c) of the TRUE pairwise distances from i to the members of c,
// from which a (own cluster), b (nearest other cluster by mean distance) and s = (b - a) / max(a, b) follow.  No
// centroid identity exists for unsquared distances, so this is m x n x dim matrix work plus a segmented reduction.
//
// Shape.  The base rows are walked in the bucketed order (row_index) in fixed tiles of 128 positions that straddle
// segments; a block owns 128 queries and one chunk of consecutive tiles.  Per tile and 32-dim chunk the block stages
// fp32 images of the 128 base rows and of its 128 queries in LDS (144-B pitch, 16-bit rows widened as they are
// staged; two image pairs, so a chunk costs one barrier, with the next chunk's global loads in flight during the
// MFMAs) and runs v_mfma_f32_32x32x2_f32 with the base rows on the A side and the queries on the B side: lane
// (r, h) of wave w then holds query 32 w + r against 64 base rows.  The epilogue forms d = sqrt(max(0, |q|^2 +
// |x|^2 - 2 D)), zeroes the self row and rows that do not exist, and parks the tile's 128 x 128 distances in the
// (now idle) operand images; 128 threads, one per query, then walk the tile's positions in order with the segment
// boundaries as wave-uniform control flow: an fp32 sum per (tile, segment) piece, added in fp64 to the running
// segment sum; a segment that ends becomes the own-cluster sum or competes for b.  Per (query, chunk) the block
// writes one record; a second kernel folds a query's records in chunk order.  No float atomics: the result is a
// pure function of the arguments (the per-piece fp32 sums do not even depend on chunk_rows).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "assign_common.h"
#include "tile_rows.h"

namespace rqsid {
namespace {

constexpr int kSilTile = 128;      // base positions per tile (4 MFMA blocks of 32)
constexpr int kSilQ = 128;         // queries per block (32 per wave)
constexpr int kSilStride = 36;     // floats per row of a chunk image: 32 + 4 of padding (topk_kernel.h)
constexpr int kSilOp = kSilTile * kSilStride;  // floats per operand image
constexpr int kSilDStride = 132;   // floats per position of the parked distances (128 queries + 4)
constexpr int kSilHeader = 256;    // workspace [0, 4): sticky error word
constexpr int kSilTargetBlocks = 2048;  // chunk_rows = 0: at least this many blocks (8 per CU of an MI355X)
constexpr uint32_t kSilErrRow = 1u;  // a row_index / query_self entry outside [0, n_rows)
constexpr uint32_t kSilErrSeg = 2u;  // a query_seg entry outside [-1, n_segments)
constexpr uint32_t kSilErrOff = 4u;  // a seg_row_off entry outside [0, n_rows] or decreasing
static_assert(4 * kSilOp >= kSilTile * kSilDStride, "the parked distances fit in the operand images");

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

struct SilParams {
  const void* x;
  const void* q;
  const int32_t* row_index;
  const int32_t* seg_off;
  const int32_t* query_self;
  const int32_t* query_seg;
  float* xn;   // [n_rows] |x_row|^2, by row
  float* qn;   // [qtiles * kSilQ]
  SilRecord* rec;  // [n_chunks][qtiles * kSilQ]
  uint32_t* err;
  float* out_a;
  float* out_b;
  int32_t* out_b_seg;
  float* out_s;
  int64_t n_rows;
  int64_t chunk_rows;
  int32_t dim, n_seg, nq, qtiles, n_chunks;
};

// a segment offset as the kernels use it: inside [0, n_rows] whatever the table holds
__device__ __forceinline__ int64_t off_at(const SilParams& p, int s) {
  const int64_t v = p.seg_off[s];
  return v < 0 ? 0 : (v > p.n_rows ? p.n_rows : v);
}
__device__ __forceinline__ int clean_seg(const SilParams& p, int i) {
  const int v = p.query_seg ? p.query_seg[i] : -1;
  return (unsigned)v < (unsigned)p.n_seg ? v : -1;
}
__device__ __forceinline__ int clean_self(const SilParams& p, int i) {
  const int v = p.query_self ? p.query_self[i] : -1;
  return (int64_t)(uint32_t)v < p.n_rows ? v : -1;
}

// out[row] = fl32(fp64 sum of squares): one wave per row, lanes over 16-B pieces (c_meta's |c|^2 rule)
template <int XF>
__global__ __launch_bounds__(256) void sil_norm_kernel(const void* __restrict__ src, int64_t n, int dim,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = dim / 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < n; row += (int64_t)gridDim.x * 4) {
    double s = 0.0;
    for (int i = lane; i < nv; i += 64) {
      const float4 a = load_row4<XF>(static_cast<const float*>(src), row, dim, i);
      s += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = (float)s;
  }
}

// the sticky error bits of the tables the kernels clamp instead of follow
__global__ __launch_bounds__(256) void sil_check_kernel(SilParams p) {
  uint32_t errs = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= p.n_seg; i += stride) {
    const int64_t v = p.seg_off[i];
    if (v < 0 || v > p.n_rows || (i > 0 && v < (int64_t)p.seg_off[i - 1])) errs |= kSilErrOff;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.nq; i += stride) {
    if (p.query_self) {
      const int v = p.query_self[i];
      if (v != -1 && (int64_t)(uint32_t)v >= p.n_rows) errs |= kSilErrRow;
    }
    if (p.query_seg) {
      const int v = p.query_seg[i];
      if (v != -1 && (unsigned)v >= (unsigned)p.n_seg) errs |= kSilErrSeg;
    }
  }
  if (errs) atomicOr(p.err, errs);
}

template <int XF>
__global__ __launch_bounds__(256, 2) void silhouette_kernel(SilParams p) {
  __shared__ __attribute__((aligned(16))) float s_buf[4 * kSilOp];  // two (query, base) image pairs / the distances
  __shared__ __attribute__((aligned(16))) int s_row[kSilTile];
  __shared__ __attribute__((aligned(16))) float s_xn[kSilTile];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int qtile = (int)(blockIdx.x % (unsigned)p.qtiles), chunk = (int)(blockIdx.x / (unsigned)p.qtiles);
  const int q0 = qtile * kSilQ;
  const int64_t c0 = (int64_t)chunk * p.chunk_rows;
  const int64_t c1 = c0 + p.chunk_rows < p.n_rows ? c0 + p.chunk_rows : p.n_rows;
  const int ntile = (int)((c1 - c0 + kSilTile - 1) / kSilTile);
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

  // MFMA role: lane (r, h) of wave wv holds query q0 + 32 wv + r
  const int qcol = wv * 32 + r;
  const int myq = q0 + qcol;
  const float qn = myq < p.nq ? p.qn[myq] : 0.f;
  const int self = myq < p.nq ? clean_self(p, myq) : -1;

  // walking role (threads 0..127): query q0 + t and the chunk's running state
  const int wq = q0 + t;
  const int my_seg = (t < kSilQ && wq < p.nq) ? clean_seg(p, wq) : -1;
  int seg = 0;            // the first segment that ends after the walk's position (block-uniform)
  {
    int lo = 0, hi = p.n_seg;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (off_at(p, mid + 1) > c0) hi = mid;
      else lo = mid + 1;
    }
    seg = lo;
  }
  double cur = 0.0;       // the open segment's sum inside this chunk
  bool open = false;
  SilRecord rec;
  rec.first_sum = rec.last_sum = rec.own_sum = 0.0;
  rec.best = INFINITY;
  rec.first_seg = rec.last_seg = rec.best_seg = -1;
  rec.bad = 0;
  uint32_t errs = 0;

  int rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows[i] = row_at(c0 + srow + 32 * i);
  load_chunk(rows[0], rows[1], rows[2], rows[3], 0);

  for (int tile = 0; tile < ntile; ++tile) {
    const int64_t pos0 = c0 + (int64_t)tile * kSilTile;
    // this tile's row numbers and norms for the epilogue, and the next tile's rows for the staging role
    int e_row = -1;
    float e_xn = 0.f;
    if (t < kSilTile) {
      e_row = row_at(pos0 + t);
      if (pos0 + t < c1 && e_row < 0) errs |= kSilErrRow;
      e_xn = e_row >= 0 ? p.xn[e_row] : 0.f;
    }
    int nrows[4] = {-1, -1, -1, -1};
    if (tile + 1 < ntile) {
#pragma unroll
      for (int i = 0; i < 4; ++i) nrows[i] = row_at(pos0 + kSilTile + srow + 32 * i);
    }

    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

    for (int ch = 0; ch < nch; ++ch) {
      float* const sq = s_buf + (ch & 1) * 2 * kSilOp;
      float* const sx = sq + kSilOp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(sx + (srow + 32 * i) * kSilStride + 4 * f4) = widen_raw<XF>(xr[i]);
        *reinterpret_cast<float4*>(sq + (srow + 32 * i) * kSilStride + 4 * f4) = widen_raw<XF>(qr[i]);
      }
      // one barrier per chunk: the pair written here was last read two chunks ago, before the previous barrier
      __syncthreads();
      {  // the next chunk's loads (the next tile's first chunk after the last), in flight during the MFMAs
        const bool last = ch + 1 == nch;
        if (!last || tile + 1 < ntile)
          load_chunk(last ? nrows[0] : rows[0], last ? nrows[1] : rows[1], last ? nrows[2] : rows[2],
                     last ? nrows[3] : rows[3], last ? 0 : ch + 1);
      }
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        // lane half h takes dims 8 qd + 4 h .. + 3 of the chunk for its four k-steps (A and B alike)
        const float4 bv = *reinterpret_cast<const float4*>(sq + qcol * kSilStride + 8 * qd + 4 * h);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float4 av = *reinterpret_cast<const float4*>(sx + (32 * b + r) * kSilStride + 8 * qd + 4 * h);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[b], 0, 0, 0);
        }
      }
    }

    // ---- epilogue: distances into the idle operand images ----
    if (t < kSilTile) {
      s_row[t] = e_row;
      s_xn[t] = e_xn;
    }
    __syncthreads();  // every wave has finished the tile's MFMAs; s_row / s_xn are visible
    float* const s_d = s_buf;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // lane (r, h) holds base positions 32 b + 8 g + 4 h + k of the tile in acc[b][4 g + k]
        const int P = 32 * b + 8 * g + 4 * h;
        const float4 xn4 = *reinterpret_cast<const float4*>(s_xn + P);
        const int4 rw4 = *reinterpret_cast<const int4*>(s_row + P);
        const auto put = [&](int k, float dot, float xn, int rw) {
          float tt = fmaf(-2.0f, dot, qn + xn);
          // the self row is excluded by INDEX and a position without a row adds nothing: their argument is zeroed
          // (sqrt(0) = 0) rather than their root branched around; a NaN stays a NaN
          const bool skip = (rw < 0) | (rw == self);
          tt = (skip | (tt < 0.f)) ? 0.f : tt;
          s_d[(P + k) * kSilDStride + qcol] = sqrtf(tt);
        };
        put(0, acc[b][4 * g + 0], xn4.x, rw4.x);
        put(1, acc[b][4 * g + 1], xn4.y, rw4.y);
        put(2, acc[b][4 * g + 2], xn4.z, rw4.z);
        put(3, acc[b][4 * g + 3], xn4.w, rw4.w);
      }
    __syncthreads();

    // ---- walk: one thread per query, the tile's positions in order, segment boundaries as uniform branches ----
    if (t < kSilQ) {
      int64_t pos = pos0;
      const int64_t tend = pos0 + kSilTile < c1 ? pos0 + kSilTile : c1;
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
          for (int u = 0; u < 8; ++u) v[u] = s_d[(j + u) * kSilDStride + t];
#pragma unroll
          for (int u = 0; u < 8; ++u) ps += v[u];
        }
        for (; j < je; ++j) ps += s_d[j * kSilDStride + t];
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
    __syncthreads();  // the distances are read before the next tile's images overwrite them
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = nrows[i];
  }

  if (errs) atomicOr(p.err, errs);
  if (t < kSilQ) {
    if (open) {  // a segment that runs past the chunk's end
      if (off_at(p, seg) < c0) {
        rec.first_seg = seg;
        rec.first_sum = cur;
      } else {
        rec.last_seg = seg;
        rec.last_sum = cur;
      }
    }
    p.rec[(int64_t)chunk * p.qtiles * kSilQ + wq] = rec;
  }
}

// a query's records in chunk order -> a, b, b_seg, s
__global__ __launch_bounds__(256) void sil_fold_kernel(SilParams p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nq) return;
  const int my_seg = clean_seg(p, i);
  const int self = clean_self(p, i);
  const int64_t nqp = (int64_t)p.qtiles * kSilQ;
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

struct SilPlan {
  int64_t chunk_rows, n_chunks, qtiles, off_xn, off_qn, off_rec, bytes;
};

// chunk_rows = 0: the fewest chunks that give kSilTargetBlocks blocks (a fixed figure, so that the workspace
// query needs no device)
bool sil_plan(int64_t n_rows, int32_t nq, int32_t chunk_rows, SilPlan& pl) {
  const int64_t tiles = cdiv(n_rows, kSilTile);
  pl.qtiles = cdiv(nq, kSilQ);
  if (chunk_rows == 0) {
    int64_t want = pl.qtiles > 0 ? cdiv(kSilTargetBlocks, pl.qtiles) : 1;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    pl.chunk_rows = (tiles > 0 ? cdiv(tiles, want) : 1) * kSilTile;
  } else {
    pl.chunk_rows = chunk_rows;
  }
  pl.n_chunks = cdiv(n_rows, pl.chunk_rows);
  const auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
  pl.off_xn = kSilHeader;
  pl.off_qn = pl.off_xn + up(n_rows * 4);
  pl.off_rec = pl.off_qn + up(pl.qtiles * kSilQ * 4);
  pl.bytes = pl.off_rec + pl.n_chunks * pl.qtiles * kSilQ * (int64_t)sizeof(SilRecord);
  return pl.n_chunks * pl.qtiles <= INT32_MAX;
}

int sil_check_shape(const char* who, int64_t n_rows, int32_t nq, int32_t chunk_rows) {
  if (n_rows < 0 || n_rows > INT32_MAX) return fail(RQSID_E_ARG, "%s: n_rows = %lld", who, (long long)n_rows);
  if (nq < 0) return fail(RQSID_E_ARG, "%s: n_queries = %d", who, nq);
  if (chunk_rows < 0 || chunk_rows % kSilTile)
    return fail(RQSID_E_ARG, "%s: chunk_rows = %d (0 or a positive multiple of %d)", who, chunk_rows, kSilTile);
  return RQSID_OK;
}

template <int XF>
int sil_launch(const SilParams& p, hipStream_t st) {
  int rc;
  const unsigned nb = grid_cap(cdiv(p.n_rows, 4), 16384), qb = grid_cap(cdiv(p.nq, 4), 16384);
  hipLaunchKernelGGL((sil_norm_kernel<XF>), dim3(nb), dim3(256), 0, st, p.x, p.n_rows, p.dim, p.xn);
  if ((rc = check_launch("rqsid_silhouette (row norms)"))) return rc;
  hipLaunchKernelGGL((sil_norm_kernel<XF>), dim3(qb), dim3(256), 0, st, p.q, (int64_t)p.nq, p.dim, p.qn);
  if ((rc = check_launch("rqsid_silhouette (query norms)"))) return rc;
  const int64_t items = p.n_seg + 1 > p.nq ? p.n_seg + 1 : p.nq;
  hipLaunchKernelGGL(sil_check_kernel, dim3(grid_cap(cdiv(items, 256), 1024)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_silhouette (tables)"))) return rc;
  hipLaunchKernelGGL((silhouette_kernel<XF>), dim3((unsigned)((int64_t)p.qtiles * p.n_chunks)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_silhouette"))) return rc;
  hipLaunchKernelGGL(sil_fold_kernel, dim3((unsigned)cdiv(p.nq, 256)), dim3(256), 0, st, p);
  return check_launch("rqsid_silhouette (fold)");
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int32_t rqsid_silhouette_tile_rows(void) { return kSilTile; }

int64_t rqsid_silhouette_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t chunk_rows) {
  int rc;
  if ((rc = sil_check_shape("rqsid_silhouette_workspace_bytes", n_rows, n_queries, chunk_rows))) return rc;
  SilPlan pl;
  if (!sil_plan(n_rows, n_queries, chunk_rows, pl))
    return fail(RQSID_E_ARG, "rqsid_silhouette_workspace_bytes: %lld chunks x %lld query tiles exceed 2^31 - 1 blocks",
                (long long)pl.n_chunks, (long long)pl.qtiles);
  return pl.bytes;
}

int rqsid_silhouette(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                     int32_t n_segments, const int32_t* seg_row_off, const void* q, int32_t n_queries,
                     const int32_t* query_self, const int32_t* query_seg, int32_t chunk_rows, float* out_a,
                     float* out_b, int32_t* out_b_seg, float* out_s, void* workspace, int64_t workspace_bytes,
                     void* stream) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "rqsid_silhouette: unknown x_format %d", x_format);
  if (dim <= 0 || dim % kChunk || dim > kMaxDim)
    return fail(RQSID_E_ARG, "rqsid_silhouette: dim = %d (a multiple of %d up to %d)", dim, kChunk, kMaxDim);
  int rc;
  if ((rc = sil_check_shape("rqsid_silhouette", n_rows, n_queries, chunk_rows))) return rc;
  if (n_segments < 0) return fail(RQSID_E_ARG, "rqsid_silhouette: n_segments = %d", n_segments);
  if (n_rows == 0 || n_queries == 0) return RQSID_OK;
  if (n_segments < 1 || !seg_row_off)
    return fail(RQSID_E_ARG, "rqsid_silhouette: n_segments = %d and seg_row_off are required", n_segments);
  if (!x || !q || ((uintptr_t)x & 15) || ((uintptr_t)q & 15))
    return fail(RQSID_E_ARG, "rqsid_silhouette: x and q are required, 16-byte aligned");
  if (!out_a || !out_b || !out_b_seg || !out_s)
    return fail(RQSID_E_ARG, "rqsid_silhouette: out_a, out_b, out_b_seg and out_s are required");
  SilPlan pl;
  if (!sil_plan(n_rows, n_queries, chunk_rows, pl))
    return fail(RQSID_E_ARG, "rqsid_silhouette: %lld chunks x %lld query tiles exceed 2^31 - 1 blocks",
                (long long)pl.n_chunks, (long long)pl.qtiles);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "rqsid_silhouette: workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)pl.bytes);
  char* ws = static_cast<char*>(workspace);
  SilParams p;
  p.x = x;
  p.q = q;
  p.row_index = row_index;
  p.seg_off = seg_row_off;
  p.query_self = query_self;
  p.query_seg = query_seg;
  p.xn = reinterpret_cast<float*>(ws + pl.off_xn);
  p.qn = reinterpret_cast<float*>(ws + pl.off_qn);
  p.rec = reinterpret_cast<SilRecord*>(ws + pl.off_rec);
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.out_a = out_a;
  p.out_b = out_b;
  p.out_b_seg = out_b_seg;
  p.out_s = out_s;
  p.n_rows = n_rows;
  p.chunk_rows = pl.chunk_rows;
  p.dim = dim;
  p.n_seg = n_segments;
  p.nq = n_queries;
  p.qtiles = (int32_t)pl.qtiles;
  p.n_chunks = (int32_t)pl.n_chunks;
  hipStream_t st = (hipStream_t)stream;
  if (x_format == RQSID_X_F32) return sil_launch<RQSID_X_F32>(p, st);
  if (x_format == RQSID_X_F16) return sil_launch<RQSID_X_F16>(p, st);
  return sil_launch<RQSID_X_BF16>(p, st);
}

}  // extern "C"
