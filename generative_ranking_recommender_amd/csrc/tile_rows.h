// tile_rows.h — the row-against-row block that silhouette.hip, row_knn.hip and probe_knn.hip share.
// Not ABI.
//
// A block owns 128 queries and a run of 128-position tiles of the bucketed order (row_index).  Per tile and 32-dim
// chunk it stages fp32 images of the 128 base rows and of its 128 queries in LDS (144-B pitch, 16-bit rows widened
// as they are staged; two image pairs, so a chunk costs one barrier, with the next chunk's global loads in flight
// during the MFMAs) and runs v_mfma_f32_32x32x2_f32 with the base rows on the A side and the queries on the B side:
// lane (r, h) of wave w then holds query 32 w + r against 64 base rows.  A caller's policy turns each dot product
// into the float that is parked in the (now idle) operand images, and 128 threads, one per query, then walk the
// tile's 128 positions in order.  Here once: the geometry, the guards of the caller's tables and the kernel that
// reports them, the norm kernel, the 64-MFMA chunk step, the block itself
// (row_tile_sweep), and the host side that both entries share (RowPairPlan, the row_pair_check_* refusals, row_pair_fill, row_pair_prepare).
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdio>

#include "assign_common.h"
#include "exact_row.h"

namespace rqsid {

constexpr int kRowTile = 128;      // base positions per tile (4 MFMA blocks of 32)
constexpr int kRowQ = 128;         // queries per block (32 per wave)
constexpr int kRowStride = 36;     // floats per row of a chunk image: 32 + 4 of padding (16-B reads, no bank conflict)
constexpr int kRowOp = kRowTile * kRowStride;  // floats per operand image
constexpr int kRowDStride = 132;   // floats per position of the parked values (128 queries + 4)
constexpr int kRowHeader = 256;    // workspace [0, 4): sticky error word; the rest of the header is the entry's own
constexpr int kRowTargetBlocks = 2048;  // chunk_rows = 0: at least this many blocks (8 per CU of an MI355X)
constexpr uint32_t kRowErrRow = 1u;  // a row_index / query_self entry outside [0, n_rows)
constexpr uint32_t kRowErrSeg = 2u;  // a query_seg entry outside [-1, n_segments)
constexpr uint32_t kRowErrOff = 4u;  // a seg_row_off entry outside [0, n_rows] or decreasing
static_assert(4 * kRowOp >= kRowTile * kRowDStride, "the parked values fit in the operand images");

// what both kernels' blocks are given; SilParams and KnnParams add their own areas and outputs
struct RowPairParams {
  const void* x;
  const void* q;
  const int32_t* row_index;
  const int32_t* seg_off;     // null: no segments (n_seg = 0)
  const int32_t* query_self;
  const int32_t* query_seg;
  const int32_t* q_row;       // null: column c of the blocks is row c of q; else row q_row[c], -1: none (the
                              // caller's own table, [qtiles * kRowQ], with every entry inside [-1, nq))
  float* xn;      // [n_rows] the row's norm term, by row (NormRule)
  float* qn;      // [qtiles * kRowQ] likewise
  uint32_t* err;  // the header: the sticky error word, then the entry's counters
  int64_t n_rows;
  int64_t chunk_rows;
  int32_t dim, n_seg, nq, qtiles, n_chunks;
};

// a segment offset as the kernels use it: inside [0, n_rows] whatever the table holds
__device__ __forceinline__ int64_t off_at(const RowPairParams& p, int s) {
  const int64_t v = p.seg_off[s];
  return v < 0 ? 0 : (v > p.n_rows ? p.n_rows : v);
}
__device__ __forceinline__ int clean_seg(const RowPairParams& p, int i) {
  const int v = p.query_seg ? p.query_seg[i] : -1;
  return (unsigned)v < (unsigned)p.n_seg ? v : -1;
}
__device__ __forceinline__ int clean_self(const RowPairParams& p, int i) {
  const int v = p.query_self ? p.query_self[i] : -1;
  return (int64_t)(uint32_t)v < p.n_rows ? v : -1;
}

// the sticky error bits of the tables the kernels clamp instead of follow; the first COUNTERS threads zero the
// header's counter words of the call
template <int COUNTERS>
__global__ __launch_bounds__(256) void row_pair_check_kernel(RowPairParams p) {
  uint32_t errs = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 < COUNTERS) p.err[1 + i0] = 0u;
  if (p.seg_off)
    for (int64_t i = i0; i <= p.n_seg; i += stride) {
      const int64_t v = p.seg_off[i];
      if (v < 0 || v > p.n_rows || (i > 0 && v < (int64_t)p.seg_off[i - 1])) errs |= kRowErrOff;
    }
  if (p.row_index)
    for (int64_t i = i0; i < p.n_rows; i += stride)
      if ((int64_t)(uint32_t)p.row_index[i] >= p.n_rows) errs |= kRowErrRow;
  for (int64_t i = i0; i < p.nq; i += stride) {
    if (p.query_self) {
      const int v = p.query_self[i];
      if (v != -1 && (int64_t)(uint32_t)v >= p.n_rows) errs |= kRowErrRow;
    }
    if (p.query_seg) {
      const int v = p.query_seg[i];
      if (v != -1 && (unsigned)v >= (unsigned)p.n_seg) errs |= kRowErrSeg;
    }
  }
  if (errs) atomicOr(p.err, errs);
}

// What the norm kernel stores for a row with s = the fp64 sum of its squares:
//   kNormSq       fl32(s)                                                                   (the silhouette)
//   kNormSqFinite fl32(s); -1 for a row with a non-finite element: it has no key            (k-NN, L2)
//   kNormInv      fl32(1 / sqrt(s)); NaN outside the range the screen's interval is proven for, 2^-30 <= |x| <=
//                 2^30, which sends the pair to the exact pass; -1 for a zero or non-finite row  (k-NN, cosine)
enum NormRule { kNormSq, kNormSqFinite, kNormInv };

// one wave per row, lanes over 16-B pieces (c_meta's |c|^2 rule)
template <int XF, int RULE>
__global__ __launch_bounds__(256) void row_norm_kernel(const void* __restrict__ src, int64_t n, int dim,
                                                       float* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = dim / 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < n; row += (int64_t)gridDim.x * 4) {
    double s = 0.0;
    bool nf = false;
    for (int i = lane; i < nv; i += 64) {
      const float4 a = load_row4<XF>(static_cast<const float*>(src), row, dim, i);
      s += sq4(a);
      if constexpr (RULE != kNormSq)
        nf |= !(fabsf(a.x) <= FLT_MAX) | !(fabsf(a.y) <= FLT_MAX) | !(fabsf(a.z) <= FLT_MAX) | !(fabsf(a.w) <= FLT_MAX);
    }
    s = wave_sum(s);
    float v = (float)s;
    if constexpr (RULE != kNormSq) nf = __any(nf);
    if constexpr (RULE == kNormInv) {
      v = (s >= 0x1p-60 && s <= 0x1p60) ? (float)(1.0 / sqrt(s)) : __uint_as_float(0x7FC00000u);
      nf |= s == 0.0;
    }
    if (lane == 0) out[row] = nf ? -1.0f : v;
  }
}

template <int XF>
__device__ __forceinline__ uint4 load_raw(const void* base, int64_t row, int dim, int i4) {
  if constexpr (XF == RQSID_X_F32) {
    return reinterpret_cast<const uint4*>(static_cast<const float*>(base) + row * dim)[i4];
  } else {
    const uint2 w = reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(base) + row * dim)[i4];
    return make_uint4(w.x, w.y, 0u, 0u);
  }
}
template <int XF>
__device__ __forceinline__ float4 widen_raw(uint4 w) {
  float4 a;
  if constexpr (XF == RQSID_X_F32) {
    a = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
  } else if constexpr (XF == RQSID_X_F16) {
    // v_cvt_f32_f16: exact for every binary16 value, subnormals, infinities and NaNs included (these kernels run
    // in the default MODE, which keeps fp16 subnormals), so the image equals the widened fp32 row bit for bit
    const __half2 lo = *reinterpret_cast<const __half2*>(&w.x), hi = *reinterpret_cast<const __half2*>(&w.y);
    a = make_float4(__low2float(lo), __high2float(lo), __low2float(hi), __high2float(hi));
  } else {
    widen2<XF, true>(w.x, a.x, a.y);
    widen2<XF, true>(w.y, a.z, a.w);
  }
  return a;
}

// The 64 MFMAs of one 32-dim chunk: 4 quarter-chunks x 4 blocks of 32 A rows x 4 k-steps, on a pair of images of
// kRowStride floats per row.  sq holds the B side (lane (r, h) reads row qcol), sx the A side (rows 32 b + r).
// Afterwards lane (r, h) holds, for B row qcol, A rows 32 b + 8 g + 4 h + k in acc[b][4 g + k].
__device__ __forceinline__ void mfma_chunk_step(const float* sq, const float* sx, int qcol, int r, int h,
                                                f32x16 (&acc)[4]) {
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    // lane half h takes dims 8 qd + 4 h .. + 3 of the chunk for its four k-steps (A and B alike)
    const float4 bv = *reinterpret_cast<const float4*>(sq + qcol * kRowStride + 8 * qd + 4 * h);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const float4 av = *reinterpret_cast<const float4*>(sx + (32 * b + r) * kRowStride + 8 * qd + 4 * h);
      acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[b], 0, 0, 0);
      acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[b], 0, 0, 0);
      acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[b], 0, 0, 0);
      acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[b], 0, 0, 0);
    }
  }
}

// The block's LDS.  Three arrays and not one struct: as distinct objects the compiler knows that the parked values
// (s_buf) do not overlap s_row / s_xn, which one object with a run-time index into it would hide (30 VGPRs more).
struct RowTileLds {
  float* s_buf;  // two (query, base) image pairs / the parked values
  int* s_row;    // the tile's row numbers, -1: none
  float* s_xn;   // and norm terms
};
__device__ __forceinline__ RowTileLds row_tile_lds() {
  __shared__ __attribute__((aligned(16))) float s_buf[4 * kRowOp];
  __shared__ __attribute__((aligned(16))) int s_row[kRowTile];
  __shared__ __attribute__((aligned(16))) float s_xn[kRowTile];
  return {s_buf, s_row, s_xn};
}

// Tiles [tile0, tile1) of the chunk [c0, c1) of positions against the block's 128 queries, columns q0 .. q0 + 127
// (rows of q, or through RowPairParams::q_row).  The policy supplies what the callers differ in, as inlined hooks:
//   tile_row(t, row, xn)          thread t < 128, before the tile's MFMAs: the row number (-1: none) and norm term
//                                 of position t of the tile, which it may change;
//   value(pos0, j, dot, xn, row)  the float that is parked for the lane's query against position j of the tile;
//   walk(pos0, s_d, s_row)        thread t < 128, after the park: query t's values are s_d[j * kRowDStride + t].
template <int XF, class Policy>
__device__ __forceinline__ void row_tile_sweep(const RowPairParams& p, int q0, int64_t c0, int64_t c1, int tile0,
                                               int tile1, const RowTileLds& lds, Policy& policy) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nch = p.dim / kChunk;
  float* const s_buf = lds.s_buf;

  // staging role: thread t moves 16 B (f4 = t & 7) of base rows / queries (t >> 3) + 32 i of every chunk
  const int f4 = t & 7, srow = t >> 3;
  int my_q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = q0 + srow + 32 * i;
    my_q[i] = p.q_row ? p.q_row[c] : (c < p.nq ? c : -1);
  }
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

  int rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows[i] = -1;
  if (tile0 < tile1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = row_at(c0 + (int64_t)tile0 * kRowTile + srow + 32 * i);
    load_chunk(rows[0], rows[1], rows[2], rows[3], 0);
  }

  for (int tile = tile0; tile < tile1; ++tile) {
    const int64_t pos0 = c0 + (int64_t)tile * kRowTile;
    // this tile's row numbers and norm terms for the epilogue, and the next tile's rows for the staging role
    int e_row = -1;
    float e_xn = 0.f;
    if (t < kRowTile) {
      e_row = row_at(pos0 + t);
      e_xn = e_row >= 0 ? p.xn[e_row] : 0.f;
      policy.tile_row(t, e_row, e_xn);
    }
    int nrows[4] = {-1, -1, -1, -1};
    if (tile + 1 < tile1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) nrows[i] = row_at(pos0 + kRowTile + srow + 32 * i);
    }

    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;

    for (int ch = 0; ch < nch; ++ch) {
      float* const sq = s_buf + (ch & 1) * 2 * kRowOp;
      float* const sx = sq + kRowOp;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(sx + (srow + 32 * i) * kRowStride + 4 * f4) = widen_raw<XF>(xr[i]);
        *reinterpret_cast<float4*>(sq + (srow + 32 * i) * kRowStride + 4 * f4) = widen_raw<XF>(qr[i]);
      }
      // one barrier per chunk: the pair written here was last read two chunks ago, before the previous barrier
      __syncthreads();
      {  // the next chunk's loads (the next tile's first chunk after the last), in flight during the MFMAs
        const bool last = ch + 1 == nch;
        if (!last || tile + 1 < tile1)
          load_chunk(last ? nrows[0] : rows[0], last ? nrows[1] : rows[1], last ? nrows[2] : rows[2],
                     last ? nrows[3] : rows[3], last ? 0 : ch + 1);
      }
      mfma_chunk_step(sq, sx, qcol, r, h, acc);
    }

    // ---- epilogue: the tile's values into the idle operand images ----
    if (t < kRowTile) {
      lds.s_row[t] = e_row;
      lds.s_xn[t] = e_xn;
    }
    __syncthreads();  // every wave has finished the tile's MFMAs; s_row / s_xn are visible
    float* const s_d = s_buf;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        // mfma_chunk_step's map: lane (r, h) holds base positions 32 b + 8 g + 4 h + k of the tile in acc[b][4 g + k]
        const int P = 32 * b + 8 * g + 4 * h;
        const float4 xn4 = *reinterpret_cast<const float4*>(lds.s_xn + P);
        const int4 rw4 = *reinterpret_cast<const int4*>(lds.s_row + P);
        s_d[(P + 0) * kRowDStride + qcol] = policy.value(pos0, P + 0, acc[b][4 * g + 0], xn4.x, rw4.x);
        s_d[(P + 1) * kRowDStride + qcol] = policy.value(pos0, P + 1, acc[b][4 * g + 1], xn4.y, rw4.y);
        s_d[(P + 2) * kRowDStride + qcol] = policy.value(pos0, P + 2, acc[b][4 * g + 2], xn4.z, rw4.z);
        s_d[(P + 3) * kRowDStride + qcol] = policy.value(pos0, P + 3, acc[b][4 * g + 3], xn4.w, rw4.w);
      }
    __syncthreads();
    if (t < kRowQ) policy.walk(pos0, s_d, lds.s_row);
    __syncthreads();  // the values are read before the next tile's images overwrite them
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = nrows[i];
  }
}

// ---- host side ----

struct RowPairPlan {
  int64_t chunk_rows, n_chunks, qtiles;
  int64_t off_xn, off_qn, off_own;  // workspace: the header, |x| terms, |q| terms, then the entry's own areas
};
inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

// chunk_rows = 0: the fewest chunks that give kRowTargetBlocks blocks (a fixed figure, so that the workspace
// query needs no device).  false: more than 2^31 - 1 blocks
inline bool row_pair_plan(int64_t n_rows, int32_t nq, int32_t chunk_rows, RowPairPlan& pl) {
  const int64_t tiles = cdiv(n_rows, kRowTile);
  pl.qtiles = cdiv(nq, kRowQ);
  if (chunk_rows == 0) {
    int64_t want = pl.qtiles > 0 ? cdiv(kRowTargetBlocks, pl.qtiles) : 1;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    pl.chunk_rows = (tiles > 0 ? cdiv(tiles, want) : 1) * kRowTile;
  } else {
    pl.chunk_rows = chunk_rows;
  }
  pl.n_chunks = cdiv(n_rows, pl.chunk_rows);
  pl.off_xn = kRowHeader;
  pl.off_qn = pl.off_xn + up256(n_rows * 4);
  pl.off_own = pl.off_qn + up256(pl.qtiles * kRowQ * 4);
  return pl.n_chunks * pl.qtiles <= INT32_MAX;
}
inline int row_pair_fail_blocks(const char* who, const RowPairPlan& pl) {
  return fail(RQSID_E_ARG, "%s: %lld chunks x %lld query tiles exceed 2^31 - 1 blocks", who, (long long)pl.n_chunks,
              (long long)pl.qtiles);
}

// The refusals both entries share, one helper per group: an entry calls them in the order it has always made its
// refusals, with its own (metric, k, its rule for the segment tables, its outputs) in between.
inline int row_pair_check_format(const char* who, int32_t x_format, int32_t dim) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "%s: unknown x_format %d", who, x_format);
  if (dim <= 0 || dim % kChunk || dim > kMaxDim)
    return fail(RQSID_E_ARG, "%s: dim = %d (a multiple of %d up to %d)", who, dim, kChunk, kMaxDim);
  return RQSID_OK;
}
inline int row_pair_check_counts(const char* who, int64_t n_rows, int32_t nq) {
  if (n_rows < 0 || n_rows > INT32_MAX) return fail(RQSID_E_ARG, "%s: n_rows = %lld", who, (long long)n_rows);
  if (nq < 0) return fail(RQSID_E_ARG, "%s: n_queries = %d", who, nq);
  return RQSID_OK;
}
inline int row_pair_check_chunks(const char* who, int32_t chunk_rows, int32_t n_seg = 0) {  // (the size queries: no n_seg)
  if (chunk_rows < 0 || chunk_rows % kRowTile)
    return fail(RQSID_E_ARG, "%s: chunk_rows = %d (0 or a positive multiple of %d)", who, chunk_rows, kRowTile);
  if (n_seg < 0) return fail(RQSID_E_ARG, "%s: n_segments = %d", who, n_seg);
  return RQSID_OK;
}
inline int row_pair_check_rows(const char* who, const void* x, const void* q) {
  if (!x || !q || ((uintptr_t)x & 15) || ((uintptr_t)q & 15))
    return fail(RQSID_E_ARG, "%s: x and q are required, 16-byte aligned", who);
  return RQSID_OK;
}

// the base part of a kernel's parameters from the entry's arguments and the plan
inline void row_pair_fill(RowPairParams& p, const void* x, int64_t n_rows, int32_t dim, const int32_t* row_index,
                          int32_t n_seg, const int32_t* seg_off, const void* q, int32_t nq, const int32_t* query_self,
                          const int32_t* query_seg, void* workspace, const RowPairPlan& pl) {
  char* ws = static_cast<char*>(workspace);
  p.x = x;
  p.q = q;
  p.row_index = row_index;
  p.seg_off = seg_off;
  p.query_self = query_self;
  p.query_seg = query_seg;
  p.q_row = nullptr;
  p.xn = reinterpret_cast<float*>(ws + pl.off_xn);
  p.qn = reinterpret_cast<float*>(ws + pl.off_qn);
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.n_rows = n_rows;
  p.chunk_rows = pl.chunk_rows;
  p.dim = dim;
  p.n_seg = n_seg;
  p.nq = nq;
  p.qtiles = (int32_t)pl.qtiles;
  p.n_chunks = (int32_t)pl.n_chunks;
}

// the kernels both entries run first: the norm terms of the rows and the queries, then the table check
template <int XF, int RULE, int COUNTERS>
int row_pair_prepare(const char* who, const RowPairParams& p, hipStream_t st) {
  const auto launched = [&](const char* step) {
    char what[96];
    snprintf(what, sizeof what, "%s (%s)", who, step);
    return check_launch(what);
  };
  int rc;
  const unsigned nb = grid_cap(cdiv(p.n_rows, 4), 16384), qb = grid_cap(cdiv(p.nq, 4), 16384);
  hipLaunchKernelGGL((row_norm_kernel<XF, RULE>), dim3(nb), dim3(256), 0, st, p.x, p.n_rows, p.dim, p.xn);
  if ((rc = launched("row norms"))) return rc;
  hipLaunchKernelGGL((row_norm_kernel<XF, RULE>), dim3(qb), dim3(256), 0, st, p.q, (int64_t)p.nq, p.dim, p.qn);
  if ((rc = launched("query norms"))) return rc;
  int64_t items = p.n_seg + 1 > p.nq ? p.n_seg + 1 : p.nq;
  if (p.row_index && p.n_rows > items) items = p.n_rows;
  hipLaunchKernelGGL(row_pair_check_kernel<COUNTERS>, dim3(grid_cap(cdiv(items, 256), 1024)), dim3(256), 0, st, p);
  return launched("tables");
}

}  // namespace rqsid
