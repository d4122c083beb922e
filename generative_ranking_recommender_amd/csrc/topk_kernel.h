// topk_kernel.h — the screen / exact-pass kernel behind rqsid_assign_topk (assign_topk.hip) and rqsid_beam_expand
// (beam.hip), and the host entry both share (include/rqsid.h; bound, list capacity and counters: DESIGN.md §3.1g,
// the item layout: §3.1h).  ITEMS = false ranks rows; ITEMS = true ranks n_items = n_rows * beam items, item i reading
// row i / beam of x (the only place the instantiations differ besides den_out at res_levels 2).
//
// One block (4 waves) per 128-row tile of one segment, three phases:
//   0  (normalised residual levels only) the row's divisor den = fl32(sqrt(fp64 sum a_i^2)) + 1e-8f, lanes over
//      dims as the exact re-score of assign.hip does it; at res_levels 1 (items: 1 and 2) it goes to den_out;
//   1  screen: t_j = |c_j|^2 - 2 v.c_j for every allowed centre, the dot products on v_mfma_f32_32x32x2_f32 from
//      fp32 LDS images of one 32-dim chunk of the tile's rows (built with the re-score's fp32 operation sequence,
//      16-bit rows widened as they load) and of 128 centres; each value carries the interval [t - e, t + e] of
//      §3.1g, a row keeps the candidates whose lower end does not exceed the k-th smallest upper end (a list of
//      KK + 2 entries per lane half in LDS, compacted against the current threshold when it fills);
//   2  exact: one wave per row, lanes over dims, fp64 sum (v_i - c_i)^2 of every listed candidate (of every allowed
//      candidate for a row whose list overflowed or whose screen saw a non-finite value), ranked by (d2, position).
// No list lives outside the block, so no write takes its position from a device counter; the sticky error word
// records clamped tile counts and row / centre indices found outside their tables.
#pragma once
#include <cfloat>

#include "assign_common.h"

namespace rqsid {
namespace {

constexpr int kTkGroup = 128;   // candidates per screen group (4 MFMA blocks of 32)
constexpr int kTkStride = 36;   // floats per row of a chunk image: 32 + 4 of padding (16-B reads, no bank conflict)
constexpr int kTkSlots = 8;     // lanes holding the running top-k of the exact pass (= RQSID_TOPK_MAX)
constexpr int kTkRound = 64 - kTkSlots;  // new candidates per ranking round
constexpr int kTkBatch = 8;             // candidates per fp64 batch of the exact pass
constexpr int kTkHeaderBytes = 256;
constexpr int kErrTkTiles = 1;  // device tile count past max_tiles (clamped)
constexpr int kErrTkRow = 2;    // a row position or row index outside [0, n_rows) (skipped)
constexpr int kErrTkCand = 4;   // a candidate's centre row outside [0, n_centers) (centre row 0 read instead)
static_assert(kTkSlots == RQSID_TOPK_MAX && kTileRows == 128, "rqsid.h / tile constants");

struct TopkParams {
  const void* x;
  int32_t xf;
  int64_t n_rows;  // rows; with ITEMS the items (outputs, den_in / den_out and row_index count items)
  int32_t beam;    // ITEMS: items per row of x
  int32_t dim;
  const int32_t* row_index;
  int32_t n_segments;
  const int32_t* seg_row_off;
  const int32_t* seg_tile_off;
  int64_t max_tiles;
  const float* centers;
  const float4* c_meta;
  int32_t n_centers;
  const int32_t* cand_base;
  const int32_t* cand_count;
  const int32_t* cand_idx;
  const int32_t* cand_lid;
  const uint8_t* seg_flags;
  int32_t rl;
  int32_t norm;
  const float* ca;
  const int32_t* seg_ca;
  const float* cb;
  const int32_t* seg_cb;
  const float* den_in;
  float* den_out;
  int32_t k;
  int32_t* out_local;
  int32_t* out_global;
  float* out_dist;
  int32_t* ws;     // [0] sticky error word, [1] rows re-scored from their list, [2] all-candidate rows, [3] non-finite
  float bound_dot;  // (2 dim + 6) 2^-24 1.01: the |v||c| coefficient of the interval
  float bound_c2;   // 3 2^-24 1.01: the |c|^2 coefficient
};

// 16 B of a row as they lie in memory (fp32: elements 4i..4i+3; 16-bit: the same four in .x, .y) and their fp32
// values; split so that the loads can be issued a chunk ahead of the arithmetic
__device__ __forceinline__ uint4 load_x_raw(const TopkParams& p, int64_t row, int i) {
  if (p.xf == RQSID_X_F32) return reinterpret_cast<const uint4*>(static_cast<const float*>(p.x) + row * p.dim)[i];
  const uint2 w = reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(p.x) + row * p.dim)[i];
  return make_uint4(w.x, w.y, 0u, 0u);
}
__device__ __forceinline__ float4 widen_raw(const TopkParams& p, uint4 w) {
  float4 a;
  if (p.xf == RQSID_X_F32) {
    a = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z), __uint_as_float(w.w));
  } else if (p.xf == RQSID_X_F16) {
    widen2<RQSID_X_F16, true>(w.x, a.x, a.y);
    widen2<RQSID_X_F16, true>(w.y, a.z, a.w);
  } else {
    widen2<RQSID_X_BF16, true>(w.x, a.x, a.y);
    widen2<RQSID_X_BF16, true>(w.y, a.z, a.w);
  }
  return a;
}
// the residual chain up to (not including) the level's own normalisation: the re-score's fp32 sequence
__device__ __forceinline__ float4 chain(const TopkParams& p, float4 a, float4 ca, float4 cb, float din) {
  if (p.rl >= 1) a = make_float4(a.x - ca.x, a.y - ca.y, a.z - ca.z, a.w - ca.w);
  if (p.rl >= 2) {
    if (p.norm) a = make_float4(a.x / din, a.y / din, a.z / din, a.w / din);
    a = make_float4(a.x - cb.x, a.y - cb.y, a.z - cb.z, a.w - cb.w);
  }
  return a;
}
__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }

// the row of x behind output index `row` (rows: itself; items: row / beam, the only division of the kernel)
template <bool ITEMS>
__device__ __forceinline__ int x_row(const TopkParams& p, int row) {
  if constexpr (ITEMS) return row < 0 ? -1 : row / p.beam;
  else return row;
}

__device__ __forceinline__ int topk_cand_global(const TopkParams& p, int base, int pos) {
  int g = p.cand_idx ? p.cand_idx[base + pos] : base + pos;
  if ((uint32_t)g >= (uint32_t)p.n_centers) {
    atomicOr(p.ws, kErrTkCand);
    g = 0;
  }
  return g;
}

// ascending insertion of x into the sorted t[0..N)
template <int N>
__device__ __forceinline__ void insert_sorted(float (&t)[N], float x) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float lo = fminf(t[i], x);
    x = fmaxf(t[i], x);
    t[i] = lo;
  }
}

// a whole row as it lies in memory, lanes over dims (lane l: 16 B pieces l, l + 64, ...), and its level-1 divisor;
// loaded ahead of its use (the next row's while this row is ranked) so that the rows of a wave do not pay the
// memory latency one after another.  row < 0: nothing is read.
struct RowRaw {
  uint4 w[kMaxDim / 256];
  float din;
};
__device__ __forceinline__ void load_row_raw(const TopkParams& p, int row, int xrow, int lane, int nv4, RowRaw& o) {
  o.din = (p.rl >= 2 && p.norm && row >= 0) ? p.den_in[row] : 1.0f;
#pragma unroll
  for (int m = 0; m < kMaxDim / 256; ++m) {
    const int i = lane + 64 * m;
    o.w[m] = (row >= 0 && i < nv4) ? load_x_raw(p, xrow, i) : make_uint4(0u, 0u, 0u, 0u);
  }
}

// the segment's residual centre rows, lanes over dims (NULL: zeros)
__device__ __forceinline__ void load_seg_rows(const float* car, const float* cbr, int lane, int nv4,
                                              float4 (&ca4)[kMaxDim / 256], float4 (&cb4)[kMaxDim / 256]) {
#pragma unroll
  for (int m = 0; m < kMaxDim / 256; ++m) {
    const int i = lane + 64 * m;
    ca4[m] = (car && i < nv4) ? reinterpret_cast<const float4*>(car)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    cb4[m] = (cbr && i < nv4) ? reinterpret_cast<const float4*>(cbr)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// the staging role's loads of chunk ch: 16 B of four rows and of four centres, and of the residual centres
__device__ __forceinline__ void load_chunk(const TopkParams& p, int ch, int f4, const int (&my_row)[4],
                                           const int (&my_cg)[4], const float* car, const float* cbr, uint4 (&xr)[4],
                                           float4 (&cr)[4], float4& car4, float4& cbr4) {
  const int i4 = ch * (kChunk / 4) + f4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    xr[i] = my_row[i] >= 0 ? load_x_raw(p, my_row[i], i4) : make_uint4(0u, 0u, 0u, 0u);
    cr[i] = my_cg[i] >= 0 ? reinterpret_cast<const float4*>(p.centers + (int64_t)my_cg[i] * p.dim)[i4]
                          : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (p.rl >= 1) car4 = reinterpret_cast<const float4*>(car)[i4];
  if (p.rl >= 2) cbr4 = reinterpret_cast<const float4*>(cbr)[i4];
}

template <int KK, bool ITEMS>
__global__ __launch_bounds__(256, 2) void assign_topk_kernel(TopkParams p) {
  constexpr int CAPH = KK + 2;  // list entries per lane half of a row
  __shared__ __attribute__((aligned(16))) float s_v[kTileRows * kTkStride];
  __shared__ __attribute__((aligned(16))) float s_c[kTkGroup * kTkStride];
  __shared__ int s_row[kTileRows];
  __shared__ int s_cg[kTkGroup];
  __shared__ float2 s_cm[kTkGroup];
  __shared__ float s_den[kTileRows];
  __shared__ float s_u[kTileRows];
  __shared__ int s_cnt[2 * kTileRows];
  __shared__ int2 s_list[2 * kTileRows * CAPH];
  __shared__ int s_scr[kWaves][64];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  // tile -> segment; a device tile count past the launch's capacity is clamped
  const int64_t ntiles_raw = p.seg_tile_off[p.n_segments];
  if (ntiles_raw > p.max_tiles && blockIdx.x == 0 && t == 0) atomicOr(p.ws, kErrTkTiles);
  const int64_t ntiles = ntiles_raw < p.max_tiles ? ntiles_raw : p.max_tiles;
  const int64_t tile = blockIdx.x;
  if (tile >= ntiles) return;
  int s = 0;
  {
    int lo = 0, hi = p.n_segments;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (p.seg_tile_off[mid] <= tile) lo = mid;
      else hi = mid;
    }
    s = lo;
  }
  const int64_t r0 = (int64_t)p.seg_row_off[s] + (tile - p.seg_tile_off[s]) * kTileRows;
  const int64_t left = (int64_t)p.seg_row_off[s + 1] - r0;
  const int nr = left < 0 ? 0 : (left > kTileRows ? kTileRows : (int)left);
  if (t < kTileRows) {
    int row = -1;
    if (t < nr) {
      const int64_t pos = r0 + t;
      if (pos >= 0 && pos < p.n_rows) {
        row = p.row_index ? p.row_index[pos] : (int)pos;
        if ((int64_t)(uint32_t)row >= p.n_rows) row = -1;
      }
      if (row < 0) atomicOr(p.ws, kErrTkRow);
    }
    s_row[t] = row;
    s_den[t] = 1.0f;
  }
  const bool penalty = p.seg_flags && (p.seg_flags[s] & RQSID_SEG_PENALTY);
  const int base = p.cand_base[s];
  const int count = penalty ? 0 : max(p.cand_count[s], 0);
  const bool normed = p.norm && p.rl >= 1;
  const float* car = p.rl >= 1 ? p.ca + (int64_t)seg_row(p.seg_ca, s) * p.dim : nullptr;
  const float* cbr = p.rl >= 2 ? p.cb + (int64_t)seg_row(p.seg_cb, s) * p.dim : nullptr;
  const int nv4 = p.dim / 4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();

  // ---- phase 0: the level's divisor (four rows' loads in flight at a time) ----
  if (normed && !penalty) {
    float4 ca4[kMaxDim / 256], cb4[kMaxDim / 256];
    load_seg_rows(car, cbr, lane, nv4, ca4, cb4);
    for (int rr0 = 0; rr0 < kRowsPerWave; rr0 += 4) {
      RowRaw raw[4];
      int rows[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        rows[u] = s_row[wv * kRowsPerWave + rr0 + u];
        load_row_raw(p, rows[u], x_row<ITEMS>(p, rows[u]), lane, nv4, raw[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (rows[u] < 0) continue;
        double ss = 0.0;
#pragma unroll
        for (int m = 0; m < kMaxDim / 256; ++m) {
          if (lane + 64 * m < nv4) {
            const float4 a = chain(p, widen_raw(p, raw[u].w[m]), ca4[m], cb4[m], raw[u].din);
            ss += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
          }
        }
        const float den = (float)sqrt(wave_sum(ss)) + 1e-8f;
        if (lane == 0) {
          s_den[wv * kRowsPerWave + rr0 + u] = den;
          if ((ITEMS || p.rl == 1) && p.den_out) p.den_out[rows[u]] = den;
        }
      }
    }
    __syncthreads();
  }

  // ---- phase 1: screen ----
  const int rowt = wv * kRowsPerWave + r;  // the tile row of this lane's MFMA column
  float tk[KK];
#pragma unroll
  for (int i = 0; i < KK; ++i) tk[i] = INFINITY;
  float U = INFINITY;
  int cnt = 0;
  bool ovf = false;
  float nv2 = 0.f, vn = 0.f;
  int2* const mylist = s_list + (h * kTileRows + rowt) * CAPH;
  // staging role: thread t moves 16 B (f4 = t & 7) of rows / candidates (t >> 3) + 32 i of every chunk
  const int f4 = t & 7, srow = t >> 3;
  int my_row[4];
  float my_din[4], my_den[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    my_row[i] = x_row<ITEMS>(p, s_row[srow + 32 * i]);  // (the row of x: what the chunk loads address)
    my_din[i] = (p.rl >= 2 && p.norm && my_row[i] >= 0) ? p.den_in[s_row[srow + 32 * i]] : 1.0f;
    my_den[i] = s_den[srow + 32 * i];
  }
  const int nch = p.dim / kChunk;
  for (int g0 = 0; g0 < count; g0 += kTkGroup) {
    __syncthreads();  // the previous group's epilogue has read s_cm
    if (t < kTkGroup) {
      const int pos = g0 + t;
      int g = -1;
      float2 cm = make_float2(0.f, 0.f);
      if (pos < count) {
        g = topk_cand_global(p, base, pos);
        const float4 m = p.c_meta[g];
        cm = make_float2(m.x, m.y);
      }
      s_cg[t] = g;
      s_cm[t] = cm;
    }
    __syncthreads();
    int my_cg[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) my_cg[i] = s_cg[srow + 32 * i];
    f32x16 acc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[b][e] = 0.f;
    uint4 xr[4];
    float4 cr[4], car4 = z4, cbr4 = z4;
    load_chunk(p, 0, f4, my_row, my_cg, car, cbr, xr, cr, car4, cbr4);
    for (int ch = 0; ch < nch; ++ch) {
      __syncthreads();  // every wave has finished the MFMAs of the previous chunk
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float4 a = chain(p, widen_raw(p, xr[i]), car4, cbr4, my_din[i]);
        if (normed) a = div4(a, my_den[i]);
        if (my_row[i] < 0) a = z4;
        *reinterpret_cast<float4*>(s_v + (srow + 32 * i) * kTkStride + 4 * f4) = a;
        *reinterpret_cast<float4*>(s_c + (srow + 32 * i) * kTkStride + 4 * f4) = cr[i];
      }
      __syncthreads();
      if (ch + 1 < nch) load_chunk(p, ch + 1, f4, my_row, my_cg, car, cbr, xr, cr, car4, cbr4);  // in flight during the MFMAs
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // lane half h takes dims 8 q + 4 h .. + 3 of the chunk for its four k-steps (A and B alike)
        const float4 bv = *reinterpret_cast<const float4*>(s_v + rowt * kTkStride + 8 * q + 4 * h);
        if (g0 == 0) nv2 = fmaf(bv.x, bv.x, fmaf(bv.y, bv.y, fmaf(bv.z, bv.z, fmaf(bv.w, bv.w, nv2))));
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float4 av = *reinterpret_cast<const float4*>(s_c + (32 * b + r) * kTkStride + 8 * q + 4 * h);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc[b], 0, 0, 0);
        }
      }
    }
    // epilogue of the group: lane (r, h) holds row r's values of candidates 32 b + (e & 3) + 8 (e >> 2) + 4 h
    if (g0 == 0) {
      const float n2 = nv2 + xor32(nv2);
      vn = sqrtf(n2) * 1.0001f;  // >= |v|: the fp32 sum of squares is within (dim + 2) 2^-24 of exact
      ovf = ovf || !(n2 <= FLT_MAX);
    }
    const float kd = p.bound_dot * vn;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int jc = 32 * b + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float2 cm = s_cm[jc];
        const bool valid = g0 + jc < count;
        const float sv = fmaf(-2.0f, acc[b][e], cm.x);
        const float ev = fmaf(kd, cm.y, fmaf(p.bound_c2, cm.x, 1e-36f));
        ovf = ovf || (valid && !(fabsf(sv) <= FLT_MAX && ev <= FLT_MAX));
        insert_sorted(tk, valid ? sv + ev : INFINITY);
        acc[b][e] = valid ? sv - ev : INFINITY;
      }
    {  // the row's k-th smallest upper end over both lane halves
      float m[KK];
#pragma unroll
      for (int i = 0; i < KK; ++i) m[i] = tk[i];
#pragma unroll
      for (int i = 0; i < KK; ++i) insert_sorted(m, xor32(tk[i]));
#pragma unroll
      for (int i = 0; i < KK; ++i) U = (i == p.k - 1) ? m[i] : U;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int jc = 32 * b + (e & 3) + 8 * (e >> 2) + 4 * h;
        const float lb = acc[b][e];
        if (g0 + jc < count && lb <= U) {
          if (cnt == CAPH) {  // full: drop what the current threshold already excludes
            int keep = 0;
            for (int i = 0; i < CAPH; ++i) {
              const int2 en = mylist[i];
              if (__int_as_float(en.y) <= U) mylist[keep++] = en;
            }
            cnt = keep;
          }
          if (cnt < CAPH) mylist[cnt++] = make_int2(g0 + jc, __float_as_int(lb));
          else ovf = true;
        }
      }
  }
  s_cnt[h * kTileRows + rowt] = ovf ? -1 : cnt;
  if (h == 0) s_u[rowt] = U;
  __syncthreads();

  // ---- phase 2: exact ----
  int n_listed = 0, n_all = 0, n_bad = 0;
  const float qnan = __int_as_float(0x7FC00000);
  float4 ca4[kMaxDim / 256], cb4[kMaxDim / 256];  // (loaded again: not kept live across the screen)
  load_seg_rows(car, cbr, lane, nv4, ca4, cb4);
  RowRaw nxt;
  int row_nxt = penalty ? -1 : s_row[wv * kRowsPerWave];
  load_row_raw(p, row_nxt, x_row<ITEMS>(p, row_nxt), lane, nv4, nxt);
  for (int rr = 0; rr < kRowsPerWave; ++rr) {
    const int rt = wv * kRowsPerWave + rr;
    const int row = s_row[rt];
    const RowRaw cur = nxt;
    if (rr + 1 < kRowsPerWave) {  // the next row's loads fly while this row is ranked
      row_nxt = penalty ? -1 : s_row[rt + 1];
      load_row_raw(p, row_nxt, x_row<ITEMS>(p, row_nxt), lane, nv4, nxt);
    }
    if (row < 0) continue;
    const int64_t ob = (int64_t)row * p.k;
    if (penalty) {
      if (lane < p.k) {
        p.out_local[ob + lane] = -1;
        p.out_global[ob + lane] = -1;
        p.out_dist[ob + lane] = INFINITY;
      }
      continue;
    }
    float4 v[kMaxDim / 256];
    double ss = 0.0;
    {
      const float den = s_den[rt];
#pragma unroll
      for (int m = 0; m < kMaxDim / 256; ++m) {
        const int i = lane + 64 * m;
        if (i < nv4) {
          float4 a = chain(p, widen_raw(p, cur.w[m]), ca4[m], cb4[m], cur.din);
          if (normed) a = div4(a, den);
          v[m] = a;
          ss += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
        } else {
          v[m] = z4;
        }
      }
    }
    bool bad = !(wave_sum(ss) < (double)INFINITY);  // a non-finite element of v (finite fp32 squares cannot overflow fp64)
    const int c0 = s_cnt[rt], c1 = s_cnt[kTileRows + rt];
    const bool all = c0 < 0 || c1 < 0;
    int n = count;
    if (!all) {  // the list: both halves' entries still within the final threshold
      const float uf = s_u[rt];
      int2 en = make_int2(0, __float_as_int(INFINITY));
      if (lane < c0) en = s_list[rt * CAPH + lane];
      else if (lane < c0 + c1) en = s_list[(kTileRows + rt) * CAPH + lane - c0];
      const bool keep = lane < c0 + c1 && __int_as_float(en.y) <= uf;
      const unsigned long long mk = __ballot(keep);
      if (keep) s_scr[wv][__popcll(mk & ((1ull << lane) - 1ull))] = en.x;
      n = __popcll(mk);
      if (count > 0) ++n_listed;
    } else if (count > 0) {
      ++n_all;
    }
    double bd = INFINITY;  // lanes 0 .. 7: the running top entries; 8 .. 63: this round's candidates
    int bp = INT_MAX;
    for (int c_lo = 0; c_lo < n; c_lo += kTkRound) {
      const int m = min(kTkRound, n - c_lo);
      for (int j0 = 0; j0 < m; j0 += kTkBatch) {
        double acc[kTkBatch];
        int loc[kTkBatch];
#pragma unroll
        for (int jj = 0; jj < kTkBatch; ++jj) {
          acc[jj] = 0.0;
          loc[jj] = INT_MAX;
          if (j0 + jj < m) {
            loc[jj] = all ? c_lo + j0 + jj : s_scr[wv][c_lo + j0 + jj];
            const float4* crow =
                reinterpret_cast<const float4*>(p.centers + (int64_t)topk_cand_global(p, base, loc[jj]) * p.dim);
#pragma unroll
            for (int mm = 0; mm < kMaxDim / 256; ++mm) {
              const int i = lane + 64 * mm;
              if (i < nv4) {
                const float4 c = crow[i];
                const double d0 = (double)v[mm].x - c.x, d1 = (double)v[mm].y - c.y, d2 = (double)v[mm].z - c.z,
                             d3 = (double)v[mm].w - c.w;
                acc[jj] += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
              }
            }
          }
        }
        // the re-score's halving reduction (assign.hip): lane l ends with the total of candidate
        // 4 (l >> 5) + 2 ((l >> 4) & 1) + ((l >> 3) & 1)
        double r4[4], r2[2], r1;
        const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) r4[j] = (b5 ? acc[j + 4] : acc[j]) + __shfl_xor(b5 ? acc[j] : acc[j + 4], 32);
#pragma unroll
        for (int j = 0; j < 2; ++j) r2[j] = (b4 ? r4[j + 2] : r4[j]) + __shfl_xor(b4 ? r4[j] : r4[j + 2], 16);
        r1 = (b3 ? r2[1] : r2[0]) + __shfl_xor(b3 ? r2[0] : r2[1], 8);
        r1 += __shfl_xor(r1, 4);
        r1 += __shfl_xor(r1, 2);
        r1 += __shfl_xor(r1, 1);
#pragma unroll
        for (int jj = 0; jj < kTkBatch; ++jj) {
          const double d = __shfl(r1, 32 * (jj >> 2) + 16 * ((jj >> 1) & 1) + 8 * (jj & 1));
          const bool real = loc[jj] != INT_MAX;
          bad = bad || (real && !(d < (double)INFINITY));
          if (real && lane == kTkSlots + j0 + jj) {
            bd = d;
            bp = loc[jj];
          }
        }
      }
      // rank by (d2, position) over the occupied lanes, then move rank t to lane t
      int rank = 0;
      for (int i = c_lo ? 0 : kTkSlots; i < kTkSlots + m; ++i) {
        const double di = __shfl(bd, i);
        const int pi = __shfl(bp, i);
        rank += (pi != INT_MAX && (di < bd || (di == bd && pi < bp))) ? 1 : 0;
      }
      double nd = INFINITY;
      int np = INT_MAX;
#pragma unroll
      for (int tt = 0; tt < kTkSlots; ++tt) {
        const unsigned long long mk = __ballot(rank == tt && bp != INT_MAX);
        if (mk) {
          const int src = __ffsll((long long)mk) - 1;
          const double d = __shfl(bd, src);
          const int pp = __shfl(bp, src);
          if (lane == tt) {
            nd = d;
            np = pp;
          }
        }
      }
      bd = nd;
      bp = np;
    }
    if (bad) ++n_bad;
    if (lane < p.k) {
      int ol = -1, og = -1;
      float od = INFINITY;
      if (bad) {
        od = qnan;
      } else if (bp != INT_MAX) {
        ol = p.cand_lid ? p.cand_lid[base + bp] : bp;
        og = topk_cand_global(p, base, bp);
        od = (float)sqrt(bd);
      }
      p.out_local[ob + lane] = ol;
      p.out_global[ob + lane] = og;
      p.out_dist[ob + lane] = od;
    }
  }
  if (lane == 0) {
    if (n_listed) atomicAdd(p.ws + 1, n_listed);
    if (n_all) atomicAdd(p.ws + 2, n_all);
    if (n_bad) atomicAdd(p.ws + 3, n_bad);
  }
}

// The host side of both entry points: every refusal before any HIP call, the counters zeroed, one launch.
// ITEMS = false: rqsid_assign_topk (beam is 1, n = rows).  ITEMS = true: rqsid_beam_expand (n = items).
template <bool ITEMS>
int topk_entry(const char* what, const void* x, int32_t x_format, int64_t n, int32_t beam, int32_t dim,
               const int32_t* row_index, int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off,
               int64_t max_tiles, const float* centers, const float* c_meta, int32_t n_centers,
               const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max, const int32_t* cand_idx,
               const int32_t* cand_lid, const uint8_t* seg_flags, int32_t res_levels, int32_t res_normalize,
               const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb, const float* den_in,
               float* den_out, int32_t k, int32_t* out_local, int32_t* out_global, float* out_dist, void* workspace,
               int64_t workspace_bytes, void* stream) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "%s: unknown x_format %d (RQSID_X_F32, RQSID_X_F16, RQSID_X_BF16)", what, x_format);
  if (k < 1 || k > RQSID_TOPK_MAX) return fail(RQSID_E_ARG, "%s: k = %d (1..%d)", what, k, RQSID_TOPK_MAX);
  if (ITEMS && (beam < 1 || beam > RQSID_TOPK_MAX))
    return fail(RQSID_E_ARG, "%s: beam = %d (1..%d)", what, beam, RQSID_TOPK_MAX);
  if (dim <= 0 || dim % kChunk || dim > kMaxDim)
    return fail(RQSID_E_ARG, "%s: dim = %d (a multiple of %d up to %d)", what, dim, kChunk, kMaxDim);
  if (n < 0 || n > INT32_MAX || n_segments <= 0 || max_tiles < 0 || max_tiles > INT32_MAX || cand_count_max < 0 ||
      res_levels < 0 || res_levels > 2)
    return fail(RQSID_E_ARG, "%s: bad arguments (n=%lld S=%d tiles=%lld levels=%d)", what, (long long)n, n_segments,
                (long long)max_tiles, res_levels);
  if (ITEMS && n % beam)
    return fail(RQSID_E_ARG, "%s: n_items = %lld is no multiple of beam = %d", what, (long long)n, beam);
  if (n == 0) return RQSID_OK;  // nothing to rank (the counters keep the previous call's values)
  {
    if (!x || (reinterpret_cast<uintptr_t>(x) & 15) || !seg_row_off || !seg_tile_off || !centers ||
        (reinterpret_cast<uintptr_t>(centers) & 15) || !c_meta || n_centers <= 0 || !cand_base || !cand_count ||
        !out_local || !out_global || !out_dist)
      return fail(RQSID_E_ARG, "%s: a required pointer is null (x and centers 16-byte aligned; K = %d)", what,
                  n_centers);
    if ((res_levels >= 1 && !ca) || (res_levels == 2 && (!cb || !seg_cb || (res_normalize && !den_in))))
      return fail(RQSID_E_ARG, "%s: residual inputs missing for res_levels=%d", what, res_levels);
  }
  if (!workspace || workspace_bytes < kTkHeaderBytes)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", what, (long long)workspace_bytes,
                (long long)kTkHeaderBytes);
  hipStream_t st = (hipStream_t)stream;
  int32_t* ws = static_cast<int32_t*>(workspace);
  if (fill_async(ws + 1, 0, 3 * sizeof(int32_t), st) != hipSuccess) return check_launch(what);
  if (max_tiles == 0) return check_launch(what);
  TopkParams p{};
  p.x = x;
  p.xf = x_format;
  p.n_rows = n;
  p.beam = ITEMS ? beam : 1;
  p.dim = dim;
  p.row_index = row_index;
  p.n_segments = n_segments;
  p.seg_row_off = seg_row_off;
  p.seg_tile_off = seg_tile_off;
  p.max_tiles = max_tiles;
  p.centers = centers;
  p.c_meta = reinterpret_cast<const float4*>(c_meta);
  p.n_centers = n_centers;
  p.cand_base = cand_base;
  p.cand_count = cand_count;
  p.cand_idx = cand_idx;
  p.cand_lid = cand_lid;
  p.seg_flags = seg_flags;
  p.rl = res_levels;
  p.norm = res_normalize != 0;
  p.ca = ca;
  p.seg_ca = seg_ca;
  p.cb = cb;
  p.seg_cb = seg_cb;
  p.den_in = den_in;
  p.den_out = den_out;
  p.k = k;
  p.out_local = out_local;
  p.out_global = out_global;
  p.out_dist = out_dist;
  p.ws = ws;
  p.bound_dot = (float)((2.0 * dim + 6.0) * std::ldexp(1.0, -24) * 1.01);
  p.bound_c2 = (float)(3.0 * std::ldexp(1.0, -24) * 1.01);
  if (k <= 2) hipLaunchKernelGGL((assign_topk_kernel<2, ITEMS>), dim3((unsigned)max_tiles), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((assign_topk_kernel<8, ITEMS>), dim3((unsigned)max_tiles), dim3(256), 0, st, p);
  return check_launch(what);
}

}  // namespace
}  // namespace rqsid

