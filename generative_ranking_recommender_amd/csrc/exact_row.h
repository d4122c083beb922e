// exact_row.h — the exact arithmetic that decides every returned ID, written once: the re-score and the fp32
// re-screen of rqsid_assign (assign.hip) are built from these pieces, and quant_error.hip takes its float4 steps
// from here.  Not ABI.
// (The exact pass of rqsid_assign_topk / rqsid_beam_expand, topk_kernel.h, still carries its own copy of the chain,
// the batch and the reduction: that kernel sits at its register limit, with spills, and every form of it built
// on these helpers measured 1-3 % slower at k <= 2 or at k = 8.  It must follow any change made here.)
//
// W lanes (a whole wave, 64, or half of one, 32) share one row; lane gl of the group owns the row's float4
// pieces gl + W m, m ascending.
//  * The row is rebuilt with the reference's fp32 operation sequence
//        x - ca,   / den_in (normalised),   - cb,   / den (normalised: the level's own divisor)
//    with den = fl32(sqrt(fp64 sum of squares)) + 1e-8f, the sum taken per lane in piece order and then over the
//    group by group_sum's exchanges.
//  * Candidates are scored kBatch = 8 at a time: every lane sums (v_i - c_i)^2 over its own pieces for each of the
//    eight (cand_dist2: fp64 for the exact passes, the fp32 fmaf nest for the re-screen), and batch_reduce's halving
//    reduction, selecting exchanges at W/2, W/4 and W/8 and then plain ones below, leaves lane gl with the
//    group's total of candidate batch_slot(gl): 10 shuffles for 8 sums of a wave instead of 48.
//  * The winner is the lexicographic minimum (distance, list position); a NaN distance never displaces a real one
//    (takes, group_min).
// The bits depend on the order of the sums and, because the compiler contracts a*b + c into FMAs, on the shape of
// each expression: sq4, cand_dist2 and the exchange sequences below are fixed, not merely equivalent.
#pragma once
#include <type_traits>

#include "assign_common.h"

namespace rqsid {

constexpr int kBatch = 8;  // candidates per batch_reduce

__device__ __forceinline__ float4 sub4(float4 a, float4 c) {
  return make_float4(a.x - c.x, a.y - c.y, a.z - c.z, a.w - c.w);
}
__device__ __forceinline__ float4 div4(float4 a, float d) { return make_float4(a.x / d, a.y / d, a.z / d, a.w / d); }
__device__ __forceinline__ double sq4(float4 a) {
  return (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
}

// The residual chain of level rl on one float4, up to (not including) the level's own divisor, which is a sum
// over the vector this returns.  rl and norm may be compile-time or run-time values: a constant folds.
__device__ __forceinline__ float4 chain4(float4 a, int rl, bool norm, float4 ca, float4 cb, float den_in) {
  if (rl >= 1) a = sub4(a, ca);
  if (rl >= 2) {
    if (norm) a = div4(a, den_in);
    a = sub4(a, cb);
  }
  return a;
}
// ... and through the level's own divisor den (levels >= 1 of a normalised chain)
__device__ __forceinline__ float4 chain4(float4 a, int rl, bool norm, float4 ca, float4 cb, float den_in, float den) {
  a = chain4(a, rl, norm, ca, cb, den_in);
  if (norm && rl >= 1) a = div4(a, den);
  return a;
}

// sum over the group's W lanes (W = 64: wave_sum), every lane ending with the total
template <int W>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// the divisor of a normalised level from the lanes' sums of squares
template <int W>
__device__ __forceinline__ float chain_divisor(double ss) {
  return (float)sqrt(group_sum<W>(ss)) + 1e-8f;
}

// Row `row` of x through chain4 (car / cbr: the segment's residual centre rows, read where RL asks for them):
// v[] = the lane's pieces (zeros past the row's end), returns the lane's fp64 sum of their squares.
template <int RL, bool NORM, int XF, int W, int MV>
__device__ __forceinline__ double build_row(const float* x, int64_t row, int dim, const float* car, const float* cbr,
                                            const float* den_in, int gl, float4 (&v)[MV]) {
  const int nv = dim / 4;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  double ss = 0.0;
#pragma unroll
  for (int m = 0; m < MV; ++m) {
    const int i = gl + W * m;
    if (i < nv) {
      const float4 ca = RL >= 1 ? reinterpret_cast<const float4*>(car)[i] : z4;
      const float4 cb = RL >= 2 ? reinterpret_cast<const float4*>(cbr)[i] : z4;
      const float d1 = (RL >= 2 && NORM) ? den_in[row] : 1.0f;
      const float4 a = chain4(load_row4<XF>(x, row, dim, i), RL, NORM, ca, cb, d1);
      v[m] = a;
      ss += sq4(a);
    } else {
      v[m] = z4;
    }
  }
  return ss;
}

// the lane's share of |v - c|^2 for the candidate row cr: fp64 (double)v - c per element, or the fp32 nest
template <int W, typename T, int MV>
__device__ __forceinline__ T cand_dist2(const float4 (&v)[MV], const float4* cr, int gl, int nv) {
  T acc = 0;
#pragma unroll
  for (int m = 0; m < MV; ++m) {
    const int i = gl + W * m;
    if (i < nv) {
      const float4 c = cr[i];
      if constexpr (std::is_same_v<T, double>) {
        const double d0 = (double)v[m].x - c.x, d1 = (double)v[m].y - c.y, d2 = (double)v[m].z - c.z,
                     d3 = (double)v[m].w - c.w;
        acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      } else {
        const float d0 = v[m].x - c.x, d1 = v[m].y - c.y, d2 = v[m].z - c.z, d3 = v[m].w - c.w;
        acc = fmaf(d0, d0, fmaf(d1, d1, fmaf(d2, d2, fmaf(d3, d3, acc))));
      }
    }
  }
  return acc;
}

// which candidate of the batch lane gl holds after batch_reduce, and which lane of the group holds candidate jj
template <int W>
__device__ __forceinline__ int batch_slot(int gl) {
  constexpr int s = __builtin_ctz(W / 8);  // gl's bits s + 2, s + 1, s select the halves of the three exchanges
  return 4 * ((gl >> (s + 2)) & 1) + 2 * ((gl >> (s + 1)) & 1) + ((gl >> s) & 1);
}
template <int W>
__device__ __forceinline__ constexpr int batch_lane(int jj) {
  return (W / 2) * ((jj >> 2) & 1) + (W / 4) * ((jj >> 1) & 1) + (W / 8) * (jj & 1);
}
// the group's totals of the eight per-lane sums acc[]: lane gl returns that of candidate batch_slot<W>(gl)
template <int W, typename T>
__device__ __forceinline__ T batch_reduce(const T (&acc)[kBatch], int gl) {
  T r4[4], r2[2], r1;
  const bool hi = gl & (W / 2), mid = gl & (W / 4), lo = gl & (W / 8);
#pragma unroll
  for (int j = 0; j < 4; ++j) r4[j] = (hi ? acc[j + 4] : acc[j]) + __shfl_xor(hi ? acc[j] : acc[j + 4], W / 2);
#pragma unroll
  for (int j = 0; j < 2; ++j) r2[j] = (mid ? r4[j + 2] : r4[j]) + __shfl_xor(mid ? r4[j] : r4[j + 2], W / 4);
  r1 = (lo ? r2[1] : r2[0]) + __shfl_xor(lo ? r2[0] : r2[1], W / 8);
#pragma unroll
  for (int o = W / 16; o > 0; o >>= 1) r1 += __shfl_xor(r1, o);
  return r1;
}
// One batch of a walk over n candidates, starting at j0, for a caller that needs nothing else per candidate: the
// lanes' sums for the candidates jj with j0 + jj < n (row(jj): candidate jj's centre row; the others count 0),
// then batch_reduce.  (Filled in the caller and handed over, the sums of the re-screen stay a vector across its
// loops: 8 more registers and an occupancy step.)
template <int W, typename T, int MV, typename F>
__device__ __forceinline__ T batch_dist2(const float4 (&v)[MV], int gl, int nv, int j0, int n, F&& row) {
  T acc[kBatch];
#pragma unroll
  for (int jj = 0; jj < kBatch; ++jj) {
    acc[jj] = 0;
    if (j0 + jj < n) acc[jj] = cand_dist2<W, T>(v, row(jj), gl, nv);
  }
  return batch_reduce<W>(acc, gl);
}

// does (ok, ol) displace (key, loc)?  loc == INT_MAX: nothing held yet.  Lexicographic (distance, position); a
// NaN distance is taken only where nothing is held and gives way to any real one.
__device__ __forceinline__ bool takes(double ok, int ol, double key, int loc) {
  const bool kn = key != key, okn = ok != ok;
  return ol != INT_MAX && (loc == INT_MAX || (!okn && (kn || ok < key || (ok == key && ol < loc))));
}
// that minimum over the group's batch_reduce results: every lane ends with the batch's winner
template <int W>
__device__ __forceinline__ void group_min(double& key, int& loc) {
#pragma unroll
  for (int o = W / 8; o < W; o <<= 1) {
    const double ok = __shfl_xor(key, o);
    const int ol = __shfl_xor(loc, o);
    const bool take = takes(ok, ol, key, loc);
    key = take ? ok : key;
    loc = take ? ol : loc;
  }
}

}  // namespace rqsid
