// quant_error.hip — quantisation error of a residual-quantisation encoding (rqsid_quant_error).
//
// The encode kernels (assign.hip) rebuild the residual chain x - c0[id0], / (||.|| + 1e-8), - c1[id1], ... in
// registers to choose the IDs and throw it away.  This kernel rebuilds it once more for IDs that are already
// chosen and keeps what the chain says about them: per level the distance from the level's input vector to the
// centre it was given, the row norm, and deterministic fp64 totals.  The arithmetic is the fp32 operation
// sequence of _compute_residuals_with_centers (hierarchical_rq_kmeans.py:1088-1128, res_normalize = 1) or of the
// simplified generator's plain residuals (simplified_semantic_id_generator.py:78-96,164-168, res_normalize = 0),
// i.e. that of exact_row.h (the float4 steps are its own) and of rqsid_residual with one dimension group.
//
// Shape: one wave per row, lanes over the row's dim/4 float4 pieces (16-byte loads only); a wave owns runs of
// kQeRun consecutive positions of the processing order and works through a run two rows at a time, so that the
// cross-lane fp64 reductions of the two rows share one butterfly, with the next pair's rows and last-level
// centre rows already in flight.  The centre rows of every level but the last stay in registers and are
// reloaded only when the id differs from the previous row's (a wave-uniform branch): in the order of the last
// level's bucketing they change once per group, so a data row costs its own bytes from HBM plus one last-level
// centre row from L2.  The ids and the row numbers of a run are read once, lane-parallel, and handed out with
// v_readlane; the per-row results are collected on the lane of the row's position and written at the end of the
// run.  Totals: every lane adds its rows' squares in position order, a wave and then a block sum theirs in a
// fixed order into one partial per block, and a second one-block kernel adds the partials in block order: no
// float atomics anywhere (they would not be bitwise reproducible).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "assign_common.h"
#include "exact_row.h"  // sub4, div4, sq4

namespace rqsid {
namespace {

constexpr int kQeRun = 64;            // positions per run: one per lane
constexpr int kQeMaxBlocks = 2048;    // persistent grid cap = number of partial records
constexpr int kQeMaxLevels = 3;
constexpr int kQeErrBytes = 256;      // workspace [0, 4): sticky error word; partials from byte 256
constexpr int kQeRec = kQeMaxLevels + 1;  // doubles per partial record
constexpr uint32_t kQeErrId = 1u;     // an id outside [0, k_l)
constexpr uint32_t kQeErrRow = 2u;    // a row_order entry outside [0, n_rows)

struct QeParams {
  const float* x;  // rows in the kernel's XF format
  const int32_t* row_order;
  const float* c[kQeMaxLevels];
  const int32_t* id[kQeMaxLevels];
  int32_t k[kQeMaxLevels];
  float* err;
  float* x_norm;
  double* partials;
  uint32_t* err_word;
  int64_t n;
  int32_t dim;
  int32_t normalize;
};

__device__ __forceinline__ int clamp_id(int32_t id, int32_t k) { return (unsigned)id < (unsigned)k ? id : 0; }

// the rows of one pair of positions and their last-level centre rows
template <int MV>
struct QePair {
  float4 xa[MV], xb[MV], ca[MV], cb[MV];
};

template <int XF, int L, int MV>
__global__ __launch_bounds__(256) void quant_error_kernel(QeParams p) {
  __shared__ double wave_part[4][kQeRec];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nv = p.dim / 4;
  const int64_t dim = p.dim;
  const bool norm = p.normalize != 0;
  const int64_t nruns = (p.n + kQeRun - 1) / kQeRun;

  double acc[L + 1];
#pragma unroll
  for (int q = 0; q <= L; ++q) acc[q] = 0.0;
  uint32_t errs = 0;
  // centre rows of the levels before the last, kept while the id stays the same
  float4 held[L > 1 ? L - 1 : 1][MV];
  int held_id[L > 1 ? L - 1 : 1];
#pragma unroll
  for (int l = 0; l < (L > 1 ? L - 1 : 1); ++l) held_id[l] = -1;

  for (int64_t run = (int64_t)blockIdx.x * 4 + wv; run < nruns; run += (int64_t)gridDim.x * 4) {
    const int64_t pos0 = run * kQeRun;
    const int cnt = (int)(p.n - pos0 < kQeRun ? p.n - pos0 : kQeRun);
    // lane j: the row of position pos0 + j and its ids (never used to form an address unless in range)
    int32_t r_row = 0, r_id[L];
    int bad_from = L;      // first level whose id is out of range
    bool row_ok = false;   // this lane's position exists and names a row
    if (lane < cnt) {
      const int64_t pos = pos0 + lane;
      const int32_t rr = p.row_order ? p.row_order[pos] : (int32_t)pos;
      row_ok = (uint32_t)rr < (uint64_t)p.n;
      if (!row_ok) errs |= kQeErrRow;
      r_row = row_ok ? rr : 0;
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      int32_t v = 0;
      if (row_ok) {
        v = p.id[l][r_row];
        if ((unsigned)v >= (unsigned)p.k[l]) {
          bad_from = bad_from < l ? bad_from : l;
          errs |= kQeErrId;
          v = 0;
        }
      }
      r_id[l] = v;
    }
    // lane j collects the fp64 sums of squares of position pos0 + j; their square roots are taken once per run,
    // lane-parallel, except where the next level's divisor needs one at once
    double s_keep[L], sx_keep = 0.0;
#pragma unroll
    for (int l = 0; l < L; ++l) s_keep[l] = 0.0;

    auto load_pair = [&](QePair<MV>& q, int j) {
      const int jb = j + 1 < cnt ? j + 1 : j;
      const int64_t ra = __builtin_amdgcn_readlane(r_row, j), rb = __builtin_amdgcn_readlane(r_row, jb);
      const int ga = clamp_id(__builtin_amdgcn_readlane(r_id[L - 1], j), p.k[L - 1]);
      const int gb = clamp_id(__builtin_amdgcn_readlane(r_id[L - 1], jb), p.k[L - 1]);
      const float4* cra = reinterpret_cast<const float4*>(p.c[L - 1] + ga * dim);
      const float4* crb = reinterpret_cast<const float4*>(p.c[L - 1] + gb * dim);
#pragma unroll
      for (int m = 0; m < MV; ++m) {
        const int i = lane + 64 * m;
        if (i < nv) {
          q.xa[m] = load_row4<XF>(p.x, ra, p.dim, i);
          q.xb[m] = load_row4<XF>(p.x, rb, p.dim, i);
          q.ca[m] = cra[i];
          q.cb[m] = crb[i];
        } else {
          q.xa[m] = q.xb[m] = q.ca[m] = q.cb[m] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    };

    QePair<MV> nxt;
    load_pair(nxt, 0);
    for (int j = 0; j < cnt; j += 2) {
      QePair<MV> cur = nxt;
      if (j + 2 < cnt) load_pair(nxt, j + 2);
      const int jb = j + 1 < cnt ? j + 1 : j;  // an odd tail computes its last row twice
      double sxa = 0.0, sxb = 0.0;
#pragma unroll
      for (int m = 0; m < MV; ++m) {
        sxa += sq4(cur.xa[m]);
        sxb += sq4(cur.xb[m]);
      }
#pragma unroll
      for (int l = 0; l < L; ++l) {
        double sa = 0.0, sb = 0.0;
        if (l == L - 1) {
#pragma unroll
          for (int m = 0; m < MV; ++m) {
            cur.xa[m] = sub4(cur.xa[m], cur.ca[m]);
            cur.xb[m] = sub4(cur.xb[m], cur.cb[m]);
            sa += sq4(cur.xa[m]);
            sb += sq4(cur.xb[m]);
          }
        } else {
          const int hl = l < L - 1 ? l : 0;
          const int ga = clamp_id(__builtin_amdgcn_readlane(r_id[l], j), p.k[l]);
          if (ga != held_id[hl]) {
            const float4* cr = reinterpret_cast<const float4*>(p.c[l] + ga * dim);
#pragma unroll
            for (int m = 0; m < MV; ++m) held[hl][m] = lane + 64 * m < nv ? cr[lane + 64 * m] : make_float4(0.f, 0.f, 0.f, 0.f);
            held_id[hl] = ga;
          }
#pragma unroll
          for (int m = 0; m < MV; ++m) {
            cur.xa[m] = sub4(cur.xa[m], held[hl][m]);
            sa += sq4(cur.xa[m]);
          }
          const int gb = clamp_id(__builtin_amdgcn_readlane(r_id[l], jb), p.k[l]);
          if (gb != held_id[hl]) {
            const float4* cr = reinterpret_cast<const float4*>(p.c[l] + gb * dim);
#pragma unroll
            for (int m = 0; m < MV; ++m) held[hl][m] = lane + 64 * m < nv ? cr[lane + 64 * m] : make_float4(0.f, 0.f, 0.f, 0.f);
            held_id[hl] = gb;
          }
#pragma unroll
          for (int m = 0; m < MV; ++m) {
            cur.xb[m] = sub4(cur.xb[m], held[hl][m]);
            sb += sq4(cur.xb[m]);
          }
        }
        // one butterfly for the pair (and, at level 0, for the two row norms): wave_sum's order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          sa += __shfl_xor(sa, o);
          sb += __shfl_xor(sb, o);
          if (l == 0) {
            sxa += __shfl_xor(sxa, o);
            sxb += __shfl_xor(sxb, o);
          }
        }
        s_keep[l] = lane == j ? sa : s_keep[l];
        s_keep[l] = lane == jb ? sb : s_keep[l];
        if (l == 0) {
          sx_keep = lane == j ? sxa : sx_keep;
          sx_keep = lane == jb ? sxb : sx_keep;
        }
        if (l < L - 1 && norm) {
          const float da = (float)sqrt(sa) + 1e-8f, db = (float)sqrt(sb) + 1e-8f;
#pragma unroll
          for (int m = 0; m < MV; ++m) {
            cur.xa[m] = div4(cur.xa[m], da);
            cur.xb[m] = div4(cur.xb[m], db);
          }
        }
      }
    }

    if (row_ok) {
      const bool clean = bad_from == L;
#pragma unroll
      for (int l = 0; l < L; ++l) {
        const float e = (float)sqrt(s_keep[l]);
        p.err[(int64_t)l * p.n + r_row] = l >= bad_from ? __uint_as_float(0x7FC00000u) : e;
        if (clean) acc[l] += (double)e * e;
      }
      const float xn_keep = (float)sqrt(sx_keep);
      if (p.x_norm) p.x_norm[r_row] = xn_keep;
      if (clean) acc[L] += (double)xn_keep * xn_keep;
    }
  }

  if (errs) atomicOr(p.err_word, errs);
#pragma unroll
  for (int q = 0; q <= L; ++q) {
    const double t = wave_sum(acc[q]);
    if (lane == 0) wave_part[wv][q] = t;
  }
  __syncthreads();
  if (threadIdx.x <= L) {
    const int q = threadIdx.x;
    p.partials[(int64_t)blockIdx.x * kQeRec + q] = ((wave_part[0][q] + wave_part[1][q]) + wave_part[2][q]) + wave_part[3][q];
  }
}

// sums[q]: wave q adds the partial records of total q, lane i those of blocks i, i + 64, ... in that order, then
// the lanes' sums in wave_sum's order: a fixed order for a fixed grid
__global__ __launch_bounds__(64 * kQeRec) void quant_error_sum_kernel(const double* __restrict__ partials,
                                                                      int n_blocks, int n_out,
                                                                      double* __restrict__ sums) {
  const int q = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double t = 0.0;
  if (q < n_out)
    for (int b = lane; b < n_blocks; b += 64) t += partials[(int64_t)b * kQeRec + q];
  t = wave_sum(t);
  if (q < n_out && lane == 0) sums[q] = t;
}

template <int XF, int L>
void launch_mv(const QeParams& p, unsigned blocks, hipStream_t st) {
  if (p.dim <= 256) hipLaunchKernelGGL((quant_error_kernel<XF, L, 1>), dim3(blocks), dim3(256), 0, st, p);
  else if (p.dim <= 512) hipLaunchKernelGGL((quant_error_kernel<XF, L, 2>), dim3(blocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((quant_error_kernel<XF, L, 4>), dim3(blocks), dim3(256), 0, st, p);
}
template <int XF>
void launch_levels(const QeParams& p, int n_levels, unsigned blocks, hipStream_t st) {
  if (n_levels == 1) launch_mv<XF, 1>(p, blocks, st);
  else if (n_levels == 2) launch_mv<XF, 2>(p, blocks, st);
  else launch_mv<XF, 3>(p, blocks, st);
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int64_t rqsid_quant_error_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0) return fail(RQSID_E_ARG, "quant_error_workspace_bytes: n_rows = %lld", (long long)n_rows);
  return kQeErrBytes + (int64_t)kQeMaxBlocks * kQeRec * (int64_t)sizeof(double);
}

int rqsid_quant_error(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_order,
                      int32_t n_levels, int32_t res_normalize, const float* c0, int32_t k0, const int32_t* id0,
                      const float* c1, int32_t k1, const int32_t* id1, const float* c2, int32_t k2,
                      const int32_t* id2, float* err, float* x_norm, double* sums, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "rqsid_quant_error: unknown x_format %d", x_format);
  if (n_levels < 1 || n_levels > kQeMaxLevels)
    return fail(RQSID_E_ARG, "rqsid_quant_error: n_levels = %d (1..%d)", n_levels, kQeMaxLevels);
  if (dim <= 0 || dim % kChunk || dim > kMaxDim)
    return fail(RQSID_E_ARG, "rqsid_quant_error: dim = %d (a multiple of %d up to %d)", dim, kChunk, kMaxDim);
  if (n_rows < 0 || n_rows > INT32_MAX)
    return fail(RQSID_E_ARG, "rqsid_quant_error: n_rows = %lld", (long long)n_rows);
  const float* cs[kQeMaxLevels] = {c0, c1, c2};
  const int32_t* ids[kQeMaxLevels] = {id0, id1, id2};
  const int32_t ks[kQeMaxLevels] = {k0, k1, k2};
  for (int l = 0; l < n_levels; ++l)
    if (!cs[l] || !ids[l] || ks[l] <= 0 || ((uintptr_t)cs[l] & 15))
      return fail(RQSID_E_ARG, "rqsid_quant_error: level %d needs centres (16-byte aligned), ids and k > 0 (k = %d)",
                  l, ks[l]);
  if (!err || !x || ((uintptr_t)x & 15))
    return fail(RQSID_E_ARG, "rqsid_quant_error: x (16-byte aligned) and err are required");
  const int64_t need = rqsid_quant_error_workspace_bytes(n_rows);
  if (!workspace || workspace_bytes < need)
    return fail(RQSID_E_WORKSPACE, "rqsid_quant_error: workspace %lld < %lld bytes", (long long)workspace_bytes,
                (long long)need);
  hipStream_t st = (hipStream_t)stream;
  if (n_rows == 0) {
    if (sums && fill_async(sums, 0, (size_t)(n_levels + 1) * sizeof(double), st) != hipSuccess)
      return check_launch("rqsid_quant_error (zero sums)");
    return RQSID_OK;
  }
  QeParams p;
  p.x = reinterpret_cast<const float*>(x);
  p.row_order = row_order;
  for (int l = 0; l < kQeMaxLevels; ++l) {
    p.c[l] = l < n_levels ? cs[l] : nullptr;
    p.id[l] = l < n_levels ? ids[l] : nullptr;
    p.k[l] = l < n_levels ? ks[l] : 0;
  }
  p.err = err;
  p.x_norm = x_norm;
  p.partials = reinterpret_cast<double*>(static_cast<char*>(workspace) + kQeErrBytes);
  p.err_word = static_cast<uint32_t*>(workspace);
  p.n = n_rows;
  p.dim = dim;
  p.normalize = res_normalize;
  const unsigned blocks = grid_cap(cdiv(cdiv(n_rows, kQeRun), 4), kQeMaxBlocks);
  if (x_format == RQSID_X_F32) launch_levels<RQSID_X_F32>(p, n_levels, blocks, st);
  else if (x_format == RQSID_X_F16) launch_levels<RQSID_X_F16>(p, n_levels, blocks, st);
  else launch_levels<RQSID_X_BF16>(p, n_levels, blocks, st);
  int rc;
  if ((rc = check_launch("rqsid_quant_error"))) return rc;
  if (sums) {
    hipLaunchKernelGGL(quant_error_sum_kernel, dim3(1), dim3(64 * kQeRec), 0, st, p.partials, (int)blocks, n_levels + 1, sums);
    if ((rc = check_launch("rqsid_quant_error (sums)"))) return rc;
  }
  return RQSID_OK;
}

}  // extern "C"
