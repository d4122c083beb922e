// beam.hip — the two steps of a beam-search encode (include/rqsid.h; semantics and item layout: DESIGN.md §3.1h).
//   rqsid_beam_expand  rqsid_assign_topk over n_rows * beam items, item i reading row i / beam of x: the kernel of
//                      topk_kernel.h instantiated with ITEMS = true (no residual or replicated matrix is written);
//   rqsid_beam_merge   per row, the next beam out of the beam_in * k expansions: slot 0 is the greedy continuation
//                      (parent 0, place 0), the other slots the remaining live expansions by (rec, parent, place).
//                      One wave per row, lane = parent * k + place, ranks by counting: no atomics, every write's
//                      position is a pure function of the row's inputs.
#include "topk_kernel.h"

namespace rqsid {
namespace {

constexpr int kMergeRowsPerBlock = 4;  // one wave each
constexpr int kMergeMaxLevel = 7;      // path prefixes of up to 7 ids in, 8 out

struct MergeParams {
  int64_t n_rows;
  int32_t beam_in, k, beam_out, level, use_global, key_mult, dead_key;
  const int32_t* exp_local;
  const int32_t* exp_global;
  const float* exp_dist;
  const float* scale_in;
  const float* den;
  const int32_t* path_in;
  int32_t* path_out;
  float* scale_out;
  float* den_next;
  float* rec_out;
  int32_t* key_out;
  int32_t* src_out;
};

__global__ __launch_bounds__(64 * kMergeRowsPerBlock) void beam_merge_kernel(MergeParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kMergeRowsPerBlock + (threadIdx.x >> 6);
  if (row >= p.n_rows) return;  // (wave-uniform)
  const int ne = p.beam_in * p.k;  // <= 64: one expansion per lane, in (parent, place) order
  const bool in = lane < ne;
  const int h = in ? lane / p.k : 0, place = lane - h * p.k;
  const int64_t item = row * p.beam_in + h;
  float S = 1.0f, sc = 1.0f, den = 1.0f, d = INFINITY;
  int g = -1, loc = -1;
  if (in) {
    sc = p.scale_in ? p.scale_in[item] : 1.0f;
    den = p.den ? p.den[item] : 1.0f;
    S = sc * den;  // S_l = fl32(S_{l-1} den_l)
    const int64_t e = item * p.k + place;
    g = p.exp_global[e];
    loc = p.exp_local[e];
    d = p.exp_dist[e];
  }
  const int id = p.use_global ? g : loc;
  // a row with a non-finite value (the expansion reports NaN, or an earlier level passed NaN on in the scale; den
  // is not asked: the expand leaves it unwritten for an item of a penalty segment, whose expansions are all dead)
  const bool row_nan = __ballot(in && (d != d || sc != sc)) != 0ull;
  const float rec = (in && g >= 0 && id >= 0) ? S * d : INFINITY;  // fl32(S_l d)
  const bool live = in && !row_nan && fabsf(rec) <= FLT_MAX;
  const unsigned long long livemask = __ballot(live);
  const unsigned long long candmask = livemask & ~1ull;  // lane 0 is the forced slot 0
  int rank = 0;
  for (int j = 1; j < ne; ++j) {
    const float rj = __shfl(rec, j);
    if ((candmask >> j) & 1ull) rank += (rj < rec || (rj == rec && j < lane)) ? 1 : 0;
  }
  const int n_cand = __popcll(candmask);
  int slot = -1;
  if (lane == 0) slot = live ? 0 : -1;
  else if (live && rank + 1 < p.beam_out) slot = rank + 1;
  const int pl = p.level + 1;
  if (slot >= 0) {
    const int64_t o = row * p.beam_out + slot;
    const int32_t* pin = p.path_in + item * p.level;  // (not read at level 0)
    for (int i = 0; i < p.level; ++i) p.path_out[o * pl + i] = pin[i];
    p.path_out[o * pl + p.level] = id;
    p.scale_out[o] = S;
    p.den_next[o] = den;
    p.rec_out[o] = rec;
    p.key_out[o] = (p.level >= 1 ? pin[p.level - 1] * p.key_mult : 0) + id;
    p.src_out[o] = lane;
  }
  if (lane < p.beam_out) {  // the slots nothing took
    const bool dead = lane == 0 ? !(livemask & 1ull) : lane - 1 >= n_cand;
    if (dead) {
      const float qnan = __int_as_float(0x7FC00000);
      const int64_t o = row * p.beam_out + lane;
      for (int i = 0; i < pl; ++i) p.path_out[o * pl + i] = -1;
      p.scale_out[o] = row_nan ? qnan : 1.0f;
      p.den_next[o] = 1.0f;
      p.rec_out[o] = row_nan ? qnan : INFINITY;
      p.key_out[o] = p.dead_key;
      p.src_out[o] = -1;
    }
  }
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int64_t rqsid_beam_expand_workspace_bytes(int64_t n_items, int32_t k) {
  (void)n_items;
  (void)k;
  return kTkHeaderBytes;  // as rqsid_assign_topk: every list lives in LDS
}

int rqsid_beam_expand(const void* x, int32_t x_format, int64_t n_items, int32_t beam, int32_t dim,
                      const int32_t* row_index, int32_t n_segments, const int32_t* seg_row_off,
                      const int32_t* seg_tile_off, int64_t max_tiles, const float* centers, const float* c_meta,
                      int32_t n_centers, const int32_t* cand_base, const int32_t* cand_count, int32_t cand_count_max,
                      const int32_t* cand_idx, const int32_t* cand_lid, const uint8_t* seg_flags, int32_t res_levels,
                      int32_t res_normalize, const float* ca, const int32_t* seg_ca, const float* cb,
                      const int32_t* seg_cb, const float* den_in, float* den_out, int32_t k, int32_t* out_local,
                      int32_t* out_global, float* out_dist, void* workspace, int64_t workspace_bytes, void* stream) {
  return topk_entry<true>("beam_expand", x, x_format, n_items, beam, dim, row_index, n_segments, seg_row_off,
                          seg_tile_off, max_tiles, centers, c_meta, n_centers, cand_base, cand_count, cand_count_max,
                          cand_idx, cand_lid, seg_flags, res_levels, res_normalize, ca, seg_ca, cb, seg_cb, den_in,
                          den_out, k, out_local, out_global, out_dist, workspace, workspace_bytes, stream);
}

int rqsid_beam_merge(int64_t n_rows, int32_t beam_in, int32_t k, int32_t beam_out, int32_t level,
                     const int32_t* exp_local, const int32_t* exp_global, const float* exp_dist,
                     const float* scale_in, const float* den, const int32_t* path_in, int32_t use_global,
                     int32_t key_mult, int32_t dead_key, int32_t* path_out, float* scale_out, float* den_next,
                     float* rec_out, int32_t* key_out, int32_t* src_out, void* stream) {
  if (beam_in < 1 || beam_in > RQSID_TOPK_MAX || k < 1 || k > RQSID_TOPK_MAX || beam_out < 1 ||
      beam_out > RQSID_TOPK_MAX || beam_out > beam_in * k)
    return fail(RQSID_E_ARG, "beam_merge: beam_in = %d, k = %d, beam_out = %d (each 1..%d, beam_out <= beam_in k)",
                beam_in, k, beam_out, RQSID_TOPK_MAX);
  if (level < 0 || level > kMergeMaxLevel) return fail(RQSID_E_ARG, "beam_merge: level = %d (0..%d)", level, kMergeMaxLevel);
  if (n_rows < 0 || n_rows * beam_in > INT32_MAX || n_rows * beam_out > INT32_MAX)
    return fail(RQSID_E_ARG, "beam_merge: n_rows = %lld (items up to 2^31 - 1)", (long long)n_rows);
  if (n_rows == 0) return RQSID_OK;
  if (!exp_local || !exp_global || !exp_dist || (level >= 1 && !path_in) || !path_out || !scale_out || !den_next ||
      !rec_out || !key_out || !src_out)
    return fail(RQSID_E_ARG, "beam_merge: a required pointer is null (level = %d)", level);
  MergeParams p{};
  p.n_rows = n_rows;
  p.beam_in = beam_in;
  p.k = k;
  p.beam_out = beam_out;
  p.level = level;
  p.use_global = use_global != 0;
  p.key_mult = key_mult;
  p.dead_key = dead_key;
  p.exp_local = exp_local;
  p.exp_global = exp_global;
  p.exp_dist = exp_dist;
  p.scale_in = scale_in;
  p.den = den;
  p.path_in = path_in;
  p.path_out = path_out;
  p.scale_out = scale_out;
  p.den_next = den_next;
  p.rec_out = rec_out;
  p.key_out = key_out;
  p.src_out = src_out;
  hipLaunchKernelGGL(beam_merge_kernel, dim3((unsigned)cdiv(n_rows, kMergeRowsPerBlock)),
                     dim3(64 * kMergeRowsPerBlock), 0, (hipStream_t)stream, p);
  return check_launch("beam_merge");
}

}  // extern "C"
