// assign_topk.hip — rqsid_assign_topk: the k nearest allowed centres per row and segment, exactly
// (include/rqsid.h; bound, list capacity and counters: DESIGN.md §3.1g).  The kernel and the host checks live in
// topk_kernel.h, shared with rqsid_beam_expand (beam.hip); this entry point instantiates the row form (ITEMS = false),
// which has no division and writes den_out at res_levels 1 only.
#include "topk_kernel.h"

using namespace rqsid;

extern "C" {

int64_t rqsid_assign_topk_workspace_bytes(int64_t n_rows, int32_t k) {
  (void)n_rows;
  (void)k;
  return kTkHeaderBytes;  // every list lives in LDS: the header alone
}

int rqsid_assign_topk(const void* x, int32_t x_format, int64_t n_rows, int32_t dim, const int32_t* row_index,
                      int32_t n_segments, const int32_t* seg_row_off, const int32_t* seg_tile_off, int64_t max_tiles,
                      const float* centers, const float* c_meta, int32_t n_centers, const int32_t* cand_base,
                      const int32_t* cand_count, int32_t cand_count_max, const int32_t* cand_idx,
                      const int32_t* cand_lid, const uint8_t* seg_flags, int32_t res_levels, int32_t res_normalize,
                      const float* ca, const int32_t* seg_ca, const float* cb, const int32_t* seg_cb,
                      const float* den_in, float* den_out, int32_t k, int32_t* out_local, int32_t* out_global,
                      float* out_dist, void* workspace, int64_t workspace_bytes, void* stream) {
  return topk_entry<false>("assign_topk", x, x_format, n_rows, 1, dim, row_index, n_segments, seg_row_off,
                           seg_tile_off, max_tiles, centers, c_meta, n_centers, cand_base, cand_count, cand_count_max,
                           cand_idx, cand_lid, seg_flags, res_levels, res_normalize, ca, seg_ca, cb, seg_cb, den_in,
                           den_out, k, out_local, out_global, out_dist, workspace, workspace_bytes, stream);
}

}  // extern "C"
