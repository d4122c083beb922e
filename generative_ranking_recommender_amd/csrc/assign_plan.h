// assign_plan.h — which screen rqsid_assign_x runs, and what follows it, as a pure function of the call's
// shape and of the RQSID_* switches.  Host-only and self-contained: no HIP header, no getenv (the caller
// reads the environment once per call, read_assign_env in assign.hip), plain C++17, so
// tests/test_assign_plan.py builds it with g++ and checks the table without a GPU.  Each screen's
// translation unit ties its own constants to the ones below with a static_assert.
#pragma once
#include <cstdint>

namespace rqsid {

constexpr int kPlanXF32 = 0;         // RQSID_X_F32 (include/rqsid.h); every other format is a 16-bit row
constexpr int kPlanMaxList = 8;      // kMaxList: candidates a work item lists
constexpr int kPlanSplitDim = 512;   // kSplitDim: widest row of the candidate-split per-tile form
constexpr int kPlanHalfDim = 512;    // kHalfDim: widest row of the two-rows-per-wave re-score and the re-screen
constexpr int kPlanStreamDim = 512;  // kSDim: the streamed screens' row width
constexpr int kPlanStreamMinRows = 64 * 256;  // fewer rows cannot fill the persistent grid
constexpr int kPlanPcDim = 512;      // kQDim
constexpr int kPlanPcRows = 128;     // kQRows: rows per producer/consumer tile
constexpr int kPlanPcDescBytes = 32; // sizeof(PcDesc)
constexpr int kPlanResDim = 512;     // kRD: the centre-resident screen's row width
constexpr int kPlanRowsDim = 512;    // kRDim: the row-resident screen's row width
constexpr int kPlanRowsMaxCand = 512;  // kRMaxCand
constexpr int kPlanPairCand = 128;   // kPairCand: candidates per segment of the pair table
constexpr int kPlanWorkItemBytes = 32;    // sizeof(WorkItem)
constexpr int kPlanDescBytesPerRow = 16;  // the workspace's descriptor area: one int4 per row

// Byte offsets of the rqsid_assign workspace (rqsid_assign_workspace_bytes = total_bytes).  Every per-row
// area holds n_rows entries; the int areas are padded to 256 B.
//
//   area      entry      per-tile        streamed         row-resident     centre-resident        producer/consumer
//   header    64 int     work count [0], overflow count [kOvfSlot], resident error word [48], sticky errors [kErrSlot]
//   work      WorkItem   compact list    item of row r    compact list     pass masks, then the   item of row r
//                                        at work[r]                        item, at work[r]       at work[r]
//   tile_seg  int        tile -> seg     tile -> seg      tile -> seg      segment of each        tile -> seg
//                        (128-row)       (256-row)        (128 / 256-row)  ambiguous row          (128 / 256-row)
//   work_idx  int        -               R-row tile offsets per segment (resident: 32-row) while the screen runs,
//                                        then the compacted list of sentinel rows (row-resident: offsets only)
//   desc      16 B       -               -                -                int4 tile descriptors  PcDesc tile descriptors
//   ovf_list  int        the fp32 re-screen's list of "every candidate" items (every screen)
struct AssignWorkspaceMap {
  int64_t header = 0, work = 256, tile_seg, work_idx, desc, ovf_list, total_bytes;
  explicit AssignWorkspaceMap(int64_t n_rows) {
    const int64_t n = n_rows > 0 ? n_rows : 0, ints = (n * 4 + 255) / 256 * 256;
    tile_seg = work + n * kPlanWorkItemBytes;
    work_idx = tile_seg + ints;
    desc = work_idx + ints;
    ovf_list = desc + n * kPlanDescBytesPerRow;
    total_bytes = ovf_list + ints;
  }
};

// ring depth of the candidate-split form (one block per CU).  S = 3 (96 KiB in flight per CU instead of
// 48) measured no faster on the XL levels (L2 15.3 vs 14.8 ms), so the smaller ring stays
#ifndef RQSID_SPLIT_S
#define RQSID_SPLIT_S 2
#endif
constexpr int kSplitS = RQSID_SPLIT_S;

// what the dispatch reads of a call
struct AssignShape {
  int x_format = kPlanXF32;
  int64_t n_rows = 0;
  int dim = 0;
  int n_segments = 0;
  int cand_count_max = 0;
  int res_levels = 0;
  bool norm = false;
  int screen_terms = 0;  // 0 auto, 1, 2 (needs has_pair), 3
  bool has_cand_lid = false;
  bool has_den_out = false;
  bool has_pair = false;  // the call brings a pair table (rqsid_pair_table): |c_j - c_k| per segment list
};

// every switch the assign path reads, with its default
struct AssignEnv {
  // RQSID_SCREEN_VARIANT (tuning / A-B tests): 0 default; 1: per-tile kernel only; 2: per-tile kernel with the
  // multi-sweep list epilogue on single-pass segments; 5: the persistent streamed kernels (stream_shape) where
  // they apply; 6: the centre-resident screen; 7: no candidate split; 8: the row-resident screen (rows_shape);
  // 9: the producer/consumer screen wherever it applies
  int screen_variant = 0;
  int pc = 1;              // RQSID_PC: 0 never, 1 the 1-term levels, 2 the 3-term ones too
  int pcw = 0;             // RQSID_PCW=1: the wide producer/consumer form on 1-term levels (A/B: measured slower)
  int stream_shape = 83;   // RQSID_STREAM_SHAPE: 83 (8 waves x 3 stages), 42 (4 x 2), 88 (ping-pong 8-wave form)
  // RQSID_ROWS_SHAPE = 100 W + 10 S + SR (waves, centre ring stages, per-wave row ring stages): 443 and 482: 4
  // waves, two blocks per CU; 883: 8 waves, one block per CU
  int rows_shape = 443;
  int rescore_full = 0;    // RQSID_RESCORE_FULL=1: one row per wave in the re-score (A/B)
  int no_rescreen = 0;     // RQSID_NO_RESCREEN=1: no fp32 re-screen (A/B)
  int no_pair = 0;         // RQSID_NO_PAIR=1: the 3-term screen where the 2-term pairwise form would run (A/B)
  int test_force_spin_cap = 0;  // RQSID_TEST_FORCE_SPIN_CAP (tests only)
};

struct AssignPlan {
  enum Screen { kTile, kStream, kRows, kResident, kPc };
  Screen screen = kTile;
  bool t3 = false;  // 3-term screen (or its 2-term pairwise form: pair)
  // per-tile screen, single pass, fp32 rows, <= 128 candidates: centres hi + lo, rows hi only, the row-rounding
  // part of the bound charged pairwise through the call's pair table
  bool pair = false;
  int nt = 4;       // MFMA candidate tiles per wave (tile, stream, pc)
  // per-tile screen only: single-pass epilogue, candidate groups (2: the candidate-split form), ring depth
  bool one = false;
  int cw = 1;
  int s = 2;
  int stream_shape = 0;  // kStream: 83, 42, 88
  int rows_shape = 0;    // kRows: 443, 482, 883
  bool pc_wide = false;  // kPc: 256-row tiles
  // after the screen
  bool compact = false;  // sentinel rows -> work_idx list
  bool expand = false;   // resident screen: pass masks -> work items
  bool rescreen = false; // fp32 list for the rows the screen left with "every candidate"
  bool half = false;     // two rows per wave in the exact re-score
  bool force_cap = false;
  bool read_err_word = false;
};

inline bool stream_supported(int nt, bool t3, int rl) {
  if (nt == 8) return !t3 && rl >= 0 && rl <= 2;
  if (nt == 4) return rl >= 0 && rl <= 2;
  return false;
}
// row-resident screen: 512-d rows, 1 term, <= 512 candidates per segment; no normalised first-level build
inline bool rows_supported(int dim, int cand_count_max, bool t3, int rl, bool norm) {
  return dim == kPlanRowsDim && !t3 && cand_count_max > 0 && cand_count_max <= kPlanRowsMaxCand && rl >= 0 && rl <= 2 &&
         !(rl == 1 && norm);
}
// centre-resident screen: one fp16 term only: the 3-term form (hi / lo centre waves) does not fit the LDS
// budget and registers beside the one-exchange epilogue (the per-tile screen serves those levels)
inline bool resident_supported(int dim, int cand_count_max, bool t3) {
  return dim == kPlanResDim && cand_count_max >= 1 && cand_count_max <= 256 && !t3;
}
// producer/consumer screen: 512-d residual levels, 3-term <= 128 or 1-term <= 256 candidates per segment
inline bool pc_supported(int dim, int cand_count_max, bool t3, int rl) {
  if (dim != kPlanPcDim || rl < 1 || rl > 2) return false;
  return t3 ? cand_count_max <= 128 : cand_count_max <= 256;
}
inline int64_t pc_desc_bytes(int64_t n_rows, int32_t n_segments) {
  return ((n_rows > 0 ? n_rows : 0) / kPlanPcRows + (int64_t)n_segments + 1) * kPlanPcDescBytes;
}

// The decision.  Priority: producer/consumer, row-resident, centre-resident, streamed, per-tile.
//  * Terms: the 3-term screen (rounding residuals of both operands summed by two more MFMAs) shrinks the
//    bound ~5x at 2 blocks/CU; auto picks it for residual levels with <= 128 candidates, and for first
//    residual levels of <= 256 (the XL preset's middle level: the 1-term bound leaves ~2/3 of those rows to
//    the fp64 re-score).  The 8-tile form has no 3-term build (256 VGPRs).  Where the per-tile single-pass
//    3-term screen of fp32 rows would run and the call brings a pair table, its 2-term pairwise form runs
//    instead (one MFMA of three dropped; screen_terms = 2 asks for it, RQSID_NO_PAIR=1 keeps 3 terms); a call
//    that asks for 2 terms where that form does not apply gets the 3-term screen.
//  * 16-bit rows take the per-tile form only, without the candidate split; variants that name another
//    screen are ignored for them.
//  * Defaults (variant 0): producer/consumer for the 1-term residual levels it covers (PROD level 2;
//    RQSID_PC=2 adds the 3-term ones, PROD level 1); row-resident for 1-term residual levels wider than 256
//    candidates (XL last level: 7.0 vs 14.8 ms); with RQSID_PC=0 the ping-pong streamed form for 1-term
//    256-candidate residual levels (L2 7.58 vs 7.92 ms); the per-tile kernel elsewhere.
//  * Per-tile: NT4 S2 runs 3 blocks/CU, NT8 S2 2 blocks/CU (independent blocks beat ring depth); segments
//    wider than one wave's tiles take the candidate split (CW = 2; 3-term <= 256 candidates, 1-term <= 512)
//    unless variant 7 or 2; anything wider is multi-pass.
inline AssignPlan plan_assign(const AssignShape& a, const AssignEnv& e) {
  AssignPlan pl;
  const int ccm = a.cand_count_max, rl = a.res_levels, variant = e.screen_variant;
  const bool x16 = a.x_format != kPlanXF32;
  const bool want3 = a.screen_terms == 3 || a.screen_terms == 2;
  const bool t3 = (ccm <= 128 && (want3 || (a.screen_terms == 0 && rl >= 1))) ||
                  (ccm <= 256 && (want3 || (a.screen_terms == 0 && rl == 1)));
  const bool legacy = variant == 2;
  pl.t3 = t3;
  pl.nt = t3 || ccm <= 128 ? 4 : 8;
  pl.half = a.dim <= kPlanHalfDim && !e.rescore_full;
  pl.rescreen = a.dim <= kPlanHalfDim && !e.no_rescreen && ccm > kPlanMaxList;

  // every persistent screen: fp32 rows, tile maps that fit their n_rows-int slots, den_out present whenever
  // the screen normalises a first-level residual
  const bool persistent_ok =
      !x16 && (int64_t)a.n_segments + 1 <= a.n_rows && (rl != 1 || !a.norm || a.has_den_out);
  const bool want_pc = variant == 9 || (variant == 0 && (e.pc >= 2 || (e.pc == 1 && !t3)));
  const bool want_rows = variant == 8 || (variant == 0 && rl >= 1 && ccm > 256);
  const int want_stream = variant == 5 ? (e.stream_shape == 42 || e.stream_shape == 88 ? e.stream_shape : 83)
                                       : (variant == 0 && pl.nt == 8 && !t3 && rl >= 1 ? 88 : 0);
  if (persistent_ok && want_pc && pc_supported(a.dim, ccm, t3, rl) &&
      pc_desc_bytes(a.n_rows, a.n_segments) <= a.n_rows * kPlanDescBytesPerRow) {
    pl.screen = AssignPlan::kPc;
    pl.nt = t3 ? 4 : 8;
    pl.pc_wide = !t3 && e.pcw == 1;
    pl.compact = true;
  } else if (persistent_ok && want_rows && rows_supported(a.dim, ccm, t3, rl, a.norm)) {
    pl.screen = AssignPlan::kRows;
    pl.rows_shape = e.rows_shape == 482 || e.rows_shape == 883 ? e.rows_shape : 443;
  } else if (persistent_ok && variant == 6 && resident_supported(a.dim, ccm, t3)) {
    pl.screen = AssignPlan::kResident;
    pl.compact = pl.expand = pl.read_err_word = true;
    pl.force_cap = e.test_force_spin_cap != 0;
  } else if (persistent_ok && want_stream && a.dim == kPlanStreamDim && ccm <= 256 && !a.has_cand_lid &&
             a.n_rows >= kPlanStreamMinRows && stream_supported(pl.nt, t3, rl)) {
    pl.screen = AssignPlan::kStream;
    pl.stream_shape = want_stream;
    pl.compact = true;
  } else {
    const bool split = !x16 && !legacy && variant != 7 && a.dim <= kPlanSplitDim;
    const int one_pass = pl.nt * 32;  // candidates one wave's tiles cover
    if (ccm <= one_pass) {
      pl.one = !legacy;
      pl.pair = t3 && pl.one && !x16 && a.has_pair && !e.no_pair && a.screen_terms != 3;
    } else if (ccm <= 2 * one_pass && split) {
      pl.one = true;
      pl.cw = 2;
      pl.s = kSplitS;
    }
  }
  return pl;
}

}  // namespace rqsid
