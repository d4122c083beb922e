// auction_plan.h — which form of the segmented auction's rounds runs (sweep only, one-block bid lists, multi-block
// bid lists, the row-sharded lists) and where every area of its workspace lies, as a pure function of the call's
// shape and of the RQSID_* switches.  Host-only and self-contained: no HIP header, no getenv (the caller reads
// the environment once per ABI call, read_auction_env in auction_seg.hip), plain C++17, so
// tests/test_auction_plan.py builds it with g++ and checks the table without a GPU.  auction_seg.hip ties its own
// constants to the ones below with static_asserts.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>

namespace rqsid {

constexpr int kPlanCh = 1024;            // kCh: jobs per chunk
constexpr int kPlanKG = 16;              // kKG: workers per block of a sweep
constexpr int kPlanAbovePad = 32;        // kAbovePad: u32 per worker in the padded per-worker counters
constexpr int kPlanRd = 16;              // kRd: first-level arrival counters of the fused round end
constexpr int kPlanMCH = 2048;           // kMCH: list entries per block of a multi-block list round
constexpr int kPlanListEq = 2048;        // kListEq: equal-to-T values a multi-block list round ranks
constexpr int kPlanLE = 4;               // kLE: list entries per thread a one-block list round keeps in registers
constexpr int kPlanLT = 1024;            // kLT: threads of a list-round block (256 for short lists: list_threads)
constexpr int64_t kPlanListMaxJpw = 16384;   // kListMaxJpw: one-block lists up to this many jobs per worker and segment
constexpr int64_t kPlanListBlockJpw = 8192;  // kListBlockJpw: one wide segment above it takes multi-block lists
constexpr int kPlanListStart = 32;       // kListStart: first round that builds lists ...
constexpr int kPlanListStartWide = 16;   // kListStartWide: ... at K >= kPlanListWideK
constexpr int kPlanListWideK = 1024;     // kListWideK
constexpr int kPlanListDelta = 32;       // kListDelta: keys below last round's threshold a list keeps
constexpr int kPlanPoll = 8;             // kPoll: rounds per captured block
constexpr int kPlanListLastRound = 1000; // the leftover rounds (> 1000) bid on unlisted pairs: they sweep
constexpr int64_t kPlanDHeader = 512;    // kDHeader: the row-sharded workspace's header

// entries of one worker's list in a segment of n_s jobs, and whether a one-block list round of `threads` threads
// keeps such a list in registers (constexpr: the kernels use the same two rules)
constexpr int64_t list_capacity(int64_t n_s, int32_t n_workers) { return 4 * (n_s / n_workers) + 256; }
constexpr bool list_in_registers(int64_t cap, int threads) { return cap <= (int64_t)kPlanLE * threads; }

// every switch the segmented and the row-sharded auction read, as the environment gives it (atoi of the variable;
// the default where it is not set); plan_auction applies the clamps
struct AuctionEnv {
  static constexpr int kUnset = INT_MIN;
  int auction_list = 1;    // RQSID_AUCTION_LIST: 0 sweep only (A/B, the tests' reference path); 1 lists; 2 one-block
                           // lists at any size
  int64_t list_mb_jpw = kPlanListBlockJpw;  // RQSID_LIST_MB_JPW (A/B): jobs per worker above which one wide segment's
                           // lists go multi-block; >= 1
  int list_js = 1;         // RQSID_LIST_JS=0: the list rounds gather winner and cost from two arrays (A/B)
  int list_start = kUnset; // RQSID_LIST_START: first round that builds lists, >= 1 (default 32, 16 at K >= 1024)
  int list_delta = kPlanListDelta;  // RQSID_LIST_DELTA: 1..128
  int list_stats = 0;      // RQSID_LIST_STATS=1: list verdict counts, printed to stderr at the end of the auction
  int dauction_list = 1;   // RQSID_DAUCTION_LIST=0: every row-sharded round sweeps (A/B)
  int list_block = 32;     // RQSID_LIST_BLOCK: list-only rounds per captured block, kPlanPoll..256
  int list_small = 1;      // RQSID_LIST_SMALL: 0 always 1024-thread list blocks; n > 1: 256 threads up to capacity n
  int list_only = 1;       // RQSID_LIST_ONLY=0: no list-only blocks (A/B)
};

// guess: the single-process entries (guessed pass, lean blocks, lists); sharded: the rqsid_dauction_* entries, where
// n_jobs is the rank's share, n_seg = n_multi = 1 and guess is off
struct AuctionShape {
  int64_t n_jobs = 0;
  int32_t n_workers = 1;
  int32_t n_seg = 1;
  int64_t total_chunks = 0;
  int32_t n_multi = 0;
  bool guess = true;
  bool sharded = false;
};

struct AuctionPlan {
  bool lists = false;        // multi-chunk segments keep bid lists
  bool multi_block = false;  // ... walked by lmb_chunks blocks per worker (sa_mlist_*), else one block per worker
  int32_t lmb_chunks = 0;
  bool js = false;           // packed {winner, cost} word per job for the list rounds
  int32_t lstart = kPlanListStart;
  int32_t ldelta = kPlanListDelta;
  bool stats = false;
  bool rdone = false;        // the last resolve block ends the round (one segment, more than one chunk)
  // row-sharded lists: entries per worker on one rank, blocks per worker of a list pass, lists on at all
  int64_t dcap = 0;
  int32_t dnb = 0;
  bool dlist_on = false;
  // list-only blocks (list pass, resolve, round end): allowed at all, and their rounds per captured block
  bool list_only = false;
  int32_t list_block_rounds = 32;
  int64_t list_small_cap = 1024;  // (0: never) capacity up to which every list block takes 256 threads

  // threads of a one-block list round, from the largest list capacity of the call (known after the init readback)
  int list_threads(int64_t lcap_max) const { return list_small_cap && lcap_max <= list_small_cap ? 256 : kPlanLT; }

  // The block of rounds after `done` rounds, when every list held through the previous block: a captured list-only
  // block of list_block_rounds rounds while one fits the round limit and ends by round 1000 (a block that reaches
  // the leftover rounds fails and is replayed in full); the rounds up to 1000 that no whole block fits run
  // list-only by direct launches (tail); after that, and when the round limit is nearer, ordinary blocks.
  struct ListBlock {
    bool graph = false, tail = false;
    int32_t rounds = 0;
  };
  ListBlock next_list_block(int32_t done, int32_t max_rounds) const {
    ListBlock b;
    if (!list_only || (max_rounds > 0 && max_rounds - done < list_block_rounds)) return b;
    const int32_t last = kPlanListLastRound + 1;
    if (done + list_block_rounds <= last) {
      b.graph = true;
      b.rounds = list_block_rounds;
    } else if (done < last && (max_rounds <= 0 || max_rounds - done >= last - done)) {
      b.tail = true;
      b.rounds = last - done;
    }
    return b;
  }
};

inline AuctionPlan plan_auction(const AuctionShape& s, const AuctionEnv& e) {
  AuctionPlan p;
  const int64_t N = s.n_jobs, K = s.n_workers, nm = s.n_multi > 0 ? s.n_multi : 1;
  // one wide segment with long lists: the multi-block list rounds (any jobs per worker); otherwise one block per
  // worker, only while the lists are short enough for it: at ~80k jobs per worker (K=128 over 10M rows) the
  // one-block-per-worker list round lost to the sweep (10M PROD training, level 1: 23 -> 33 s)
  p.multi_block = s.guess && s.n_multi == 1 && e.auction_list == 1 && N / K > std::max<int64_t>(1, e.list_mb_jpw);
  p.lists = s.guess && s.n_multi > 0 && e.auction_list != 0 &&
            (e.auction_list == 2 || p.multi_block || N / (nm * K) <= kPlanListMaxJpw);
  p.lmb_chunks = p.multi_block ? (int32_t)((list_capacity(N, s.n_workers) + kPlanMCH - 1) / kPlanMCH) : 0;
  p.js = p.lists && K <= 65535 && e.list_js != 0;  // (the packed word's winner is 16 bits)
  p.lstart = e.list_start != AuctionEnv::kUnset ? std::max(1, e.list_start)
                                                : K >= kPlanListWideK ? kPlanListStartWide : kPlanListStart;
  p.ldelta = std::min(128, std::max(1, e.list_delta));
  p.stats = p.lists && e.list_stats != 0;
  p.rdone = s.guess && s.n_seg == 1 && s.n_multi == 1;
  if (s.sharded) {  // one rank's share: 8 * (N / K) + 256 entries per worker
    p.dcap = 8 * (N / K) + 256;
    p.dnb = (int32_t)std::max<int64_t>(1, (list_capacity(N, s.n_workers) + kPlanMCH - 1) / kPlanMCH);
    p.dlist_on = e.dauction_list != 0;
  }
  p.list_only = p.lists && s.n_multi == s.n_seg && e.list_only != 0;  // (one-chunk segments have no lists)
  p.list_block_rounds = std::min(256, std::max(kPlanPoll, e.list_block));
  // short lists take 256-thread list-round blocks: capacity <= 4096 entries in every segment when there are many
  // segments (S x K blocks per round), <= 1024 for one segment (a 100k x 128 auction, capacity 3380, ran
  // 0.0194 -> 0.0207 ms per round with 256 threads; K=1280 x 100k, capacity 568, 0.0295 -> 0.0253)
  p.list_small_cap = e.list_small == 0 ? 0 : e.list_small > 1 ? e.list_small : s.n_multi > 1 ? 4096 : 1024;
  return p;
}

// Every area of the workspace in layout order: X(map field, SegAuction member, bytes per element, elements, present).
// S, K, N, C (chunks), M (n_multi), nm (max(M, 1)), MK (nm * K), guess, snap and p (the plan) are the map
// constructor's.  Each present area is rounded up to 256 B; an absent one has offset -1 (a null pointer in
// SegAuction).  The row-sharded entries (guess off) have none of the single-process list areas and take their own
// six at the end, which is why lst .. lsel appear twice.
#define RQSID_AUCTION_AREAS(X)                                                       \
  X(flag, flag, 1, S, true)                                                          \
  X(eps, eps, 2, S, true)                                                            \
  X(mm, mm, 4, 2 * S, true)                                                          \
  X(have, have, 4, S, true)                                                          \
  X(live_count, live_count, 4, 4, true)                                              \
  X(round_dev, round_dev, 4, 1, true)                                                \
  X(hidx, hidx, 4, S, true)                                                          \
  X(mseg, mseg, 4, nm, true)                                                         \
  X(cost, cost, 2, N, true)                                                          \
  X(hb, hb, 4, N, true)                                                              \
  X(nobid, nobid, 1, N, true)                                                        \
  X(key, key, 4, N, true)                                                            \
  X(hist, hist, 4, M * K * 256 + (sharded ? 64 : 0), true) /* (+ the list failure count) */ \
  X(sel, sel, 4, S * K * 4, true)                                                    \
  X(eqcnt, eqcnt, 4, K * C, true)                                                    \
  X(eqtot, eqtot, 4, S * K, true)                                                    \
  X(above, above, 4, M * K * kPlanAbovePad, guess)                                   \
  X(miss, miss, 1, M * K, guess)                                                     \
  X(chist, chist, 2, C * K * 256, snap)                                              \
  X(any_miss, any_miss, 4, 1, guess)                                                 \
  X(s_cost, s_cost, 2, N, snap)                                                      \
  X(s_hb, s_hb, 4, N, snap)                                                          \
  X(s_nobid, s_nobid, 1, N, snap)                                                    \
  X(s_out, s_out, 4, N, snap)                                                        \
  X(s_sel, s_sel, 4, S * K * 4 + 1, snap) /* (+ the round number) */                 \
  X(s_flag, s_flag, 1, S, snap)                                                      \
  X(s_rounds, s_rounds, 4, S, snap)                                                  \
  X(lh, lh, 4, MK * 512, p.multi_block)                                              \
  X(lsel, lsel, 4, MK * 4, p.multi_block)                                            \
  X(leq, leq, 4, MK * kPlanListEq, p.multi_block)                                    \
  X(leqn, leqn, 4, MK, p.multi_block)                                                \
  X(lok, lok, 1, MK, p.multi_block)                                                  \
  X(lst, lst, 8, 4 * N + 256 * MK, p.lists) /* segment s: K * (4 * (N_s / K) + 256) <= 4 N_s + 256 K entries */ \
  X(lcnt, lcnt, 4, MK * kPlanAbovePad, p.lists)                                      \
  X(lkb, lkb, 4, MK, p.lists)                                                        \
  X(lbad, lbad, 1, MK, p.lists)                                                      \
  X(loff, loff, 8, nm, p.lists)                                                      \
  X(lcs, lcs, 4, nm, p.lists)                                                        \
  X(lany, lany, 4, 1, p.lists)                                                       \
  X(js, js, 4, N, p.js)                                                              \
  X(rdone, rdone, 8, 16 * (1 + kPlanRd), p.rdone)                                    \
  X(lstat, lstat, 4, 8, p.stats)                                                     \
  X(d_lst, lst, 8, p.dcap * K, sharded)                                              \
  X(d_lcnt, lcnt, 4, K * kPlanAbovePad, sharded)                                     \
  X(d_lkb, lkb, 4, K, sharded)                                                       \
  X(d_lbad, lbad, 1, K, sharded)                                                     \
  X(d_lany, lany, 4, 1, sharded)                                                     \
  X(d_lsel, lsel, 4, K * 4, sharded)

// Byte offsets from the start of the workspace.  The row-sharded workspace opens with a kPlanDHeader-byte header:
// the one segment's job and chunk tables, its round count and the slot mode words {mode, sweep-slot flag}; the
// second word is that mode's any_miss (the sweep kernels exit unless it is set).
struct AuctionWorkspaceMap {
  int64_t seg_off = -1, chunk_off = -1, rounds = -1, dmode = -1;
#define RQSID_X(name, field, bytes, count, present) int64_t name = -1;
  RQSID_AUCTION_AREAS(RQSID_X)
#undef RQSID_X
  int64_t total_bytes = 0;

  AuctionWorkspaceMap(const AuctionShape& s, const AuctionPlan& p) {
    const int64_t S = s.n_seg, K = s.n_workers, N = s.n_jobs, C = s.total_chunks, M = s.n_multi;
    const int64_t nm = M > 0 ? M : 1, MK = nm * K;
    const bool guess = s.guess, sharded = s.sharded, snap = guess && M > 0;
    int64_t used = 0;
    if (sharded) {
      seg_off = 0;
      chunk_off = 64;
      rounds = 128;
      dmode = 192;
      used = kPlanDHeader;
    }
#define RQSID_X(name, field, bytes, count, present) \
  if (present) {                                     \
    name = used;                                     \
    used += ((count) * (bytes) + 255) / 256 * 256;   \
  }
    RQSID_AUCTION_AREAS(RQSID_X)
#undef RQSID_X
    if (sharded) any_miss = dmode + 4;
    total_bytes = used;
  }
};

}  // namespace rqsid
