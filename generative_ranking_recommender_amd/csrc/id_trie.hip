// id_trie.hip — the ID trie and its two consumers.
//
//   rqsid_id_trie         the trie tables from rqsid_id_cells's cells: the cells arrive in lexicographic ID order, so a
//                         depth-d node is a run of cells with the same d-prefix: head flags, scans, scatters.
//   rqsid_trie_mask       ConstrainedLogitsProcessor.__call__ for a batch: a walk kernel (one wave per row) finds each
//                         row's prefix and node, a mask kernel (one block per slice of a row) writes -inf everywhere but
//                         on the allowed tokens.
//   rqsid_trie_beam_step  one constrained beam step over trie nodes: one block per batch row.
//
// The build: flag kernel (a kept, in-range, ascending cell) -> scan -> compaction of the kept cells' IDs into the
// workspace -> head kernel (bit d - 1 of a byte: the cell starts a depth-d node) -> one scan of all depths' bits at
// once (8 channels) -> emit kernel (value, child_off, leaf_cell).  A scan is three launches: per-tile sums (2048 cells
// a block), one block over the tile sums (a run of tiles per thread, any number of them), and the pass that uses
// them.  Every grid is sized by n_cells; the number of kept cells stays on the device.
// Safety: a write position is a scan of flags this file computed, compared with the capacity before it is used; the
// consumers compare every node, child offset, value, token and level_tok entry with its table's size before it
// indexes anything.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace rqsid {
namespace {

constexpr int kTrieHeader = 256;   // workspace header: error word, counters / totals
constexpr int kTrieTile = 2048;    // cells per block of the scans: 256 threads x 8 flag bytes
constexpr int kTrieCh = RQSID_TRIE_LEVELS_MAX;  // channels of a scan: one per depth
constexpr int kMaskSlice = 8192;   // elements of a row per block of the mask kernel (an LDS bitmap of 1 KiB)
constexpr int64_t kTrieGroupsMax = int64_t(1) << 24;
constexpr uint32_t kTrieErrCell = 1u;                      // rqsid_id_trie
constexpr uint32_t kMaskErrRange = 1u, kMaskErrTok = 2u;   // rqsid_trie_mask
static_assert(kTrieCh == 8, "a flag byte holds one bit per depth");

// the levels, checked on the host; passed by value
struct TrieShape {
  int32_t levels;
  int32_t sizes[kTrieCh];
  int32_t div[kTrieCh + 1];  // depth d < levels (levels > 1): group / div[d] is the d-prefix
  int32_t tok_off[kTrieCh];  // first level_tok entry of each level
  int32_t groups;            // product of the group levels' sizes
  int32_t n_fine;            // the last level's size (1 with one level)
};

struct TrieTables {
  int64_t cap;  // entries per depth in value (cap + 1 in child_off)
  const int32_t *count, *value, *child_off;
  TrieShape sh;
};

int trie_shape(const char* who, int32_t levels, const int32_t* sizes, TrieShape& sh) {
  if (levels < 1 || levels > RQSID_TRIE_LEVELS_MAX)
    return fail(RQSID_E_ARG, "%s: levels = %d outside [1, %d]", who, levels, RQSID_TRIE_LEVELS_MAX);
  if (!sizes) return fail(RQSID_E_ARG, "%s: sizes is required", who);
  sh = TrieShape{};
  sh.levels = levels;
  int64_t groups = 1, off = 0;
  const int gl = levels > 1 ? levels - 1 : 1;
  for (int l = 0; l < levels; ++l) {
    if (sizes[l] < 1) return fail(RQSID_E_ARG, "%s: sizes[%d] = %d is not positive", who, l, sizes[l]);
    sh.sizes[l] = sizes[l];
    sh.tok_off[l] = (int32_t)off;
    off += sizes[l];
    if (l < gl) {
      groups *= sizes[l];
      if (groups > kTrieGroupsMax)
        return fail(RQSID_E_ARG, "%s: the sizes of every level but the last multiply to more than 2^24", who);
    }
  }
  sh.n_fine = levels > 1 ? sizes[levels - 1] : 1;
  if (sh.n_fine > RQSID_CELLS_FINE_MAX)
    return fail(RQSID_E_ARG, "%s: the last level's size %d exceeds %d", who, sh.n_fine, RQSID_CELLS_FINE_MAX);
  sh.groups = (int32_t)groups;
  int64_t d = 1;
  for (int l = gl; l >= 0; --l) {  // div[l] = product of sizes[l .. gl)
    sh.div[l] = (int32_t)d;
    if (l > 0) d *= sizes[l - 1];
  }
  return RQSID_OK;
}

// the level-(d - 1) value of a cell's ID
__device__ __forceinline__ int32_t trie_level_value(const TrieShape& sh, int d, int32_t g, int32_t f) {
  if (sh.levels == 1) return g;
  if (d == sh.levels) return f;
  return (g / sh.div[d]) % sh.sizes[d - 1];
}

// ---------------------------------------------------------------------------------------------------------------
// scans

// exclusive scan over the block's threads of 8 counters each: in-wave by shuffles, across waves through LDS
template <int NW>
__device__ __forceinline__ void trie_block_scan(const int32_t (&v)[kTrieCh], int32_t (&excl)[kTrieCh],
                                                int32_t (&tot)[kTrieCh], int32_t (*wsum)[kTrieCh], int t) {
  const int lane = t & 63, w = t >> 6;
  int32_t inc[kTrieCh];
#pragma unroll
  for (int c = 0; c < kTrieCh; ++c) {
    int32_t a = v[c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t up = __shfl_up(a, o);
      if (lane >= o) a += up;
    }
    inc[c] = a;
  }
  __syncthreads();  // (wsum may still be read from an earlier call)
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < kTrieCh; ++c) wsum[w][c] = inc[c];
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < kTrieCh; ++c) {
    int32_t before = 0, all = 0;
    for (int k = 0; k < NW; ++k) {
      const int32_t s = wsum[k][c];
      before += k < w ? s : 0;
      all += s;
    }
    excl[c] = before + inc[c] - v[c];
    tot[c] = all;
  }
}

// the 8 flag bytes of a thread's cells, counted per bit
__device__ __forceinline__ void trie_count_bits(uint64_t word, int32_t (&cnt)[kTrieCh]) {
#pragma unroll
  for (int c = 0; c < kTrieCh; ++c) cnt[c] = __popcll((word >> c) & 0x0101010101010101ull);
}

// per tile: the number of set bits of each channel
__global__ __launch_bounds__(256) void trie_tile_sums_kernel(const uint8_t* __restrict__ bits,
                                                             int32_t* __restrict__ tile_sums) {
  __shared__ int32_t wsum[4][kTrieCh];
  const int t = threadIdx.x;
  const uint64_t word = *reinterpret_cast<const uint64_t*>(bits + (int64_t)blockIdx.x * kTrieTile + t * 8);
  int32_t cnt[kTrieCh], excl[kTrieCh], tot[kTrieCh];
  trie_count_bits(word, cnt);
  trie_block_scan<4>(cnt, excl, tot, wsum, t);
  if (t == 0) {
#pragma unroll
    for (int c = 0; c < kTrieCh; ++c) tile_sums[(int64_t)blockIdx.x * kTrieCh + c] = tot[c];
  }
}

struct TrieBuild {
  int64_t n, cap;
  const int32_t *cell_group, *cell_fine;
  const uint8_t* keep;
  int32_t *count, *value, *child_off, *leaf_cell;
  uint32_t* err;       // workspace [0, 4)
  int32_t* kept;       // workspace [16, 20): the number of kept cells
  uint8_t* bits;       // [tiles * kTrieTile]
  int32_t *kg, *kf, *kidx;  // [n] the kept cells' group, fine ID and cell number, compacted
  int32_t* tile_sums;  // [tiles][kTrieCh]
  int32_t tiles;
  TrieShape sh;
};

// one block: exclusive scan of the tile sums in place, every channel at once (a run of tiles per thread).  final = 0:
// the total of channel 0 is the number of kept cells; final = 1: the totals are the node counts, written with the
// root's entries and each depth's closing child_off.
__global__ __launch_bounds__(1024) void trie_scan_tiles_kernel(TrieBuild p, int final_pass) {
  __shared__ int32_t wsum[16][kTrieCh];
  const int t = threadIdx.x;
  const int run = (p.tiles + 1023) / 1024;
  const int64_t k0l = (int64_t)t * run;
  const int k0 = k0l < p.tiles ? (int)k0l : p.tiles, k1 = k0 + run < p.tiles ? k0 + run : p.tiles;
  int32_t a[kTrieCh], excl[kTrieCh], tot[kTrieCh];
#pragma unroll
  for (int c = 0; c < kTrieCh; ++c) a[c] = 0;
  for (int k = k0; k < k1; ++k) {
#pragma unroll
    for (int c = 0; c < kTrieCh; ++c) a[c] += p.tile_sums[(int64_t)k * kTrieCh + c];
  }
  trie_block_scan<16>(a, excl, tot, wsum, t);
  for (int k = k0; k < k1; ++k) {
#pragma unroll
    for (int c = 0; c < kTrieCh; ++c) {
      const int32_t s = p.tile_sums[(int64_t)k * kTrieCh + c];
      p.tile_sums[(int64_t)k * kTrieCh + c] = excl[c];
      excl[c] += s;
    }
  }
  if (t != 0) return;
  if (!final_pass) {
    *p.kept = tot[0];
    return;
  }
  const int L = p.sh.levels;
  p.count[0] = 1;
  p.child_off[0] = 0;
  int32_t prev = 1;  // nodes of the depth above
#pragma unroll
  for (int d = 1; d <= kTrieCh; ++d) {
    if (d > L) break;
    const int32_t cnt = tot[d - 1] < p.cap ? tot[d - 1] : (int32_t)p.cap;
    p.count[d] = cnt;
    p.child_off[(int64_t)(d - 1) * (p.cap + 1) + prev] = cnt;  // child_off[d - 1][count[d - 1]] = count[d]
    prev = cnt;
  }
}

// flag byte of each cell: 1 = in the trie (kept, inside sizes, above the cell before it)
__global__ __launch_bounds__(256) void trie_flag_kernel(TrieBuild p) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // < tiles * kTrieTile
  uint8_t v = 0;
  if (i < p.n) {
    const int32_t g = p.cell_group[i], f = p.cell_fine[i];
    bool ok = (uint32_t)g < (uint32_t)p.sh.groups && (uint32_t)f < (uint32_t)p.sh.n_fine;
    if (ok && i > 0) {
      const int32_t pg = p.cell_group[i - 1], pf = p.cell_fine[i - 1];
      if (pg > g || (pg == g && pf >= f)) ok = false;
    }
    if (!ok) atomicOr(p.err, kTrieErrCell);
    v = ok && (!p.keep || p.keep[i]);
  }
  p.bits[i] = v;
}

// the kept cells' IDs and numbers, compacted in order
__global__ __launch_bounds__(256) void trie_compact_kernel(TrieBuild p) {
  __shared__ int32_t wsum[4][kTrieCh];
  const int t = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * kTrieTile + t * 8;
  const uint64_t word = *reinterpret_cast<const uint64_t*>(p.bits + i0);
  int32_t cnt[kTrieCh], excl[kTrieCh], tot[kTrieCh];
  trie_count_bits(word, cnt);
  trie_block_scan<4>(cnt, excl, tot, wsum, t);
  int64_t pos = (int64_t)p.tile_sums[(int64_t)blockIdx.x * kTrieCh] + excl[0];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (!((word >> (8 * e)) & 1)) continue;
    const int64_t i = i0 + e;
    if (i < p.n && pos >= 0 && pos < p.n) {
      p.kg[pos] = p.cell_group[i];
      p.kf[pos] = p.cell_fine[i];
      p.kidx[pos] = (int32_t)i;
    }
    ++pos;
  }
}

// flag byte of each kept cell: bit d - 1 = its d-prefix differs from the kept cell before it
__global__ __launch_bounds__(256) void trie_head_kernel(TrieBuild p) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t m = *p.kept;
  if (m > p.n) m = p.n;
  uint32_t v = 0;
  if (j < m) {
    const int L = p.sh.levels;
    const int32_t g = p.kg[j], f = p.kf[j];
    if (j == 0) {
      v = (1u << L) - 1u;
    } else {
      const int32_t pg = p.kg[j - 1], pf = p.kf[j - 1];
      if (L == 1) {
        v = pg != g;
      } else {
#pragma unroll
        for (int d = 1; d < kTrieCh; ++d)
          if (d < L && pg / p.sh.div[d] != g / p.sh.div[d]) v |= 1u << (d - 1);
        if (pg != g || pf != f) v |= 1u << (L - 1);
      }
    }
  }
  p.bits[j] = (uint8_t)v;
}

// the tables: a kept cell that starts a depth-d node writes the node's value, its first child (the number the cell's
// depth-(d + 1) node gets: a cell that starts a node starts one at every deeper level) and, at the last depth, its cell
__global__ __launch_bounds__(256) void trie_emit_kernel(TrieBuild p) {
  __shared__ int32_t wsum[4][kTrieCh];
  const int t = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * kTrieTile + t * 8;
  const uint64_t word = *reinterpret_cast<const uint64_t*>(p.bits + j0);
  int32_t cnt[kTrieCh], r[kTrieCh], tot[kTrieCh];
  trie_count_bits(word, cnt);
  trie_block_scan<4>(cnt, r, tot, wsum, t);
#pragma unroll
  for (int c = 0; c < kTrieCh; ++c) r[c] += p.tile_sums[(int64_t)blockIdx.x * kTrieCh + c];
  const int L = p.sh.levels;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t byte = (uint32_t)(word >> (8 * e)) & 0xffu;
    const int64_t j = j0 + e;
    if (!byte || j >= p.n) continue;
    const int32_t g = p.kg[j], f = p.kf[j];
#pragma unroll
    for (int d = 1; d <= kTrieCh; ++d) {
      if (d > L || !((byte >> (d - 1)) & 1u)) continue;
      const int64_t node = r[d - 1];
      if (node < 0 || node >= p.cap) continue;
      p.value[(int64_t)(d - 1) * p.cap + node] = trie_level_value(p.sh, d, g, f);
      if (d == L) {
        p.leaf_cell[node] = p.kidx[j];
      } else {
        p.child_off[(int64_t)d * (p.cap + 1) + node] = r[d < kTrieCh ? d : 0];
      }
    }
#pragma unroll
    for (int c = 0; c < kTrieCh; ++c) r[c] += (byte >> c) & 1u;
  }
}

struct TriePlan {
  int64_t tiles, off_bits, off_kg, off_kf, off_kidx, off_sums, bytes;
};

inline TriePlan trie_plan(int64_t n) {
  TriePlan pl;
  pl.tiles = cdiv(n, kTrieTile);
  pl.off_bits = kTrieHeader;
  pl.off_kg = pl.off_bits + pl.tiles * kTrieTile;
  pl.off_kf = pl.off_kg + n * 4;
  pl.off_kidx = pl.off_kf + n * 4;
  pl.off_sums = pl.off_kidx + n * 4;
  pl.bytes = (pl.off_sums + pl.tiles * kTrieCh * 4 + 7) / 8 * 8;
  return pl;
}

int trie_check_cells(const char* who, int64_t n_cells, int32_t levels) {
  if (n_cells < 0 || n_cells >= (1ll << 31))
    return fail(RQSID_E_ARG, "%s: n_cells = %lld outside [0, 2^31)", who, (long long)n_cells);
  if (levels < 1 || levels > RQSID_TRIE_LEVELS_MAX)
    return fail(RQSID_E_ARG, "%s: levels = %d outside [1, %d]", who, levels, RQSID_TRIE_LEVELS_MAX);
  return RQSID_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// the consumers' view of the tables

// the child range of depth-d node `node` (d < levels), clamped into the depth below; false for no such node
__device__ __forceinline__ bool trie_children(const TrieTables& T, int d, int32_t node, int32_t& lo, int32_t& hi,
                                              uint32_t& errs) {
  int64_t cnt_d = 1;
  if (d > 0) {
    cnt_d = T.count[d];
    cnt_d = cnt_d < 0 ? 0 : (cnt_d > T.cap ? T.cap : cnt_d);
  }
  if (node < 0 || node >= cnt_d) return false;
  int64_t cnt_c = T.count[d + 1];
  cnt_c = cnt_c < 0 ? 0 : (cnt_c > T.cap ? T.cap : cnt_c);
  const int64_t a = T.child_off[(int64_t)d * (T.cap + 1) + node], b = T.child_off[(int64_t)d * (T.cap + 1) + node + 1];
  const int64_t l = a < 0 ? 0 : (a > cnt_c ? cnt_c : a), h = b < l ? l : (b > cnt_c ? cnt_c : b);
  if (l != a || h != b) errs |= kMaskErrRange;
  lo = (int32_t)l;
  hi = (int32_t)h;
  return true;
}

// the token of child c at depth d + 1 (level d), or -1; no address from an unchecked value
__device__ __forceinline__ int32_t trie_child_token(const TrieTables& T, int d, int32_t c,
                                                    const int32_t* __restrict__ level_tok, int32_t V, uint32_t& errs) {
  const int32_t val = T.value[(int64_t)d * T.cap + c];
  if ((uint32_t)val >= (uint32_t)T.sh.sizes[d]) return -1;
  const int32_t tk = level_tok[T.sh.tok_off[d] + val];
  if ((uint32_t)tk < (uint32_t)V) return tk;
  if (tk != -1) errs |= kMaskErrTok;
  return -1;
}

__device__ __forceinline__ int32_t wave_sum_i32(int32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct MaskParams {
  TrieTables T;
  const void* ids;
  int32_t ids_i64;
  int64_t B, ids_ld;
  int32_t T_len;
  void* scores;
  int32_t V;
  int64_t ld;
  const int32_t *tok_code, *level_tok;
  int32_t eos;
  int32_t *out_kind, *out_node, *out_count;
  uint32_t* err;     // workspace [0, 4)
  int32_t* ctr;      // workspace [4, 16): rows of kind 0, 1, 2
  int4* rowinfo;     // [B] kind, prefix length, child range
  int32_t slices;
  uint32_t ninf;     // -inf of the format (twice in a word for the 16-bit formats)
};

// tok_code of the token at position pos of row b, -1 for a token outside the vocabulary
__device__ __forceinline__ int32_t mask_code_at(const MaskParams& p, int64_t b, int32_t pos) {
  const int64_t at = b * p.ids_ld + pos;
  const int64_t tok = p.ids_i64 ? reinterpret_cast<const int64_t*>(p.ids)[at]
                                : (int64_t) reinterpret_cast<const int32_t*>(p.ids)[at];
  if (tok < 0 || tok >= p.V) return -1;
  return p.tok_code[tok];
}

// one wave per row: rules 1 - 4
__global__ __launch_bounds__(256) void trie_walk_kernel(MaskParams p) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= p.B) return;
  const TrieShape& sh = p.T.sh;
  const int L = sh.levels;
  uint32_t errs = 0;
  // the last level-0 token: 64 positions a step, from the end
  int32_t first = -1;
  for (int32_t base = p.T_len - 1; base >= 0 && first < 0; base -= 64) {
    const int32_t pos = base - lane;
    bool is0 = false;
    if (pos >= 0) {
      const int32_t code = mask_code_at(p, b, pos);
      is0 = code >= 0 && (code >> 24) == 0;
    }
    const unsigned long long m = __ballot(is0);
    if (m) first = base - (__ffsll((long long)m) - 1);
  }
  const int plen = first < 0 ? 0 : (p.T_len - first < L ? p.T_len - first : L);
  int32_t kind, node = -1, lo = 0, hi = 0, count = 0;
  if (plen == L) {
    kind = 1;
    for (int32_t v = lane; v < sh.sizes[0]; v += 64) {
      const int32_t tk = p.level_tok[v];
      if ((uint32_t)tk < (uint32_t)p.V) ++count; else if (tk != -1) errs |= kMaskErrTok;
    }
    count = wave_sum_i32(count);
    const int32_t ec = p.tok_code[p.eos];  // (eos was checked on the host)
    const bool dup = ec >= 0 && (ec >> 24) == 0 && (ec & 0xffffff) < sh.sizes[0] && p.level_tok[ec & 0xffffff] == p.eos;
    count += !dup;
  } else {
    bool ok = true;
    node = 0;
    for (int t = 0; t < plen && ok; ++t) {  // (wave-uniform)
      const int32_t code = mask_code_at(p, b, first + t);
      int32_t clo, chi;
      if (code < 0 || (code >> 24) != t || !trie_children(p.T, t, node, clo, chi, errs)) {
        ok = false;
        break;
      }
      const int32_t want = code & 0xffffff;
      const int32_t* vals = p.T.value + (int64_t)t * p.T.cap;
      int32_t l = clo, h = chi;
      while (l < h) {
        const int32_t mid = l + ((h - l) >> 1);
        if (vals[mid] < want) l = mid + 1; else h = mid;
      }
      if (l < chi && vals[l] == want) node = l; else ok = false;
    }
    if (ok && trie_children(p.T, plen, node, lo, hi, errs)) {
      for (int32_t c = lo + lane; c < hi; c += 64) count += trie_child_token(p.T, plen, c, p.level_tok, p.V, errs) >= 0;
      count = wave_sum_i32(count);
    }
    if (count > 0) {
      kind = 0;
    } else {
      kind = 2;
      node = -1;
      lo = hi = 0;
      count = 1;
    }
  }
  if (errs) atomicOr(p.err, errs);
  if (lane == 0) {
    p.rowinfo[b] = make_int4(kind, plen, lo, hi);
    atomicAdd(&p.ctr[kind], 1);
    if (p.out_kind) p.out_kind[b] = kind;
    if (p.out_node) p.out_node[b] = node;
    if (p.out_count) p.out_count[b] = count;
  }
}

// rule 5 for one slice of one row.  ES: bytes of an element
template <int ES>
__global__ __launch_bounds__(256) void trie_mask_kernel(MaskParams p) {
  constexpr int K = 16 / ES;  // elements of a 16-byte piece
  __shared__ uint32_t bm[kMaskSlice / 32 + 2];
  const int t = threadIdx.x;
  const int64_t b = blockIdx.x / p.slices;
  const int32_t s0 = (int32_t)(blockIdx.x % p.slices) * kMaskSlice;
  const int32_t s1 = s0 + kMaskSlice < p.V ? s0 + kMaskSlice : p.V;
  const int32_t n = s1 - s0;
  for (int w = t; w < kMaskSlice / 32 + 2; w += 256) bm[w] = 0u;
  __syncthreads();
  const int4 info = p.rowinfo[b];
  const TrieShape& sh = p.T.sh;
  uint32_t errs = 0;
  auto allow = [&](int32_t tk) {
    if (tk >= s0 && tk < s1) atomicOr(&bm[(tk - s0) >> 5], 1u << ((tk - s0) & 31));
  };
  if (info.x == 0 && info.y >= 0 && info.y < sh.levels) {
    const int64_t lo = info.z < 0 ? 0 : (info.z > p.T.cap ? p.T.cap : info.z);
    const int64_t hi = info.w < lo ? lo : (info.w > p.T.cap ? p.T.cap : info.w);
    for (int64_t c = lo + t; c < hi; c += 256) {
      const int32_t tk = trie_child_token(p.T, info.y, (int32_t)c, p.level_tok, p.V, errs);
      if (tk >= 0) allow(tk);
    }
  } else if (info.x == 1) {
    for (int32_t v = t; v < sh.sizes[0]; v += 256) {
      const int32_t tk = p.level_tok[v];
      if ((uint32_t)tk < (uint32_t)p.V) allow(tk);
    }
    if (t == 0) allow(p.eos);
  } else if (t == 0) {
    allow(p.eos);
  }
  __syncthreads();
  char* row = static_cast<char*>(p.scores) + (b * p.ld + s0) * ES;
  const int32_t head_want = (int32_t)(((16 - (reinterpret_cast<uintptr_t>(row) & 15)) & 15) / ES);
  const int32_t head = head_want < n ? head_want : n;
  const int32_t nvec = (n - head) / K, tail = head + nvec * K;
  auto bit = [&](int32_t e) { return (bm[e >> 5] >> (e & 31)) & 1u; };
  auto store_elem = [&](int32_t e) {
    if (ES == 4) reinterpret_cast<uint32_t*>(row)[e] = p.ninf;
    else reinterpret_cast<uint16_t*>(row)[e] = (uint16_t)p.ninf;
  };
  for (int32_t e = t; e < head; e += 256)
    if (!bit(e)) store_elem(e);
  for (int32_t e = tail + t; e < n; e += 256)
    if (!bit(e)) store_elem(e);
  const uint4 all_ninf = make_uint4(p.ninf, p.ninf, p.ninf, p.ninf);
  for (int32_t q = t; q < nvec; q += 256) {
    const int32_t e = head + q * K;
    const uint64_t two = (uint64_t)bm[e >> 5] | ((uint64_t)bm[(e >> 5) + 1] << 32);
    const uint32_t bits = (uint32_t)(two >> (e & 31)) & ((1u << K) - 1u);
    if (bits == (1u << K) - 1u) continue;  // every element keeps its bytes
    uint4* ptr = reinterpret_cast<uint4*>(row + (int64_t)e * ES);
    if (bits == 0u) {
      *ptr = all_ninf;  // no allowed token: stored without being read
      continue;
    }
    uint4 v = *ptr;
    uint32_t* w = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t keep;
      if (ES == 4) keep = ((bits >> k) & 1u) ? 0xffffffffu : 0u;
      else keep = (((bits >> (2 * k)) & 1u) ? 0x0000ffffu : 0u) | (((bits >> (2 * k + 1)) & 1u) ? 0xffff0000u : 0u);
      w[k] = (w[k] & keep) | (p.ninf & ~keep);
    }
    *ptr = v;
  }
  if (errs) atomicOr(p.err, errs);
}

// ---------------------------------------------------------------------------------------------------------------
// beam step

struct BeamStepParams {
  TrieTables T;
  int32_t depth, beam_in, beam_out;
  const int32_t* node_in;
  const float* score_in;
  const void* logp;
  int32_t x_format, V;
  int64_t ld;
  const int32_t* level_tok;
  int32_t* node_out;
  float* score_out;
  int32_t *parent_out, *value_out, *token_out;
};

__device__ __forceinline__ float beam_load(const void* x, int32_t fmt, int64_t at) {
  if (fmt == RQSID_X_F32) return reinterpret_cast<const float*>(x)[at];
  const uint16_t h = reinterpret_cast<const uint16_t*>(x)[at];
  if (fmt == RQSID_X_F16) return (float)__builtin_bit_cast(_Float16, h);
  return __uint_as_float((uint32_t)h << 16);
}

// a live score's place in ascending order, never 0 (-0 taken as +0)
__device__ __forceinline__ uint32_t beam_ord(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One block per batch row.  Every candidate has its own 64-bit key (score order above the inverted (h, child rank)),
// so "the first beam_out in (s descending, h ascending, value ascending)" is beam_out extractions of the largest key.
// Each thread holds the largest key of its own candidates; a round finds the block's largest, and only the thread that
// owned it looks through its candidates again, for its largest key below the one just taken.
__global__ __launch_bounds__(256) void trie_beam_kernel(BeamStepParams p) {
  __shared__ int32_t hlo[RQSID_TRIE_BEAM_MAX], hn[RQSID_TRIE_BEAM_MAX];
  __shared__ float hs[RQSID_TRIE_BEAM_MAX];
  __shared__ uint64_t wmax[4];
  const int t = threadIdx.x, d = p.depth;
  const int64_t b = blockIdx.x;
  if (t < p.beam_in) {
    const int32_t node = p.node_in[b * p.beam_in + t];
    const float sc = p.score_in ? p.score_in[b * p.beam_in + t] : 0.0f;
    int32_t lo = 0, hi = 0;
    uint32_t errs = 0;
    const bool ok = sc == sc && trie_children(p.T, d, node, lo, hi, errs);
    hlo[t] = ok ? lo : 0;
    hn[t] = ok ? (hi - lo < (1 << 24) ? hi - lo : (1 << 24)) : 0;
    hs[t] = sc;
  }
  __syncthreads();
  struct Cand {
    int32_t c, val, tk;
    float s;
  };
  auto cand = [&](int h, int32_t j, Cand& o) -> uint64_t {
    uint32_t errs = 0;
    o.c = hlo[h] + j;
    o.val = p.T.value[(int64_t)d * p.T.cap + o.c];
    o.tk = trie_child_token(p.T, d, o.c, p.level_tok, p.V, errs);
    if (o.tk < 0) return 0ull;
    o.s = hs[h] + beam_load(p.logp, p.x_format, (b * p.beam_in + h) * p.ld + o.tk);
    if (!(o.s == o.s) || o.s == -__builtin_inff()) return 0ull;
    return ((uint64_t)beam_ord(o.s) << 32) | (uint64_t)(0x3fffffffu - (((uint32_t)h << 24) | (uint32_t)j));
  };
  auto best_below = [&](uint64_t limit) {
    uint64_t best = 0ull;
    Cand o;
    for (int h = 0; h < p.beam_in; ++h)
      for (int32_t j = t; j < hn[h]; j += 256) {
        const uint64_t k = cand(h, j, o);
        if (k < limit && k > best) best = k;
      }
    return best;
  };
  uint64_t mine = best_below(~0ull);
  int r = 0;
  for (; r < p.beam_out; ++r) {
    uint64_t m = mine;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t lo32 = __shfl_xor((uint32_t)m, o), hi32 = __shfl_xor((uint32_t)(m >> 32), o);
      const uint64_t other = ((uint64_t)hi32 << 32) | lo32;
      m = other > m ? other : m;
    }
    if ((t & 63) == 0) wmax[t >> 6] = m;
    __syncthreads();
    uint64_t top = wmax[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) top = wmax[k] > top ? wmax[k] : top;
    if (top == 0ull) break;  // (block-uniform)
    if (mine == top) {       // keys are distinct: one thread
      const uint32_t low = 0x3fffffffu - (uint32_t)(top & 0xffffffffu);
      const int h = (int)(low >> 24);
      const int32_t j = (int32_t)(low & 0xffffffu);
      Cand o;
      if (h < p.beam_in && j < hn[h] && cand(h, j, o) == top) {
        const int64_t at = b * p.beam_out + r;
        p.node_out[at] = o.c;
        p.score_out[at] = o.s;
        if (p.parent_out) p.parent_out[at] = h;
        if (p.value_out) p.value_out[at] = o.val;
        if (p.token_out) p.token_out[at] = o.tk;
      }
      mine = best_below(top);
    }
    __syncthreads();
  }
  for (int q = r + t; q < p.beam_out; q += 256) {
    const int64_t at = b * p.beam_out + q;
    p.node_out[at] = -1;
    p.score_out[at] = -__builtin_inff();
    if (p.parent_out) p.parent_out[at] = -1;
    if (p.value_out) p.value_out[at] = -1;
    if (p.token_out) p.token_out[at] = -1;
  }
}

int trie_tables(const char* who, int64_t cap, int32_t levels, const int32_t* sizes, const int32_t* count,
                const int32_t* value, const int32_t* child_off, TrieTables& T) {
  int rc;
  if ((rc = trie_shape(who, levels, sizes, T.sh))) return rc;
  if (cap < 0 || cap >= (1ll << 31)) return fail(RQSID_E_ARG, "%s: capacity = %lld outside [0, 2^31)", who, (long long)cap);
  T.cap = cap;
  T.count = count;
  T.value = value;
  T.child_off = child_off;
  return RQSID_OK;
}

int trie_check_format(const char* who, int32_t x_format) {
  if (x_format != RQSID_X_F32 && x_format != RQSID_X_F16 && x_format != RQSID_X_BF16)
    return fail(RQSID_E_ARG, "%s: x_format = %d is none of RQSID_X_F32 / F16 / BF16", who, x_format);
  return RQSID_OK;
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int64_t rqsid_id_trie_workspace_bytes(int64_t n_cells, int32_t levels) {
  int rc;
  if ((rc = trie_check_cells("rqsid_id_trie_workspace_bytes", n_cells, levels))) return rc;
  return trie_plan(n_cells).bytes;
}

int rqsid_id_trie(int64_t n_cells, const int32_t* cell_group, const int32_t* cell_fine, int32_t levels,
                  const int32_t* sizes, const uint8_t* keep, int32_t* count, int32_t* value, int32_t* child_off,
                  int32_t* leaf_cell, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "rqsid_id_trie";
  int rc;
  TrieBuild p{};
  if ((rc = trie_check_cells(who, n_cells, levels))) return rc;
  if ((rc = trie_shape(who, levels, sizes, p.sh))) return rc;
  if (n_cells == 0) return RQSID_OK;
  if (!cell_group || !cell_fine) return fail(RQSID_E_ARG, "%s: cell_group and cell_fine are required", who);
  if (!count || !value || !child_off || !leaf_cell) return fail(RQSID_E_ARG, "%s: every output is required", who);
  const TriePlan pl = trie_plan(n_cells);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes,
                (long long)pl.bytes);
  char* ws = static_cast<char*>(workspace);
  p.n = p.cap = n_cells;
  p.cell_group = cell_group;
  p.cell_fine = cell_fine;
  p.keep = keep;
  p.count = count;
  p.value = value;
  p.child_off = child_off;
  p.leaf_cell = leaf_cell;
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.kept = reinterpret_cast<int32_t*>(ws + 16);
  p.bits = reinterpret_cast<uint8_t*>(ws + pl.off_bits);
  p.kg = reinterpret_cast<int32_t*>(ws + pl.off_kg);
  p.kf = reinterpret_cast<int32_t*>(ws + pl.off_kf);
  p.kidx = reinterpret_cast<int32_t*>(ws + pl.off_kidx);
  p.tile_sums = reinterpret_cast<int32_t*>(ws + pl.off_sums);
  p.tiles = (int32_t)pl.tiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 per_cell((unsigned)(pl.tiles * (kTrieTile / 256))), per_tile((unsigned)pl.tiles);
  hipLaunchKernelGGL(trie_flag_kernel, per_cell, dim3(256), 0, st, p);
  hipLaunchKernelGGL(trie_tile_sums_kernel, per_tile, dim3(256), 0, st, p.bits, p.tile_sums);
  hipLaunchKernelGGL(trie_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, p, 0);
  hipLaunchKernelGGL(trie_compact_kernel, per_tile, dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_id_trie (compact)"))) return rc;
  hipLaunchKernelGGL(trie_head_kernel, per_cell, dim3(256), 0, st, p);
  hipLaunchKernelGGL(trie_tile_sums_kernel, per_tile, dim3(256), 0, st, p.bits, p.tile_sums);
  hipLaunchKernelGGL(trie_scan_tiles_kernel, dim3(1), dim3(1024), 0, st, p, 1);
  hipLaunchKernelGGL(trie_emit_kernel, per_tile, dim3(256), 0, st, p);
  return check_launch("rqsid_id_trie (emit)");
}

int64_t rqsid_trie_mask_workspace_bytes(int64_t n_rows) {
  if (n_rows < 0 || n_rows >= (1ll << 31))
    return fail(RQSID_E_ARG, "rqsid_trie_mask_workspace_bytes: n_rows = %lld outside [0, 2^31)", (long long)n_rows);
  return kTrieHeader + n_rows * 16;
}

int rqsid_trie_mask(int64_t capacity, int32_t levels, const int32_t* sizes, const int32_t* count, const int32_t* value,
                    const int32_t* child_off, const void* input_ids, int32_t ids_format, int64_t n_rows,
                    int32_t n_tokens, int64_t ids_ld, void* scores, int32_t x_format, int32_t vocab, int64_t ld,
                    const int32_t* tok_code, const int32_t* level_tok, int32_t eos, int32_t* out_kind,
                    int32_t* out_node, int32_t* out_count, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "rqsid_trie_mask";
  int rc;
  MaskParams p{};
  if ((rc = trie_tables(who, capacity, levels, sizes, count, value, child_off, p.T))) return rc;
  if ((rc = trie_check_format(who, x_format))) return rc;
  if (ids_format != RQSID_IDS_I32 && ids_format != RQSID_IDS_I64)
    return fail(RQSID_E_ARG, "%s: ids_format = %d is neither RQSID_IDS_I32 nor RQSID_IDS_I64", who, ids_format);
  if (n_rows < 0 || n_rows >= (1ll << 31))
    return fail(RQSID_E_ARG, "%s: n_rows = %lld outside [0, 2^31)", who, (long long)n_rows);
  if (n_tokens < 0) return fail(RQSID_E_ARG, "%s: n_tokens = %d is negative", who, n_tokens);
  if (vocab < 0 || vocab > RQSID_TRIE_VOCAB_MAX)
    return fail(RQSID_E_ARG, "%s: vocab = %d outside [0, %d]", who, vocab, RQSID_TRIE_VOCAB_MAX);
  if (n_rows == 0 || vocab == 0) return RQSID_OK;
  if (ld < vocab) return fail(RQSID_E_ARG, "%s: ld = %lld < vocab = %d", who, (long long)ld, vocab);
  if (ids_ld < n_tokens) return fail(RQSID_E_ARG, "%s: ids_ld = %lld < n_tokens = %d", who, (long long)ids_ld, n_tokens);
  if (eos < 0 || eos >= vocab) return fail(RQSID_E_ARG, "%s: eos = %d outside [0, %d)", who, eos, vocab);
  if (!count || !child_off || (capacity > 0 && !value))
    return fail(RQSID_E_ARG, "%s: the trie tables are required", who);
  if (!scores || !tok_code || !level_tok || (n_tokens > 0 && !input_ids))
    return fail(RQSID_E_ARG, "%s: scores, tok_code, level_tok and (with tokens) input_ids are required", who);
  const int es = x_format == RQSID_X_F32 ? 4 : 2;
  if (reinterpret_cast<uintptr_t>(scores) % es)
    return fail(RQSID_E_ARG, "%s: scores is not aligned to its element size", who);
  const int64_t slices = cdiv(vocab, kMaskSlice);
  if (n_rows * slices >= (1ll << 31))
    return fail(RQSID_E_ARG, "%s: n_rows x ceil(vocab / %d) must stay below 2^31", who, kMaskSlice);
  const int64_t need = kTrieHeader + n_rows * 16;
  if (!workspace || workspace_bytes < need)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes, (long long)need);
  char* ws = static_cast<char*>(workspace);
  p.ids = input_ids;
  p.ids_i64 = ids_format == RQSID_IDS_I64;
  p.B = n_rows;
  p.ids_ld = ids_ld;
  p.T_len = n_tokens;
  p.scores = scores;
  p.V = vocab;
  p.ld = ld;
  p.tok_code = tok_code;
  p.level_tok = level_tok;
  p.eos = eos;
  p.out_kind = out_kind;
  p.out_node = out_node;
  p.out_count = out_count;
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.ctr = reinterpret_cast<int32_t*>(ws + 4);
  p.rowinfo = reinterpret_cast<int4*>(ws + kTrieHeader);
  p.slices = (int32_t)slices;
  p.ninf = x_format == RQSID_X_F32 ? 0xff800000u : (x_format == RQSID_X_F16 ? 0xfc00fc00u : 0xff80ff80u);
  hipStream_t st = (hipStream_t)stream;
  if (fill_async(ws + 4, 0, 12, st) != hipSuccess) return fail(RQSID_E_LAUNCH, "%s: zeroing the counters", who);
  hipLaunchKernelGGL(trie_walk_kernel, dim3((unsigned)cdiv(n_rows, 4)), dim3(256), 0, st, p);
  if ((rc = check_launch("rqsid_trie_mask (walk)"))) return rc;
  const dim3 grid((unsigned)(n_rows * slices));
  if (es == 4) hipLaunchKernelGGL(trie_mask_kernel<4>, grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL(trie_mask_kernel<2>, grid, dim3(256), 0, st, p);
  return check_launch("rqsid_trie_mask (mask)");
}

int rqsid_trie_beam_step(int64_t capacity, int32_t levels, const int32_t* sizes, const int32_t* count,
                         const int32_t* value, const int32_t* child_off, int32_t depth, int64_t n_rows,
                         int32_t beam_in, int32_t beam_out, const int32_t* node_in, const float* score_in,
                         const void* logp, int32_t x_format, int32_t vocab, int64_t ld, const int32_t* level_tok,
                         int32_t* node_out, float* score_out, int32_t* parent_out, int32_t* value_out,
                         int32_t* token_out, void* stream) {
  const char* const who = "rqsid_trie_beam_step";
  int rc;
  BeamStepParams p{};
  if ((rc = trie_tables(who, capacity, levels, sizes, count, value, child_off, p.T))) return rc;
  if ((rc = trie_check_format(who, x_format))) return rc;
  if (depth < 0 || depth >= levels) return fail(RQSID_E_ARG, "%s: depth = %d outside [0, %d)", who, depth, levels);
  if (beam_in < 1 || beam_in > RQSID_TRIE_BEAM_MAX || beam_out < 1 || beam_out > RQSID_TRIE_BEAM_MAX)
    return fail(RQSID_E_ARG, "%s: beam_in = %d, beam_out = %d outside [1, %d]", who, beam_in, beam_out,
                RQSID_TRIE_BEAM_MAX);
  if (n_rows < 0 || n_rows >= (1ll << 31))
    return fail(RQSID_E_ARG, "%s: n_rows = %lld outside [0, 2^31)", who, (long long)n_rows);
  if (vocab < 1 || vocab > RQSID_TRIE_VOCAB_MAX)
    return fail(RQSID_E_ARG, "%s: vocab = %d outside [1, %d]", who, vocab, RQSID_TRIE_VOCAB_MAX);
  if (ld < vocab) return fail(RQSID_E_ARG, "%s: ld = %lld < vocab = %d", who, (long long)ld, vocab);
  if (n_rows == 0) return RQSID_OK;
  if (!count || !child_off || (capacity > 0 && !value))
    return fail(RQSID_E_ARG, "%s: the trie tables are required", who);
  if (!node_in || !logp || !level_tok || !node_out || !score_out)
    return fail(RQSID_E_ARG, "%s: node_in, logp, level_tok, node_out and score_out are required", who);
  p.depth = depth;
  p.beam_in = beam_in;
  p.beam_out = beam_out;
  p.node_in = node_in;
  p.score_in = score_in;
  p.logp = logp;
  p.x_format = x_format;
  p.V = vocab;
  p.ld = ld;
  p.level_tok = level_tok;
  p.node_out = node_out;
  p.score_out = score_out;
  p.parent_out = parent_out;
  p.value_out = value_out;
  p.token_out = token_out;
  hipLaunchKernelGGL(trie_beam_kernel, dim3((unsigned)n_rows), dim3(256), 0, (hipStream_t)stream, p);
  return check_launch(who);
}

}  // extern "C"
