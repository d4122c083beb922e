// id_cells.hip — rqsid_id_cells: the ID cell index.  A cell is the set of rows with the same full
// ID.  The rows arrive grouped by every level but the last (rqsid_bucket's output), so a group's cells are the
// occupied values of its rows' last-level ("fine") ID: one LDS histogram over the fine ID per group finds them, an
// LDS cursor places the rows, and each cell is ranked by (key bits, row number) words in LDS.
//
//   pass 1  cells_count_kernel  per group: histogram, number of non-empty cells; each position's bin to the workspace
//   scan    cells_scan_kernel   one block: each group's first cell number
//   pass 2  cells_place_kernel  per group: recount from the stored bins, exclusive scan, per-cell outputs,
//                               placement of the rows (in cursor order) into the workspace
//   stats   cells_stats_kernel  the call's counters from the cells' sizes
//   pass 3  cells_rank_kernel   per tile of 1024 positions: the placed rows' words in LDS, each cell that starts in
//                               the tile ranked, every per-row output and out_order written
//
// Groups are unbounded (only the n_fine + 1 counters live in LDS).  Passes 1 and 2 exist in three block sizes by the
// group's rows (one wave up to kCellsWaveRows: typical groups hold a few hundred rows, XL ones ~95; 256 threads; 1024
// threads beyond kCellsBlockRows); each launch covers every group and a block of another class leaves at once.
// Pass 3 does not follow the groups, so one large group is ranked by many blocks.
// Ranking: a cell of up to kCellsCount rows is ranked by counting, one thread per row, over its words in LDS (the
// tile's buffer reaches to the end of the cell that holds the tile's last position), one of up to kCellsLdsRows rows
// by a bitonic sort of those words, and a larger one by the block that holds its first position: sorted runs written to the workspace, each element's rank being the sum of its lower
// bounds in the runs (the words are distinct: the row number is part of them).  That last path costs
// rows x runs x log2(run) reads for one cell.
// Safety: every global index is formed from a checked value.  Positions stay inside the group's clamped span or the
// cell's checked span, rows are compared with n_rows before they index anything, cell numbers with the cell
// capacity, and a fine ID outside [0, n_fine) only selects the extra bin.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "internal.h"

namespace rqsid {
namespace {

constexpr int kCellsLdsRows = 1024;     // largest cell ranked in LDS in one piece (a power of two: the bitonic width)
constexpr int kCellsTile = 1024;        // positions per block of pass 3
constexpr int kCellsWaveRows = 1536;    // groups up to this many rows run on one-wave blocks
constexpr int kCellsBlockRows = 16384;  // and up to this many on 256 threads
constexpr int kCellsHeader = 256;       // workspace header: error word, counters
constexpr int kCellsCounters = 37;      // n_cells, cells >= 2, rows in them, cells of 1, largest, 32 size bins
constexpr int kCellsCount = 384;        // cells up to this size are ranked by counting, larger ones by a sort
constexpr int kCellsList = 8;           // cells beyond kCellsCount that can start inside one tile, with room
constexpr uint32_t kCellsErrRow = 1u, kCellsErrOff = 2u, kCellsErrFine = 4u;
constexpr uint64_t kCellsPad = ~0ull;
constexpr uint16_t kCellsNoBin = 0xffffu;  // bins[] entry of a row_index entry that was skipped
constexpr int32_t kCellsNoCode = -1;       // poscell[] entry of a position pass 3 leaves alone
static_assert(kCellsTile >= kCellsLdsRows, "a tile holds the start of at most one cell beyond the buffer");

struct CellsParams {
  int64_t n_rows;
  const int32_t* row_index;
  int32_t n_groups;
  const int32_t* seg_off;
  const uint8_t* flags;
  const int32_t* fine;
  int32_t n_fine;
  const float* key;
  int32_t *out_order, *out_rank, *out_size, *out_cell, *cell_off, *cell_group, *cell_fine;
  uint32_t* err;       // workspace [0, 4)
  int32_t* ctr;        // workspace [4, 4 + 4 kCellsCounters)
  int32_t* ncells;     // [n_groups]
  int32_t* cell_base;  // [n_groups + 1]
  int32_t* xoff;       // [n_groups] first position of the group's extra bin
  int32_t* xcnt;       // [n_groups] rows in it
  uint64_t* runs;      // [n_rows] by position: sorted runs of the cells beyond the LDS buffer
  int32_t* placed;     // [n_rows] by position: the rows grouped by cell, in cursor order
  int32_t* poscell;    // [n_rows] by position: the cell number, -2 - group for an extra bin, kCellsNoCode
  int32_t* csize;      // [cell_cap] rows of each cell
  uint16_t* bins;      // [n_rows] by position of row_index: pass 1's bin of the row, read back by pass 2
  int64_t cell_cap;
};

struct CellsPlan {
  int64_t off_base, off_ncells, off_xoff, off_xcnt, off_runs, off_placed, off_poscell, off_csize, off_bins, bytes, cap;
};

inline CellsPlan cells_plan(int64_t n_rows, int64_t n_groups, int64_t n_fine) {
  CellsPlan pl;
  pl.cap = n_groups * n_fine < n_rows ? n_groups * n_fine : n_rows;
  pl.off_base = kCellsHeader;
  pl.off_ncells = pl.off_base + (n_groups + 1) * 4;
  pl.off_xoff = pl.off_ncells + n_groups * 4;
  pl.off_xcnt = pl.off_xoff + n_groups * 4;
  pl.off_runs = (pl.off_xcnt + n_groups * 4 + 7) / 8 * 8;
  pl.off_placed = pl.off_runs + n_rows * 8;
  pl.off_poscell = pl.off_placed + n_rows * 4;
  pl.off_csize = pl.off_poscell + n_rows * 4;
  pl.off_bins = pl.off_csize + pl.cap * 4;
  pl.bytes = (pl.off_bins + n_rows * 2 + 7) / 8 * 8;
  return pl;
}

// the float's place in a total order: -0 is +0, every NaN ranks after +inf
__device__ __forceinline__ uint32_t cells_key_bits(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the group's span of positions, clamped into [0, n_rows]; false when an offset had to be clamped
__device__ __forceinline__ bool cells_span(const CellsParams& p, int g, int64_t& r0, int64_t& r1) {
  const int64_t a = p.seg_off[g], b = p.seg_off[g + 1];
  r0 = a < 0 ? 0 : (a > p.n_rows ? p.n_rows : a);
  r1 = b < r0 ? r0 : (b > p.n_rows ? p.n_rows : b);
  return r0 == a && r1 == b;
}

// the block size that takes a group of `span` rows
__device__ __forceinline__ int cells_class(int64_t span) {
  return span <= kCellsWaveRows ? 64 : (span <= kCellsBlockRows ? 256 : 1024);
}

__device__ __forceinline__ int32_t cells_row_at(const CellsParams& p, int64_t pos) {
  return p.row_index ? p.row_index[pos] : (int32_t)pos;
}

// bin of a checked row: its fine ID, or the extra bin n_fine when the ID is out of range (no address from the ID)
__device__ __forceinline__ int cells_bin(const CellsParams& p, int32_t row, uint32_t& errs) {
  if (!p.fine) return 0;
  const uint32_t f = (uint32_t)p.fine[row];
  if (f < (uint32_t)p.n_fine) return (int)f;
  errs |= kCellsErrFine;
  return p.n_fine;
}

template <int T>
__global__ __launch_bounds__(T) void cells_count_kernel(CellsParams p) {
  extern __shared__ __attribute__((aligned(16))) int32_t hist[];
  __shared__ int32_t nz;
  const int g = blockIdx.x, t = threadIdx.x;
  int64_t r0, r1;
  const bool clean = cells_span(p, g, r0, r1);
  const int64_t span = r1 - r0;
  if (cells_class(span) != T) return;
  uint32_t errs = clean ? 0u : kCellsErrOff;
  const bool skip = p.flags && (p.flags[g] & RQSID_CELLS_GROUP_SKIP);
  if (!skip && span > 0) {
    for (int b = t; b < p.n_fine; b += T) hist[b] = 0;
    if (t == 0) nz = 0;
    __syncthreads();
    for (int64_t i = t; i < span; i += T) {
      const int32_t row = cells_row_at(p, r0 + i);
      if ((uint32_t)row >= (uint64_t)p.n_rows) {
        errs |= kCellsErrRow;
        p.bins[r0 + i] = kCellsNoBin;
        continue;
      }
      const int bin = cells_bin(p, row, errs);
      p.bins[r0 + i] = (uint16_t)bin;
      if (bin < p.n_fine) atomicAdd(&hist[bin], 1);
    }
    __syncthreads();
    int c = 0;
    for (int b = t; b < p.n_fine; b += T) c += hist[b] != 0;
    if (c) atomicAdd(&nz, c);
    __syncthreads();
    if (t == 0) p.ncells[g] = nz;
  } else {
    if (t == 0) p.ncells[g] = 0;
    if (skip)  // a skipped group's row_index entries are still checked
      for (int64_t i = t; i < span; i += T)
        if ((uint32_t)cells_row_at(p, r0 + i) >= (uint64_t)p.n_rows) errs |= kCellsErrRow;
  }
  if (errs) atomicOr(p.err, errs);
}

// one block: exclusive scan of the groups' cell counts (the layout of bucket_scan_kernel: a run of groups per thread)
__global__ __launch_bounds__(1024) void cells_scan_kernel(const int32_t* __restrict__ counts, int S,
                                                          int32_t* __restrict__ base) {
  __shared__ int32_t sa[1024];
  const int t = threadIdx.x;
  const int run = (S + 1023) / 1024;
  const int64_t k0l = (int64_t)t * run;
  const int k0 = k0l < S ? (int)k0l : S, k1 = k0 + run < S ? k0 + run : S;
  int32_t a = 0;
#pragma unroll 8
  for (int k = k0; k < k1; ++k) a += counts[k];  // (independent loads: several in flight)
  sa[t] = a;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int32_t v = t >= o ? sa[t - o] : 0;
    __syncthreads();
    sa[t] += v;
    __syncthreads();
  }
  int32_t e = sa[t] - a;
  for (int k = k0; k < k1; ++k) {
    base[k] = e;
    e += counts[k];
  }
  if (t == 1023) base[S] = sa[1023];
}

// everything a row and its place get: out_order by position, rank / size / cell by row (-1 for the extra bin)
__device__ __forceinline__ void cells_emit(const CellsParams& p, int64_t pos, int64_t lim, int32_t row, bool counted,
                                           int32_t rank, int32_t size, int32_t cell) {
  if (pos >= lim) return;  // (only tables that change under the call can ask for it)
  p.out_order[pos] = row;
  if ((uint32_t)row < (uint64_t)p.n_rows) {
    p.out_rank[row] = counted ? rank : -1;
    p.out_size[row] = counted ? size : -1;
    p.out_cell[row] = counted ? cell : -1;
  }
}

// the word of the row placed at `pos`: key bits above the row number (rows that fail the check sort last)
__device__ __forceinline__ uint64_t cells_word(const CellsParams& p, int64_t pos, int64_t lim, bool keyed) {
  if (pos >= lim) return kCellsPad;
  const int32_t row = p.placed[pos];
  uint32_t kb = 0u;
  if ((uint32_t)row >= (uint64_t)p.n_rows) return kCellsPad;
  if (keyed && p.key) kb = cells_key_bits(p.key[row]);
  return ((uint64_t)kb << 32) | (uint32_t)row;
}

template <int T>
__global__ __launch_bounds__(T) void cells_place_kernel(CellsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cells_lds[];
  const int nb = p.n_fine + 1;  // the bins: the fine IDs, then the extra bin of rows whose fine ID is out of range
  int32_t* A = reinterpret_cast<int32_t*>(cells_lds);   // [nb] count -> start (cursor) of each bin
  uint16_t* ord = reinterpret_cast<uint16_t*>(A + nb);  // [nb] the bin's cell number inside the group
  __shared__ int32_t sa[T], sb[T];
  const int g = blockIdx.x, t = threadIdx.x;
  int64_t r0, r1;
  cells_span(p, g, r0, r1);
  const int64_t span = r1 - r0;
  if (cells_class(span) != T) return;
  const int32_t n_cells = p.cell_base[p.n_groups];
  if (g == 0 && t == 0) {
    p.ctr[0] = n_cells;
    if (n_cells == 0) p.cell_off[0] = 0;
  }
  if (span == 0) return;
  if (p.flags && (p.flags[g] & RQSID_CELLS_GROUP_SKIP)) {  // final here: pass 3 leaves these positions alone
    for (int64_t i = t; i < span; i += T) cells_emit(p, r0 + i, r1, cells_row_at(p, r0 + i), false, -1, -1, -1);
    return;
  }
  for (int b = t; b < nb; b += T) A[b] = 0;
  __syncthreads();
  for (int64_t i = t; i < span; i += T) {
    const int bin = p.bins[r0 + i];  // pass 1 looked the row's fine ID up (and reported what it clamped)
    if (bin < nb) atomicAdd(&A[bin], 1);
  }
  __syncthreads();
  // exclusive scans over the bins (rows before the bin, non-empty cells before it): a run of bins per thread
  const int run = (nb + T - 1) / T;
  const int k0 = t * run < nb ? t * run : nb, k1 = k0 + run < nb ? k0 + run : nb;
  int32_t a = 0, c = 0;
  for (int k = k0; k < k1; ++k) {
    const int32_t cnt = A[k];
    a += cnt;
    c += cnt != 0 && k < p.n_fine;
  }
  sa[t] = a;
  sb[t] = c;
  __syncthreads();
  for (int o = 1; o < T; o <<= 1) {
    const int32_t va = t >= o ? sa[t - o] : 0, vb = t >= o ? sb[t - o] : 0;
    __syncthreads();
    sa[t] += va;
    sb[t] += vb;
    __syncthreads();
  }
  const int32_t base = p.cell_base[g];
  {
    int32_t ea = sa[t] - a, ec = sb[t] - c;
    for (int k = k0; k < k1; ++k) {
      const int32_t cnt = A[k];
      A[k] = ea;
      ord[k] = (uint16_t)ec;
      if (k == p.n_fine) {
        p.xoff[g] = (int32_t)(r0 + ea);
        p.xcnt[g] = cnt;
      } else if (cnt != 0) {
        const int64_t j = (int64_t)base + ec;
        if (j >= 0 && j < p.cell_cap) {
          p.cell_off[j] = (int32_t)(r0 + ea);
          p.cell_group[j] = g;
          p.cell_fine[j] = k;
          p.csize[j] = cnt;
          if (j + 1 == n_cells) p.cell_off[j + 1] = (int32_t)(r0 + ea + cnt);
        }
        ++ec;
      }
      ea += cnt;
    }
  }
  const int32_t n_valid = sa[T - 1];
  __syncthreads();
  // place the rows: an LDS cursor gives the slot inside the bin's span (pass 3's ranking fixes the final order)
  for (int64_t i = t; i < span; i += T) {
    const int bin = p.bins[r0 + i];
    if (bin >= nb) continue;
    const int32_t slot = atomicAdd(&A[bin], 1);
    if ((uint32_t)slot < (uint64_t)span) {
      p.placed[r0 + slot] = cells_row_at(p, r0 + i);
      p.poscell[r0 + slot] = bin < p.n_fine ? base + (int32_t)ord[bin] : -2 - g;
    }
  }
  for (int64_t i = (int64_t)n_valid + t; i < span; i += T) p.out_order[r0 + i] = -1;  // entries that were skipped
}

// The call's counters from the cells' sizes: registers, one wave reduction, LDS, then one global atomic per block and
// counter (tens of thousands of groups adding to the same words from pass 2 would queue up at one L2 line).
__global__ __launch_bounds__(256) void cells_stats_kernel(CellsParams p) {
  __shared__ int32_t stat[kCellsCounters];
  const int t = threadIdx.x;
  if (t < kCellsCounters) stat[t] = 0;
  __syncthreads();
  int64_t n_cells = p.cell_base[p.n_groups];
  if (n_cells > p.cell_cap) n_cells = p.cell_cap;
  int32_t n2 = 0, r2 = 0, n1 = 0, mx = 0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + t; j < n_cells; j += (int64_t)gridDim.x * 256) {
    const int32_t cnt = p.csize[j];
    if (cnt <= 0) continue;
    if (cnt >= 2) {
      ++n2;
      r2 += cnt;
    } else {
      ++n1;
    }
    mx = cnt > mx ? cnt : mx;
    atomicAdd(&stat[5 + (31 - __clz(cnt))], 1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n2 += __shfl_xor(n2, o);
    r2 += __shfl_xor(r2, o);
    n1 += __shfl_xor(n1, o);
    const int32_t other = __shfl_xor(mx, o);
    mx = other > mx ? other : mx;
  }
  if ((t & 63) == 0) {
    atomicAdd(&stat[1], n2);
    atomicAdd(&stat[2], r2);
    atomicAdd(&stat[3], n1);
    atomicMax(&stat[4], mx);
  }
  __syncthreads();
  if (t > 0 && t < kCellsCounters && stat[t]) {
    if (t == 4) atomicMax(&p.ctr[4], stat[4]); else atomicAdd(&p.ctr[t], stat[t]);
  }
}

// first position and rows of the cell (or extra bin) behind a poscell code, checked against every table's size
__device__ __forceinline__ bool cells_geometry(const CellsParams& p, int32_t code, int64_t& cs, int32_t& m) {
  if (code >= 0) {
    if (code >= p.cell_cap) return false;
    cs = p.cell_off[code];
    m = p.csize[code];
  } else {
    const int64_t g = -2 - (int64_t)code;
    if (g < 0 || g >= p.n_groups) return false;
    cs = p.xoff[g];
    m = p.xcnt[g];
  }
  return cs >= 0 && m > 0 && cs + m <= p.n_rows;
}

template <int T>
__device__ __forceinline__ void cells_bitonic(uint64_t* buf, int width, int t) {
  for (int k = 2; k <= width; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < width; i += T) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = buf[i], b = buf[x];
          if ((a > b) == ((i & k) == 0)) {
            buf[i] = b;
            buf[x] = a;
          }
        }
      }
      __syncthreads();
    }
}

// rank one cell of m > kCellsLdsRows rows at positions [c0, c0 + m): sorted runs, then the sum of lower bounds
template <int T>
__device__ void cells_rank_large(const CellsParams& p, uint64_t* buf, int64_t c0, int32_t m, bool counted,
                                 int32_t cell, int t) {
  const int64_t lim = c0 + m;
  const int n_runs = (m + kCellsLdsRows - 1) / kCellsLdsRows;
  for (int r = 0; r < n_runs; ++r) {
    const int32_t base = r * kCellsLdsRows;
    const int len = m - base < kCellsLdsRows ? m - base : kCellsLdsRows;
    for (int i = t; i < kCellsLdsRows; i += T)
      buf[i] = i < len ? cells_word(p, c0 + base + i, lim, counted) : kCellsPad;
    __syncthreads();
    cells_bitonic<T>(buf, kCellsLdsRows, t);
    for (int i = t; i < len; i += T) p.runs[c0 + base + i] = buf[i];
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  for (int32_t i = t; i < m; i += T) {
    const uint64_t w = p.runs[c0 + i];
    const int own = i / kCellsLdsRows;
    int32_t rank = i - own * kCellsLdsRows;
    for (int r = 0; r < n_runs; ++r) {
      if (r == own) continue;
      const uint64_t* run = p.runs + c0 + (int64_t)r * kCellsLdsRows;
      int lo = 0, hi = m - r * kCellsLdsRows < kCellsLdsRows ? m - r * kCellsLdsRows : kCellsLdsRows;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (run[mid] < w) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < m) cells_emit(p, c0 + rank, lim, (int32_t)(uint32_t)w, counted, rank, m, cell);
  }
  __syncthreads();
}

// Pass 3.  Block b owns the cells (and extra bins) whose FIRST position lies in [b kCellsTile, (b + 1) kCellsTile).
// It loads the words of its tile and on to the end of the cell that holds the tile's last position (when that cell
// starts in the tile and fits the buffer: at most kCellsLdsRows - 1 further positions), ranks each owned cell of up to
// kCellsCount rows by counting the smaller words of its span (one thread per row), then, one after another, sorts the
// owned cells of up to kCellsLdsRows rows in sbuf and runs cells_rank_large on a larger one.
__global__ __launch_bounds__(256) void cells_rank_kernel(CellsParams p) {
  constexpr int T = 256;
  __shared__ uint64_t buf[kCellsTile + kCellsLdsRows];
  __shared__ uint64_t sbuf[kCellsLdsRows];  // the cell being sorted
  __shared__ int32_t code[kCellsTile + kCellsLdsRows];
  __shared__ int32_t list[kCellsList], nlist;
  const int t = threadIdx.x;
  const int64_t P = (int64_t)blockIdx.x * kCellsTile;
  int64_t E = P + kCellsTile < p.n_rows ? P + kCellsTile : p.n_rows;
  {
    const int32_t c = p.poscell[E - 1];
    int64_t cs;
    int32_t m;
    if (c != kCellsNoCode && cells_geometry(p, c, cs, m) && cs >= P && m <= kCellsLdsRows && cs + m > E) E = cs + m;
  }
  const int n_load = (int)(E - P);  // <= kCellsTile + kCellsLdsRows - 1
  for (int i = t; i < n_load; i += T) {
    const int32_t c = p.poscell[P + i];
    code[i] = c;
    buf[i] = c == kCellsNoCode ? kCellsPad : cells_word(p, P + i, E, c >= 0);
  }
  if (t == 0) nlist = 0;
  __syncthreads();
  for (int i = t; i < n_load; i += T) {
    const int32_t c = code[i];
    int64_t cs;
    int32_t m;
    if (c == kCellsNoCode || !cells_geometry(p, c, cs, m)) continue;
    if (cs < P || cs >= P + kCellsTile) continue;  // another block's cell
    if (m > kCellsCount) {
      if (P + i == cs) {
        const int32_t slot = atomicAdd(&nlist, 1);
        if (slot < kCellsList) list[slot] = c;
      }
      continue;
    }
    const int lo = (int)(cs - P);
    if (lo + m > n_load) continue;  // (only tables that change under the call can ask for it)
    const uint64_t w = buf[i];
    int32_t rank = 0;
    for (int j = lo; j < lo + m; ++j) rank += buf[j] < w;
    cells_emit(p, cs + rank, cs + m, (int32_t)(uint32_t)w, c >= 0, rank, m, c);
  }
  __syncthreads();
  const int32_t n_large = nlist < kCellsList ? nlist : kCellsList;
  for (int q = 0; q < n_large; ++q) {
    const int32_t c = list[q];
    int64_t cs;
    int32_t m;
    if (!cells_geometry(p, c, cs, m)) continue;  // (block-uniform, as everything below)
    if (m > kCellsLdsRows) {
      cells_rank_large<T>(p, sbuf, cs, m, c >= 0, c, t);
      continue;
    }
    const int lo = (int)(cs - P);
    if (lo + m > n_load) continue;
    int width = 512;
    while (width < m) width <<= 1;
    for (int i = t; i < width; i += T) sbuf[i] = i < m ? buf[lo + i] : kCellsPad;
    __syncthreads();
    cells_bitonic<T>(sbuf, width, t);
    for (int i = t; i < m; i += T) cells_emit(p, cs + i, cs + m, (int32_t)(uint32_t)sbuf[i], c >= 0, i, m, c);
    __syncthreads();
  }
}

inline size_t cells_place_lds(int n_fine) { return (size_t)(n_fine + 1) * 6 + 16; }

int cells_check_shape(const char* who, int64_t n_rows, int64_t n_groups, int32_t n_fine) {
  if (n_rows < 0 || n_rows >= (1ll << 31))
    return fail(RQSID_E_ARG, "%s: n_rows = %lld outside [0, 2^31)", who, (long long)n_rows);
  if (n_groups < 0) return fail(RQSID_E_ARG, "%s: n_groups = %lld is negative", who, (long long)n_groups);
  if (n_fine < 1 || n_fine > RQSID_CELLS_FINE_MAX)
    return fail(RQSID_E_ARG, "%s: n_fine = %d outside [1, %d]", who, n_fine, RQSID_CELLS_FINE_MAX);
  return RQSID_OK;
}

}  // namespace
}  // namespace rqsid

using namespace rqsid;

extern "C" {

int32_t rqsid_id_cells_lds_rows(void) { return kCellsLdsRows; }

int64_t rqsid_id_cells_workspace_bytes(int64_t n_rows, int32_t n_groups, int32_t n_fine) {
  int rc;
  if ((rc = cells_check_shape("rqsid_id_cells_workspace_bytes", n_rows, n_groups, n_fine))) return rc;
  return cells_plan(n_rows, n_groups, n_fine).bytes;
}

int rqsid_id_cells(int64_t n_rows, const int32_t* row_index, int32_t n_groups, const int32_t* seg_row_off,
                   const uint8_t* group_flags, const int32_t* fine_id, int32_t n_fine, const float* rank_key,
                   int32_t* out_order, int32_t* out_rank, int32_t* out_size, int32_t* out_cell, int32_t* cell_off,
                   int32_t* cell_group, int32_t* cell_fine, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "rqsid_id_cells";
  int rc;
  if ((rc = cells_check_shape(who, n_rows, n_groups, n_fine))) return rc;
  if (n_rows == 0) return RQSID_OK;
  if (n_groups < 1 || !seg_row_off)
    return fail(RQSID_E_ARG, "%s: n_groups = %d and seg_row_off are required with rows", who, n_groups);
  if (!fine_id && n_fine > 1) return fail(RQSID_E_ARG, "%s: fine_id NULL needs n_fine = 1, not %d", who, n_fine);
  if (!out_order || !out_rank || !out_size || !out_cell || !cell_off || !cell_group || !cell_fine)
    return fail(RQSID_E_ARG, "%s: every output is required", who);
  const CellsPlan pl = cells_plan(n_rows, n_groups, n_fine);
  if (!workspace || workspace_bytes < pl.bytes)
    return fail(RQSID_E_WORKSPACE, "%s: workspace %lld < %lld bytes", who, (long long)workspace_bytes,
                (long long)pl.bytes);
  char* ws = static_cast<char*>(workspace);
  CellsParams p;
  p.n_rows = n_rows;
  p.row_index = row_index;
  p.n_groups = n_groups;
  p.seg_off = seg_row_off;
  p.flags = group_flags;
  p.fine = fine_id;
  p.n_fine = n_fine;
  p.key = rank_key;
  p.out_order = out_order;
  p.out_rank = out_rank;
  p.out_size = out_size;
  p.out_cell = out_cell;
  p.cell_off = cell_off;
  p.cell_group = cell_group;
  p.cell_fine = cell_fine;
  p.err = reinterpret_cast<uint32_t*>(ws);
  p.ctr = reinterpret_cast<int32_t*>(ws + 4);
  p.cell_base = reinterpret_cast<int32_t*>(ws + pl.off_base);
  p.ncells = reinterpret_cast<int32_t*>(ws + pl.off_ncells);
  p.xoff = reinterpret_cast<int32_t*>(ws + pl.off_xoff);
  p.xcnt = reinterpret_cast<int32_t*>(ws + pl.off_xcnt);
  p.runs = reinterpret_cast<uint64_t*>(ws + pl.off_runs);
  p.placed = reinterpret_cast<int32_t*>(ws + pl.off_placed);
  p.poscell = reinterpret_cast<int32_t*>(ws + pl.off_poscell);
  p.csize = reinterpret_cast<int32_t*>(ws + pl.off_csize);
  p.bins = reinterpret_cast<uint16_t*>(ws + pl.off_bins);
  p.cell_cap = pl.cap;
  hipStream_t st = (hipStream_t)stream;
  if (fill_async(ws + 4, 0, (size_t)kCellsCounters * 4, st) != hipSuccess ||
      fill_async(p.poscell, 0xff, (size_t)n_rows * 4, st) != hipSuccess)  // kCellsNoCode everywhere
    return fail(RQSID_E_LAUNCH, "%s: zeroing the counters", who);
  const dim3 grid((unsigned)n_groups);
  const size_t lds1 = (size_t)n_fine * 4, lds2 = cells_place_lds(n_fine);
  hipLaunchKernelGGL(cells_count_kernel<64>, grid, dim3(64), lds1, st, p);
  hipLaunchKernelGGL(cells_count_kernel<256>, grid, dim3(256), lds1, st, p);
  hipLaunchKernelGGL(cells_count_kernel<1024>, grid, dim3(1024), lds1, st, p);
  if ((rc = check_launch("rqsid_id_cells (count)"))) return rc;
  hipLaunchKernelGGL(cells_scan_kernel, dim3(1), dim3(1024), 0, st, p.ncells, n_groups, p.cell_base);
  if ((rc = check_launch("rqsid_id_cells (scan)"))) return rc;
  hipLaunchKernelGGL(cells_place_kernel<64>, grid, dim3(64), lds2, st, p);
  hipLaunchKernelGGL(cells_place_kernel<256>, grid, dim3(256), lds2, st, p);
  hipLaunchKernelGGL(cells_place_kernel<1024>, grid, dim3(1024), lds2, st, p);
  if ((rc = check_launch("rqsid_id_cells (place)"))) return rc;
  hipLaunchKernelGGL(cells_stats_kernel, dim3(grid_cap(cdiv(pl.cap, 2048), 1024)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(cells_rank_kernel, dim3((unsigned)cdiv(n_rows, kCellsTile)), dim3(256), 0, st, p);
  return check_launch("rqsid_id_cells (rank)");
}

}  // extern "C"
