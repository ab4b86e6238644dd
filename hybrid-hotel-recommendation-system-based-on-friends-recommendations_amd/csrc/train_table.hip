// prepare_data on the device (dcnr_train_table_build): the driver's noise
// filter and derived columns (train.py:280-287), then prepare_data
// (train.py:36-65) up to the split -- median fill, category drop, first-
// appearance id maps, sorted category codes, MinMaxScaler fit and transform --
// from the raw review columns to the reference's (collab, cat, num, y), bit for
// bit.  The contract is in include/dcnr.h; DESIGN.md section 9 has the why.
//
//   init      counts, selection state, histograms, min / max keys
//   rows      one lane per input row: the filter flag, the category-missing
//             flag, the raw and derived columns into a column-major float64
//             scratch [n_num][M] (every later column pass streams one column)
//   scan      an inclusive scan of the survivor flags (tile sums, one block
//             over the tile sums, tiles again): a row's output position is the
//             number of survivors before it -- no atomic decides a position
//   emit      row[j] = i, y[j]
//   median    exact radix select, MSB first, 6 passes of 11 bits over order-
//             preserving uint64 keys of the rows that passed the filter, every
//             column in one grid (blockIdx.y).  Both middle order statistics of
//             an even count ride the same passes: a second histogram is kept
//             only once their prefixes differ.  Histograms live in LDS (integer
//             atomics; a wave whose lanes all hold one digit adds once), then
//             go to the column's global histogram with integer atomics.
//   minmax    per column over the surviving rows, filled: uint64 keys, a wave
//             and block reduction, then one integer atomicMin / atomicMax per
//             block.  A +-inf sets DCNR_REQ_BAD_DATA.
//   stats     one block: median, data_min_, data_max_, scale_, min_
//   transform num[j][c] = float32(x * scale_ + min_), never an fma
//   ids       per id column: records (key, j) of the surviving rows, the stable
//             rsort over 65 bits (dropped rows behind everything), segment
//             heads.  rsort is stable and the records enter in row order, so a
//             head is its id's first row.  A sum scan over "row j is a first
//             row" numbers the ids in first-appearance order; a max scan over
//             "head ? index : 0" hands every record its head.
//   cats      per category column: the same sort; a record's code is the
//             number of heads before it.
//
// Every atomic is an integer min, max, add or or: the same bytes on every run.
#include "device_prims.h"

namespace dcnr {

namespace {

using namespace rsort;
using namespace tscan;

constexpr int TT_NT = 256;
constexpr int TT_MAXB = 2048;                 // workgroups of the grid-stride kernels
constexpr int TT_COLB = 256;                  // workgroups per column of the column passes
constexpr int SEL_PASSES = 6;                 // 9 + 5 * 11 bits
constexpr uint64_t KEY_NONE = ~0ull;

struct alignas(16) TRec {
  uint64_t key;
  uint32_t j;      // the row's output position
  uint32_t dead;   // 1: not a surviving row (sorts behind every key)
};

__device__ __forceinline__ uint32_t radix_digit(const TRec& r, int shift) {
  uint32_t d = (uint32_t)(r.key >> shift);
  if (shift > 64 - RBITS) d |= r.dead << (64 - shift);
  return d & (uint32_t)(NB - 1);
}
constexpr int REC_PASSES = (65 + RBITS - 1) / RBITS;

// IEEE order as an unsigned order (not for NaN); -0.0 takes +0.0's key
__device__ __forceinline__ uint64_t okey(double x) {
  uint64_t u = (uint64_t)__double_as_longlong(x);
  if (u == SIGN) u = 0ull;
  return (u & SIGN) ? ~u : (u | SIGN);
}
__device__ __forceinline__ double okey_value(uint64_t k) {
  return __longlong_as_double((long long)((k & SIGN) ? (k & ~SIGN) : ~k));
}

// --------------------------------------------------------------- init, rows
__global__ __launch_bounds__(TT_NT) void tt_init_kernel(int32_t* counts, int n_counts, uint32_t* ghist,
                                                        int64_t n_hist, uint64_t* sel, int n_num,
                                                        uint64_t* mm) {
  const int64_t i0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = i0; i < n_hist; i += step) ghist[i] = 0u;
  if (i0 < n_counts) counts[i0] = 0;
  if (i0 < 4 * (int64_t)n_num) sel[i0] = 0ull;
  if (i0 < n_num) {
    mm[2 * i0] = KEY_NONE;   // the smallest key
    mm[2 * i0 + 1] = 0ull;   // the largest (no double has key 0)
  }
}

__global__ __launch_bounds__(TT_NT) void tt_rows_kernel(const int64_t* cat_key, const double* raw, int64_t M,
                                                        int n_cat, int n_raw, int fcol, double lo, double hi,
                                                        Derived dv, double* colmaj, uint8_t* flags,
                                                        uint32_t* alive, int32_t* counts) {
  __shared__ int part[TT_NT / WAVE];
  int passed = 0;
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < M; i += step) {
    const double* r = raw + i * n_raw;
    bool pass = true;
    if (fcol >= 0) {
      const double v = r[fcol];
      pass = v >= hi || v <= lo;   // (NaN fails both)
    }
    bool miss = false;
    for (int c = 0; c < n_cat; ++c) miss |= cat_key[i * n_cat + c] < 0;
    const bool live = pass && !miss;
    flags[i] = (uint8_t)((pass ? 1 : 0) | (live ? 2 : 0));
    alive[i] = live ? 1u : 0u;
    passed += pass ? 1 : 0;
    for (int c = 0; c < n_raw; ++c) colmaj[(int64_t)c * M + i] = r[c];
    for (int d = 0; d < dv.n; ++d) colmaj[(int64_t)(n_raw + d) * M + i] = derived_value(dv, d, r);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) passed += __shfl_xor(passed, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = passed;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < TT_NT / WAVE; ++w) s += part[w];
    if (s) atomicAdd(counts + 3, s);
  }
}

__global__ __launch_bounds__(TT_NT) void tt_emit_kernel(const uint8_t* flags, const uint32_t* pos,
                                                        const uint8_t* target, int64_t M, int32_t* row,
                                                        float* y, int32_t* counts) {
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < M; i += step) {
    if (flags[i] & 2) {
      const int64_t j = (int64_t)pos[i] - 1;
      if (j >= 0 && j < M) {
        row[j] = (int32_t)i;
        y[j] = target[i] ? 1.0f : 0.0f;
      }
    }
    if (i == M - 1) counts[0] = (int32_t)pos[i];
  }
}

// ------------------------------------------------------------------ median
// sel [n_num][4]: {prefix 0, prefix 1, rank 0, rank 1}; a rank of KEY_NONE: no value
__global__ __launch_bounds__(TT_NT) void tt_sel_hist_kernel(const double* colmaj, const uint8_t* flags,
                                                            int64_t M, int pass, const uint64_t* sel,
                                                            uint32_t* ghist) {
  __shared__ uint32_t h[2][NB];
  const int c = blockIdx.y, lane = threadIdx.x & 63;
  const int shift = 55 - RBITS * pass;
  const uint64_t p0 = sel[4 * c], p1 = sel[4 * c + 1];
  const bool two = pass > 0 && p0 != p1;
  if (sel[4 * c + 2] == KEY_NONE && pass > 0) return;   // (uniform: nothing to select)
  for (int d = threadIdx.x; d < 2 * NB; d += TT_NT) (&h[0][0])[d] = 0u;
  __syncthreads();
  const double* col = colmaj + (int64_t)c * M;
  const int64_t step = (int64_t)gridDim.x * TT_NT;
  for (int64_t base = (int64_t)blockIdx.x * TT_NT + (threadIdx.x & ~63); base < M; base += step) {
    const int64_t i = base + lane;
    double x = 0.0;
    bool valid = false;
    if (i < M) {
      x = col[i];
      valid = (flags[i] & 1) && !is_nan(x);
    }
    const uint64_t k = okey(x);
    const uint64_t above = pass > 0 ? k >> (shift + RBITS) : 0ull;
    const uint32_t d = (uint32_t)(k >> shift) & (uint32_t)(NB - 1);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s == 1 && !two) break;
      const bool m = valid && (pass == 0 || above == (s ? p1 : p0));
      const uint64_t bal = __ballot(m);
      if (bal == 0ull) continue;
      const int first = __ffsll((unsigned long long)bal) - 1;
      const uint32_t d0 = (uint32_t)__shfl((int)d, first, 64);
      if (__ballot(m && d == d0) == bal) {   // one digit in the whole wave: one add
        if (lane == first) atomicAdd(&h[s][d0], (uint32_t)__popcll(bal));
      } else if (m) {
        atomicAdd(&h[s][d], 1u);
      }
    }
  }
  __syncthreads();
  uint32_t* g = ghist + (int64_t)c * 2 * NB;
  for (int d = threadIdx.x; d < (two ? 2 : 1) * NB; d += TT_NT) {
    const uint32_t v = (&h[0][0])[d];
    if (v) atomicAdd(g + d, v);
  }
}

// one workgroup per column: the digit that holds each rank; the histogram is
// zeroed for the next pass.  After the last pass: the median.
__global__ __launch_bounds__(TT_NT) void tt_sel_pick_kernel(int pass, uint64_t* sel, uint32_t* ghist,
                                                            double* median) {
  __shared__ uint32_t sm[TT_NT / 64];
  __shared__ uint32_t found_d[2], found_below[2];
  const int c = blockIdx.x;
  uint64_t* st = sel + 4 * c;
  const uint64_t p0 = st[0], p1 = st[1];
  uint64_t r0 = st[2], r1 = st[3];
  const bool two = pass > 0 && p0 != p1;
  const bool none = pass > 0 && r0 == KEY_NONE;
  constexpr int PER = NB / TT_NT;
  uint32_t* g = ghist + (int64_t)c * 2 * NB;
  uint64_t k_total = 0;
  for (int s = 0; s < 2; ++s) {
    const uint32_t* hs = g + ((s == 1 && two) ? NB : 0);
    uint32_t v[PER], sum = 0u;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      v[q] = hs[threadIdx.x * PER + q];
      sum += v[q];
    }
    uint32_t total;
    const uint32_t inc = block_scan<false, TT_NT>(sum, sm, total);
    if (pass == 0 && s == 0) {
      k_total = total;
      if (total == 0u) {
        r0 = r1 = KEY_NONE;
      } else {
        r0 = (total - 1u) / 2u;
        r1 = total / 2u;
      }
    }
    const uint64_t r = s ? r1 : r0;
    uint32_t below = inc - sum;
    if (r != KEY_NONE) {
#pragma unroll
      for (int q = 0; q < PER; ++q) {
        if (r >= below && r < (uint64_t)below + v[q]) {
          found_d[s] = threadIdx.x * PER + q;
          found_below[s] = below;
        }
        below += v[q];
      }
    }
    __syncthreads();
  }
  for (int d = threadIdx.x; d < 2 * NB; d += TT_NT) g[d] = 0u;
  if (threadIdx.x == 0) {
    if (none || r0 == KEY_NONE) {
      st[2] = st[3] = KEY_NONE;
      if (pass == SEL_PASSES - 1) median[c] = __longlong_as_double(0x7FF8000000000000ll);
    } else {
      const uint64_t n0 = (p0 << RBITS) | found_d[0], n1 = (p1 << RBITS) | found_d[1];
      st[0] = n0;
      st[1] = n1;
      st[2] = r0 - found_below[0];
      st[3] = r1 - found_below[1];
      if (pass == SEL_PASSES - 1) {
        // an even count when the two ranks differ (in their key, or within it):
        // its sum is formed even of two equal values -- it may overflow, as
        // the reference's does
        const bool even = n0 != n1 || st[2] != st[3];
        const double a = okey_value(n0), b = okey_value(n1);
        median[c] = even ? (a + b) / 2.0 : a;
      }
    }
  }
}

// ----------------------------------------------------------------- scaler
__global__ __launch_bounds__(TT_NT) void tt_minmax_kernel(const double* colmaj, const uint8_t* flags, int64_t M,
                                                          const double* median, uint64_t* mm,
                                                          int32_t* counts) {
  __shared__ uint64_t smin[TT_NT / 64], smax[TT_NT / 64];
  __shared__ int sinf[TT_NT / 64];
  const int c = blockIdx.y;
  const double med = median[c];
  const double* col = colmaj + (int64_t)c * M;
  uint64_t lo = KEY_NONE, hi = 0ull;
  int inf = 0;
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < M; i += step) {
    if (!(flags[i] & 2)) continue;
    double x = col[i];
    if (is_nan(x)) x = med;
    if (is_nan(x)) continue;
    inf |= is_inf(x) ? 1 : 0;
    const uint64_t k = okey(x);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t l2 = (uint64_t)__shfl_xor((long long)lo, o, 64), h2 = (uint64_t)__shfl_xor((long long)hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    inf |= __shfl_xor(inf, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    smin[threadIdx.x >> 6] = lo;
    smax[threadIdx.x >> 6] = hi;
    sinf[threadIdx.x >> 6] = inf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TT_NT / 64; ++w) {
      lo = smin[w] < lo ? smin[w] : lo;
      hi = smax[w] > hi ? smax[w] : hi;
      inf |= sinf[w];
    }
    if (lo != KEY_NONE) {
      atomicMin((unsigned long long*)(mm + 2 * c), (unsigned long long)lo);
      atomicMax((unsigned long long*)(mm + 2 * c + 1), (unsigned long long)hi);
    }
    if (inf) atomicOr(counts + 4, DCNR_REQ_BAD_DATA);
  }
}

// MinMaxScaler.fit's scale_ and min_: separately rounded operations
__device__ __forceinline__ void fit_scale(double dmin, double dmax, double& scale, double& mn) {
#pragma clang fp contract(off)
  double range = dmax - dmin;
  if (range < 10.0 * 2.220446049250313e-16) range = 1.0;
  scale = 1.0 / range;
  const double t = dmin * scale;
  mn = 0.0 - t;
}

// stats [5][n_num]: median, data_min_, data_max_, scale_, min_
__global__ __launch_bounds__(MAXC) void tt_stats_kernel(const uint64_t* mm, const double* median, int n_num,
                                                           double* stats, double* host_stats) {
  const int c = threadIdx.x;
  if (c >= n_num) return;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  const bool none = mm[2 * c] == KEY_NONE;
  const double dmin = none ? nan : okey_value(mm[2 * c]), dmax = none ? nan : okey_value(mm[2 * c + 1]);
  double v[5];
  v[0] = median[c];
  v[1] = dmin;
  v[2] = dmax;
  fit_scale(dmin, dmax, v[3], v[4]);
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    stats[q * n_num + c] = v[q];
    if (host_stats)
      __hip_atomic_store(host_stats + q * n_num + c, v[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(TT_NT) void tt_transform_kernel(const double* colmaj, const int32_t* row,
                                                             const int32_t* counts, int64_t M, int n_num,
                                                             const double* stats, float* num) {
  __shared__ double st[3][MAXC];   // median, scale_, min_
  if (threadIdx.x < n_num) {
    st[0][threadIdx.x] = stats[threadIdx.x];
    st[1][threadIdx.x] = stats[3 * n_num + threadIdx.x];
    st[2][threadIdx.x] = stats[4 * n_num + threadIdx.x];
  }
  __syncthreads();
  const int64_t n = min((int64_t)counts[0], M);
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t j = t0; j < n; j += step) {
    const int64_t i = row[j];
    if (i < 0 || i >= M) continue;
    for (int c = 0; c < n_num; ++c) {
      double x = colmaj[(int64_t)c * M + i];
      if (is_nan(x)) x = st[0][c];
      num[j * n_num + c] = scaled(x, st[1][c], st[2][c]);
    }
  }
}

// ------------------------------------------------------------ ids and cats
// rec[j] = (src[row[j]][off] ^ flip, j) for the surviving rows; the others dead
__global__ __launch_bounds__(TT_NT) void tt_records_kernel(const int64_t* src, int stride, int off, uint64_t flip,
                                                           const int32_t* row, const int32_t* counts, int64_t M,
                                                           TRec* rec) {
  const int64_t n = min((int64_t)counts[0], M);
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t j = t0; j < M; j += step) {
    TRec r;
    r.j = (uint32_t)j;
    if (j < n) {
      int64_t i = row[j];
      if (i < 0 || i >= M) i = 0;
      r.key = (uint64_t)src[i * stride + off] ^ flip;
      r.dead = 0u;
    } else {
      r.key = ~0ull;
      r.dead = 1u;
    }
    rec[j] = r;
  }
}

// ids: a [i] = head ? i : 0 (max scan: every record's head), b [j] = row j is
// its id's first row (sum scan: the codes).  cats: a [i] = head (sum scan).
template <bool IDS>
__global__ __launch_bounds__(TT_NT) void tt_heads_kernel(const TRec* rec, const int32_t* counts, int64_t M,
                                                         uint32_t* a, uint32_t* b) {
  const int64_t n = min((int64_t)counts[0], M);
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < n; i += step) {
    const TRec r = rec[i];
    const bool head = i == 0 || rec[i - 1].key != r.key;
    if (IDS) {
      a[i] = head ? (uint32_t)i : 0u;
      if ((int64_t)r.j < n) b[r.j] = head ? 1u : 0u;
    } else {
      a[i] = head ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(TT_NT) void tt_id_codes_kernel(const TRec* rec, const uint32_t* headidx,
                                                            const uint32_t* code1, const int32_t* counts,
                                                            int64_t M, int col, uint64_t flip, int64_t* collab,
                                                            int64_t* ids, int32_t* count_out) {
  const int64_t n = min((int64_t)counts[0], M);
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < n; i += step) {
    const TRec r = rec[i];
    int64_t h = headidx[i];
    if (h >= n) h = i;
    int64_t hj = rec[h].j;
    if (hj >= n) hj = 0;
    int64_t code = (int64_t)code1[hj] - 1;
    if (code < 0 || code >= n) code = 0;   // (cannot happen; keeps every store in bounds)
    if ((int64_t)r.j < n) collab[(int64_t)r.j * 2 + col] = code;
    if (h == i) ids[code] = (int64_t)(r.key ^ flip);
    if (i == n - 1) *count_out = (int32_t)code1[n - 1];
  }
}

__global__ __launch_bounds__(TT_NT) void tt_cat_codes_kernel(const TRec* rec, const uint32_t* rank1,
                                                             const int32_t* counts, int64_t M, int n_cat, int col,
                                                             int64_t* cat, int64_t* keys, int32_t* count_out) {
  const int64_t n = min((int64_t)counts[0], M);
  const int64_t t0 = (int64_t)blockIdx.x * TT_NT + threadIdx.x, step = (int64_t)gridDim.x * TT_NT;
  for (int64_t i = t0; i < n; i += step) {
    const TRec r = rec[i];
    int64_t code = (int64_t)rank1[i] - 1;
    if (code < 0 || code >= n) code = 0;
    if ((int64_t)r.j < n) cat[(int64_t)r.j * n_cat + col] = code;
    if (i == 0 || rec[i - 1].key != r.key) keys[code] = (int64_t)r.key;
    if (i == n - 1) *count_out = (int32_t)rank1[i];
  }
}

// ------------------------------------------------------------------- host
struct Plan {
  int units; int64_t chunk;   // sort units and records per unit
  int blocks, colb;           // of the grid-stride kernels; per column of the column passes
};

Plan make_plan(int64_t M) {
  Plan p;
  p.units = (int)std::min<int64_t>(MAX_UNITS, std::max<int64_t>(1, cdiv(M, UNIT_KEYS)));
  p.chunk = rup(cdiv(M, p.units), WAVE);
  p.blocks = (int)std::min<int64_t>(TT_MAXB, std::max<int64_t>(1, cdiv(M, TT_NT)));
  p.colb = (int)std::min<int64_t>(TT_COLB, std::max<int64_t>(1, cdiv(M, TT_NT)));
  return p;
}

struct Ws {
  double* colmaj;      // [n_num][M]
  TRec *ra, *rb;       // [M] each
  uint32_t *sa, *sb;   // [M] each: scan arrays
  uint8_t* flags;      // [M]
  uint32_t* tile_tot;  // [scan_tiles(M)]
  uint32_t* scounts;   // [units][NB]
  uint32_t* stot;      // [NB]
  uint32_t* ghist;     // [n_num][2][NB]
  uint64_t* sel;       // [n_num][4]
  uint64_t* mm;        // [n_num][2]
  double* median;      // [n_num]
  size_t total;
};

Ws carve(const Plan& p, int64_t M, int n_num, void* base) {
  Bump b(base);
  Ws w;
  w.colmaj = (double*)b.take((size_t)M * n_num * 8);
  w.ra = (TRec*)b.take((size_t)M * sizeof(TRec));
  w.rb = (TRec*)b.take((size_t)M * sizeof(TRec));
  w.sa = (uint32_t*)b.take((size_t)M * 4);
  w.sb = (uint32_t*)b.take((size_t)M * 4);
  w.flags = (uint8_t*)b.take((size_t)M);
  w.tile_tot = (uint32_t*)b.take((size_t)scan_tiles(M) * 4);
  w.scounts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.stot = (uint32_t*)b.take((size_t)NB * 4);
  w.ghist = (uint32_t*)b.take((size_t)std::max(1, n_num) * 2 * NB * 4);
  w.sel = (uint64_t*)b.take((size_t)std::max(1, n_num) * 32);
  w.mm = (uint64_t*)b.take((size_t)std::max(1, n_num) * 16);
  w.median = (double*)b.take((size_t)std::max(1, n_num) * 8);
  w.total = b.off;
  return w;
}

}  // namespace

static size_t train_table_ws_bytes(int64_t M, int n_num) {
  return carve(make_plan(M), M, n_num, nullptr).total;
}

static dcnr_status train_table_build(const dcnr_train_table_args& a, void* ws, hipStream_t s) {
  const int64_t M = a.M;
  const int n_cat = a.n_cat, n_raw = a.n_raw, n_num = a.n_raw + a.n_derived;
  const int n_counts = DCNR_TRAIN_TABLE_COUNTS + n_cat;
  const Plan p = make_plan(M);
  const Ws w = carve(p, M, n_num, ws);
  const Derived dv = derived_pack(a.derived, a.n_derived);
  const int64_t n_hist = (int64_t)n_num * 2 * NB;
  hipLaunchKernelGGL(tt_init_kernel, dim3((unsigned)std::max<int64_t>(1, cdiv(std::max<int64_t>(n_hist, 512), TT_NT))),
                     dim3(TT_NT), 0, s, a.counts, n_counts, w.ghist, n_hist, w.sel, n_num, w.mm);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(tt_rows_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, a.cat_key, a.raw, M, n_cat, n_raw,
                     a.filter_col, a.filter_lo, a.filter_hi, dv, w.colmaj, w.flags, w.sa, a.counts);
  DCNR_LAUNCH_CHECK();
  TRY(scan_inplace<false>(w.sa, nullptr, M, w.tile_tot, s));
  hipLaunchKernelGGL(tt_emit_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, (const uint8_t*)w.flags,
                     (const uint32_t*)w.sa, a.target, M, a.row, a.y, a.counts);
  DCNR_LAUNCH_CHECK();
  if (n_num > 0) {
    for (int ps = 0; ps < SEL_PASSES; ++ps) {
      hipLaunchKernelGGL(tt_sel_hist_kernel, dim3(p.colb, n_num), dim3(TT_NT), 0, s, (const double*)w.colmaj,
                         (const uint8_t*)w.flags, M, ps, (const uint64_t*)w.sel, w.ghist);
      DCNR_LAUNCH_CHECK();
      hipLaunchKernelGGL(tt_sel_pick_kernel, dim3(n_num), dim3(TT_NT), 0, s, ps, w.sel, w.ghist, w.median);
      DCNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(tt_minmax_kernel, dim3(p.colb, n_num), dim3(TT_NT), 0, s, (const double*)w.colmaj,
                       (const uint8_t*)w.flags, M, (const double*)w.median, w.mm, a.counts);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tt_stats_kernel, dim3(1), dim3(MAXC), 0, s, (const uint64_t*)w.mm,
                       (const double*)w.median, n_num, a.stats, a.host_stats);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(tt_transform_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, (const double*)w.colmaj,
                       (const int32_t*)a.row, (const int32_t*)a.counts, M, n_num, (const double*)a.stats, a.num);
    DCNR_LAUNCH_CHECK();
  }
  for (int col = 0; col < 2 + n_cat; ++col) {
    const bool ids = col < 2;
    const uint64_t flip = ids ? SIGN : 0ull;
    TRec *src = w.ra, *dst = w.rb;
    if (ids)
      hipLaunchKernelGGL(tt_records_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, col ? a.item : a.user, 1, 0, flip,
                         (const int32_t*)a.row, (const int32_t*)a.counts, M, src);
    else
      hipLaunchKernelGGL(tt_records_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, a.cat_key, n_cat, col - 2, flip,
                         (const int32_t*)a.row, (const int32_t*)a.counts, M, src);
    DCNR_LAUNCH_CHECK();
    // the records by (dead, key), stable: a head is its key's first row
    TRY(sort_passes(src, dst, M, p.units, p.chunk, 0, REC_PASSES, w.scounts, w.stot, nullptr, s));
    if (ids) {
      hipLaunchKernelGGL(tt_heads_kernel<true>, dim3(p.blocks), dim3(TT_NT), 0, s, (const TRec*)src,
                         (const int32_t*)a.counts, M, w.sa, w.sb);
      DCNR_LAUNCH_CHECK();
      TRY(scan_inplace<true>(w.sa, a.counts, M, w.tile_tot, s));
      TRY(scan_inplace<false>(w.sb, a.counts, M, w.tile_tot, s));
      hipLaunchKernelGGL(tt_id_codes_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, (const TRec*)src,
                         (const uint32_t*)w.sa, (const uint32_t*)w.sb, (const int32_t*)a.counts, M, col, flip,
                         a.collab, col ? a.item_ids : a.user_ids, a.counts + 1 + col);
    } else {
      hipLaunchKernelGGL(tt_heads_kernel<false>, dim3(p.blocks), dim3(TT_NT), 0, s, (const TRec*)src,
                         (const int32_t*)a.counts, M, w.sa, w.sb);
      DCNR_LAUNCH_CHECK();
      TRY(scan_inplace<false>(w.sa, a.counts, M, w.tile_tot, s));
      hipLaunchKernelGGL(tt_cat_codes_kernel, dim3(p.blocks), dim3(TT_NT), 0, s, (const TRec*)src,
                         (const uint32_t*)w.sa, (const int32_t*)a.counts, M, n_cat, col - 2, a.cat,
                         a.cat_keys + (int64_t)(col - 2) * M, a.counts + DCNR_TRAIN_TABLE_COUNTS + (col - 2));
    }
    DCNR_LAUNCH_CHECK();
  }
  if (a.host_counts) TRY(mirror_words(a.counts, n_counts, a.host_counts, s));
  return DCNR_OK;
}

}  // namespace dcnr

using namespace dcnr;

extern "C" {

static dcnr_status train_table_shape(int64_t M, int32_t n_cat, int32_t n_raw, int32_t n_derived) {
  if (M < 0 || n_cat < 0 || n_raw < 0 || n_derived < 0) return DCNR_BAD_ARG;
  if (M >= 2147483647ll || n_cat > 64 || (int64_t)n_raw + n_derived > MAXC) return DCNR_UNSUPPORTED_SHAPE;
  return DCNR_OK;
}

size_t dcnr_train_table_workspace_size(int64_t M, int32_t n_cat, int32_t n_raw, int32_t n_derived) {
  if (train_table_shape(M, n_cat, n_raw, n_derived) != DCNR_OK) return 0;
  return train_table_ws_bytes(M, n_raw + n_derived) + 256;
}

dcnr_status dcnr_train_table_build(const dcnr_train_table_args* a, void* ws, size_t ws_bytes,
                                   dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!a) {
    set_error("dcnr_train_table_build: null args");
    return DCNR_BAD_ARG;
  }
  const dcnr_status shape = train_table_shape(a->M, a->n_cat, a->n_raw, a->n_derived);
  bool bad = shape == DCNR_BAD_ARG || !a->counts || a->filter_col < -1 ||
             (a->filter_col >= 0 && a->filter_col >= a->n_raw) || !derived_ok(a->derived, a->n_derived, a->n_raw);
  if (!bad && a->M > 0) {
    const bool num = a->n_raw + a->n_derived > 0;
    bad = !a->user || !a->item || !a->target || !ws || (a->n_cat > 0 && (!a->cat_key || !a->cat || !a->cat_keys)) ||
          (a->n_raw > 0 && !a->raw) || (num && (!a->num || !a->stats)) || !a->row || !a->collab || !a->y ||
          !a->user_ids || !a->item_ids;
  }
  if (bad) {
    set_error("dcnr_train_table_build: bad argument (M=%lld, n_cat=%d, n_raw=%d, n_derived=%d, filter_col=%d)",
              (long long)a->M, a->n_cat, a->n_raw, a->n_derived, a->filter_col);
    return DCNR_BAD_ARG;
  }
  if (shape != DCNR_OK) {
    set_error("dcnr_train_table_build: unsupported shape (M=%lld, n_cat=%d, n_raw=%d, n_derived=%d)",
              (long long)a->M, a->n_cat, a->n_raw, a->n_derived);
    return shape;
  }
  if (a->M == 0) return zero_counts(a->counts, a->host_counts, DCNR_TRAIN_TABLE_COUNTS + a->n_cat, s);
  const size_t need = train_table_ws_bytes(a->M, a->n_raw + a->n_derived) + 256;
  if (ws_bytes < need) {
    set_error("dcnr_train_table_build: workspace too small: %zu < %zu", ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TRYP(DCNR_K_SERVE, s, train_table_build(*a, ws_align(ws), s));
  return DCNR_OK;
}

}  // extern "C"
