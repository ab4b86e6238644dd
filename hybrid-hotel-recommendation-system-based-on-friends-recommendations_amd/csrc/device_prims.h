// Device building blocks of the data-preparation files (metrics.hip,
// city_sets.hip, item_features.hip, train_table.hip, transform.hip): the stable
// radix sort, the tiled scan, the row arithmetic of the fitted preprocessing and
// the tails their entry points share.  One copy of each: prepare_data,
// Preprocessor.transform and ItemFeatures agree bit for bit because they run
// the same functions.  Kernels are templates, or static where they are not.
#pragma once
#include "dcnr_internal.h"

namespace dcnr {

// ---------------------------------------------------------------------------
// The stable LSD radix sort: passes of RBITS bits over records T, a 64-bit key
// or a struct with its own radix_digit (found by argument-dependent lookup).
// A "unit" is the contiguous run of records one wave walks 64 at a time; per
// pass: per-unit digit counts, a scan over (digit, unit), a stable scatter that
// ranks equal digits within a wave by match-any over ballots (no atomics: the
// order within a digit is the input's).  The scan needs tot [NB], the digit
// totals of the whole input: a digit histogram does not depend on the order of
// the records, so a caller may count all its passes in one sweep beforehand
// (metrics.hip) or have every pass sum the unit counts (sort_tot_kernel).
namespace rsort {

constexpr int RBITS = 11;                                  // digit width
constexpr int NB = 1 << RBITS;                             // buckets per pass
constexpr int UNIT_KEYS = 4096;                            // keys per unit before MAX_UNITS binds
constexpr int MAX_UNITS = 1024;
constexpr int SORT_NT = 256, SORT_WAVES = SORT_NT / WAVE;  // 4 units per block
constexpr int SORT_UNROLL = 4;                             // 64-key steps loaded ahead
constexpr int SCAN_NT = 1024, SCAN_SEG = SCAN_NT / WAVE;   // 64 buckets x 16 unit segments

__device__ __forceinline__ uint32_t radix_digit(uint64_t k, int shift) {
  return (uint32_t)((k >> shift) & (NB - 1));
}

// counts[u][d] = keys of unit u whose digit is d
template <typename T>
__global__ __launch_bounds__(SORT_NT) void sort_hist_kernel(const T* keys, int64_t n, int units,
                                                            int64_t chunk, int shift, uint32_t* counts) {
  __shared__ uint32_t h[SORT_WAVES][NB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * SORT_WAVES + w;
  for (int d = lane; d < NB; d += WAVE) h[w][d] = 0u;
  __syncthreads();
  if (u < units) {
    const int64_t lo = (int64_t)u * chunk, hi = min(n, lo + chunk);
    for (int64_t i0 = lo + lane; i0 < hi; i0 += SORT_UNROLL * WAVE) {
      T k[SORT_UNROLL];
#pragma unroll
      for (int q = 0; q < SORT_UNROLL; ++q) k[q] = i0 + q * WAVE < hi ? keys[i0 + q * WAVE] : T{};
#pragma unroll
      for (int q = 0; q < SORT_UNROLL; ++q)
        if (i0 + q * WAVE < hi) atomicAdd(&h[w][(int)radix_digit(k[q], shift)], 1u);
    }
  }
  __syncthreads();
  if (u < units)
    for (int d = lane; d < NB; d += WAVE) counts[(int64_t)u * NB + d] = h[w][d];
}

// tot[d] = the sum over the units of counts[u][d] (before sort_scan_kernel
// overwrites the counts): one workgroup per 64 digits, thread (j, s) sums digit
// b0 + j over unit segment s.  (Eight workgroups that each walked all the units
// took 156 us a pass at 1024 units, half of dcnr_train_table_build's time.)
static __global__ __launch_bounds__(SCAN_NT) void sort_tot_kernel(const uint32_t* counts, int units,
                                                                  uint32_t* tot) {
  __shared__ uint32_t seg[SCAN_SEG][WAVE];
  const int j = threadIdx.x & 63, s = threadIdx.x >> 6, b0 = blockIdx.x * WAVE;
  const int useg = (units + SCAN_SEG - 1) / SCAN_SEG;
  const int u0 = min(units, s * useg), u1 = min(units, u0 + useg);
  uint32_t t = 0u;
  for (int u = u0; u < u1; ++u) t += counts[(int64_t)u * NB + b0 + j];
  seg[s][j] = t;
  __syncthreads();
  if (s == 0) {
    uint32_t sum = 0u;
    for (int k = 0; k < SCAN_SEG; ++k) sum += seg[k][j];
    tot[b0 + j] = sum;
  }
}

// counts[u][d] -> first output position of unit u's keys of digit d: the keys
// of lower digits (tot), then the lower units' keys of digit d.  One block
// per 64 digits; thread (j, s) walks digit b0 + j over unit segment s.
static __global__ __launch_bounds__(SCAN_NT) void sort_scan_kernel(const uint32_t* tot, uint32_t* counts,
                                                                   int units) {
  __shared__ uint32_t red[SCAN_SEG];
  __shared__ uint32_t tl[WAVE];
  __shared__ uint32_t seg[SCAN_SEG][WAVE];
  const int tid = threadIdx.x, j = tid & 63, s = tid >> 6;
  const int b0 = blockIdx.x * WAVE;
  uint32_t a = 0u;
  for (int d = tid; d < b0; d += SCAN_NT) a += tot[d];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) a += (uint32_t)__shfl_xor((int)a, o, 64);
  if (j == 0) red[s] = a;
  if (tid < WAVE) tl[tid] = tot[b0 + tid];
  const int useg = (units + SCAN_SEG - 1) / SCAN_SEG;
  const int u0 = min(units, s * useg), u1 = min(units, u0 + useg);
  uint32_t t = 0u;
  for (int u = u0; u < u1; ++u) t += counts[(int64_t)u * NB + b0 + j];
  seg[s][j] = t;
  __syncthreads();
  uint32_t base = 0u;
  for (int k = 0; k < SCAN_SEG; ++k) base += red[k];
  for (int k = 0; k < j; ++k) base += tl[k];
  for (int k = 0; k < s; ++k) base += seg[k][j];
  for (int u = u0; u < u1; ++u) {
    const int64_t idx = (int64_t)u * NB + b0 + j;
    const uint32_t c = counts[idx];
    counts[idx] = base;
    base += c;
  }
}

// Stable scatter of one pass.  A wave walks its unit 64 keys at a time; the
// lanes holding the same digit find each other with RBITS ballots, the lowest
// of them advances the unit's offset of that digit by their number, and each
// writes at offset + (equal-digit lanes below it).
template <typename T>
__global__ __launch_bounds__(SORT_NT) void sort_scatter_kernel(const T* in, T* out, int64_t n, int units,
                                                               int64_t chunk, int shift,
                                                               const uint32_t* counts) {
  __shared__ uint32_t c[SORT_WAVES][NB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * SORT_WAVES + w;
  if (u < units)
    for (int d = lane; d < NB; d += WAVE) c[w][d] = counts[(int64_t)u * NB + d];
  __syncthreads();
  if (u >= units) return;
  const uint64_t lt = (1ull << lane) - 1ull;
  const int64_t lo = (int64_t)u * chunk, hi = min(n, lo + chunk);
  for (int64_t i0 = lo; i0 < hi; i0 += SORT_UNROLL * WAVE) {   // wave-uniform trip count
    // the loads of SORT_UNROLL steps up front (the walk is latency-bound: one
    // dependent chain through the unit's LDS offsets), then the steps in order
    T keys[SORT_UNROLL];
    bool valids[SORT_UNROLL];
#pragma unroll
    for (int q = 0; q < SORT_UNROLL; ++q) {
      const int64_t i = i0 + q * WAVE + lane;
      valids[q] = i < hi;
      keys[q] = valids[q] ? in[i] : T{};
    }
#pragma unroll
    for (int q = 0; q < SORT_UNROLL; ++q) {
      const bool valid = valids[q];
      const T key = keys[q];
      const uint32_t d = radix_digit(key, shift);
      uint64_t mask = __ballot(valid);
#pragma unroll
      for (int b = 0; b < RBITS; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bal = __ballot(bit);
        mask &= bit ? bal : ~bal;
      }
      const int leader = valid ? __ffsll((unsigned long long)mask) - 1 : lane;
      uint32_t pre = 0u;
      if (valid && lane == leader) {
        pre = c[w][d];
        c[w][d] = pre + (uint32_t)__popcll(mask);
      }
      pre = (uint32_t)__shfl((int)pre, leader, 64);
      if (valid) {
        const uint32_t pos = pre + (uint32_t)__popcll(mask & lt);
        if ((int64_t)pos < n) out[pos] = key;
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// npass passes over bits [shift0, shift0 + npass * RBITS) of the n records in
// `units` units of `chunk` records; src ends as the sorted array.  counts
// [units][NB] is scratch.  pre_tot [npass][NB]: the digit totals of every pass,
// counted by the caller; null: each pass sums its unit counts into tot [NB].
template <typename T>
dcnr_status sort_passes(T*& src, T*& dst, int64_t n, int units, int64_t chunk, int shift0, int npass,
                        uint32_t* counts, uint32_t* tot, const uint32_t* pre_tot, hipStream_t s) {
  const int sort_blocks = (int)cdiv(units, SORT_WAVES);
  for (int ps = 0; ps < npass; ++ps) {
    const int shift = shift0 + ps * RBITS;
    hipLaunchKernelGGL(sort_hist_kernel<T>, dim3(sort_blocks), dim3(SORT_NT), 0, s, (const T*)src, n, units, chunk,
                       shift, counts);
    DCNR_LAUNCH_CHECK();
    if (!pre_tot) {
      hipLaunchKernelGGL(sort_tot_kernel, dim3(NB / WAVE), dim3(SCAN_NT), 0, s, (const uint32_t*)counts, units, tot);
      DCNR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sort_scan_kernel, dim3(NB / WAVE), dim3(SCAN_NT), 0, s,
                       pre_tot ? pre_tot + ps * NB : (const uint32_t*)tot, counts, units);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_scatter_kernel<T>, dim3(sort_blocks), dim3(SORT_NT), 0, s, (const T*)src, dst, n, units,
                       chunk, shift, (const uint32_t*)counts);
    DCNR_LAUNCH_CHECK();
    std::swap(src, dst);
  }
  return DCNR_OK;
}

}  // namespace rsort

// ---------------------------------------------------------------------------
// The tiled scan of a uint32 array, a sum or a max: tile sums, one workgroup
// over the tile sums, tiles again.  A row's output position is the number of
// kept rows before it -- no atomic decides a position.
namespace tscan {

constexpr int TS_NT = 256;
constexpr int TS_TILE = TS_NT * 4;            // elements per scan tile
constexpr int TS_SCAN_NT = 1024;

inline int64_t scan_tiles(int64_t M) { return std::max<int64_t>(1, cdiv(M, TS_TILE)); }

template <bool MAX>
__device__ __forceinline__ uint32_t comb(uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; }

// inclusive scan over the workgroup (sum, or max); sm holds NT / 64 words
template <bool MAX, int NT>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* sm, uint32_t& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)v, o, 64);
    if (lane >= o) v = comb<MAX>(v, t);
  }
  if (lane == 63) sm[w] = v;
  __syncthreads();
  uint32_t pre = 0u;
  total = 0u;
  for (int k = 0; k < NT / 64; ++k) {
    if (k < w) pre = comb<MAX>(pre, sm[k]);
    total = comb<MAX>(total, sm[k]);
  }
  __syncthreads();
  return comb<MAX>(pre, v);
}

// a [M] -> its inclusive scan in place over the first n = *np (or M) elements
template <bool MAX>
__global__ __launch_bounds__(TS_NT) void tile_sum_kernel(const uint32_t* a, const int32_t* np, int64_t M,
                                                         uint32_t* tile_tot) {
  __shared__ uint32_t sm[TS_NT / 64];
  const int64_t n = np ? min((int64_t)*np, M) : M;
  const int64_t i0 = (int64_t)blockIdx.x * TS_TILE + threadIdx.x * 4;
  uint32_t v = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (i0 + q < n) v = comb<MAX>(v, a[i0 + q]);
  uint32_t total;
  block_scan<MAX, TS_NT>(v, sm, total);
  if (threadIdx.x == 0) tile_tot[blockIdx.x] = total;
}

// tile_tot [tiles] -> its exclusive scan in place (one workgroup)
template <bool MAX>
__global__ __launch_bounds__(TS_SCAN_NT) void tile_scan_kernel(uint32_t* tile_tot, int64_t tiles) {
  __shared__ uint32_t sm[TS_SCAN_NT / 64];
  uint32_t carry = 0u;
  for (int64_t t0 = 0; t0 < tiles; t0 += TS_SCAN_NT) {   // uniform trip count
    const int64_t t = t0 + threadIdx.x;
    const uint32_t v = t < tiles ? tile_tot[t] : 0u;
    uint32_t total;
    const uint32_t inc = block_scan<MAX, TS_SCAN_NT>(v, sm, total);
    // exclusive: what lies before this tile
    uint32_t before = (uint32_t)__shfl_up((int)inc, 1, 64);
    __shared__ uint32_t last[TS_SCAN_NT / 64];
    if ((threadIdx.x & 63) == 63) last[threadIdx.x >> 6] = inc;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) before = threadIdx.x ? last[(threadIdx.x >> 6) - 1] : 0u;
    if (t < tiles) tile_tot[t] = comb<MAX>(carry, before);
    carry = comb<MAX>(carry, total);
    __syncthreads();
  }
}

template <bool MAX>
__global__ __launch_bounds__(TS_NT) void tile_apply_kernel(uint32_t* a, const int32_t* np, int64_t M,
                                                           const uint32_t* tile_tot) {
  __shared__ uint32_t sm[TS_NT / 64];
  const int64_t n = np ? min((int64_t)*np, M) : M;
  const int64_t i0 = (int64_t)blockIdx.x * TS_TILE + threadIdx.x * 4;
  uint32_t x[4];
  uint32_t v = 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[q] = i0 + q < n ? a[i0 + q] : 0u;
    v = comb<MAX>(v, x[q]);
  }
  uint32_t total;
  const uint32_t inc = block_scan<MAX, TS_NT>(v, sm, total);
  // what lies before this lane's four: the tile's base and the lanes below
  uint32_t before = (uint32_t)__shfl_up((int)inc, 1, 64);
  __shared__ uint32_t last[TS_NT / 64];
  if ((threadIdx.x & 63) == 63) last[threadIdx.x >> 6] = inc;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) before = threadIdx.x ? last[(threadIdx.x >> 6) - 1] : 0u;
  uint32_t run = comb<MAX>(tile_tot[blockIdx.x], before);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    run = comb<MAX>(run, x[q]);
    if (i0 + q < n) a[i0 + q] = run;
  }
}

// tile_tot: scan_tiles(M) words of scratch
template <bool MAX>
dcnr_status scan_inplace(uint32_t* a, const int32_t* np, int64_t M, uint32_t* tile_tot, hipStream_t s) {
  const int64_t tiles = scan_tiles(M);
  hipLaunchKernelGGL(tile_sum_kernel<MAX>, dim3((unsigned)tiles), dim3(TS_NT), 0, s, (const uint32_t*)a, np, M,
                     tile_tot);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(tile_scan_kernel<MAX>, dim3(1), dim3(TS_SCAN_NT), 0, s, tile_tot, tiles);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(tile_apply_kernel<MAX>, dim3((unsigned)tiles), dim3(TS_NT), 0, s, a, np, M,
                     (const uint32_t*)tile_tot);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // namespace tscan

// ---------------------------------------------------------------------------
// Row arithmetic of the fitted preprocessing
constexpr uint64_t SIGN = 0x8000000000000000ull;
constexpr int MAXC = 64;                      // numeric columns, raw and derived

// (integer tests: no arithmetic that could flush a denormal or quiet a NaN)
__device__ __forceinline__ bool is_nan(double x) {
  return ((uint64_t)__double_as_longlong(x) & ~SIGN) > 0x7FF0000000000000ull;
}
__device__ __forceinline__ bool is_inf(double x) {
  return ((uint64_t)__double_as_longlong(x) & ~SIGN) == 0x7FF0000000000000ull;
}

// MinMaxScaler.transform and torch's float32 conversion: X *= scale_; X += min_
// in float64, two separately rounded operations, then one rounding to float32
// (to nearest even) -- never an fma.  hipcc contracts x * s + m into an fma by
// default, so contraction is off for this function (this ROCm has no __dmul_rn
// / __dadd_rn).  NaN payloads, +-inf and -0.0 go through v_mul_f64 / v_add_f64
// / v_cvt_f32_f64 as numpy's float64 operations and its float32 cast pass them.
__device__ __forceinline__ float scaled(double x, double scale, double mn) {
#pragma clang fp contract(off)
  double y = x * scale;
  y = y + mn;
  return (float)y;
}

// the derived columns, unpacked from the ABI's triples {op, a, b}
struct Derived { int n; int op[MAXC], a[MAXC], b[MAXC]; };

inline Derived derived_pack(const int32_t* triples, int n) {
  Derived dv = {};
  dv.n = n;
  for (int d = 0; d < n; ++d) {
    dv.op[d] = triples[3 * d];
    dv.a[d] = triples[3 * d + 1];
    dv.b[d] = triples[3 * d + 2];
  }
  return dv;
}

// every triple names a known operation and two raw columns
inline bool derived_ok(const int32_t* triples, int n_derived, int n_raw) {
  if (n_derived > 0 && !triples) return false;
  bool ok = true;
  for (int d = 0; d < n_derived; ++d) {
    const int32_t op = triples[3 * d], i = triples[3 * d + 1], j = triples[3 * d + 2];
    ok &= (op == DCNR_DERIVED_RATIO || op == DCNR_DERIVED_DIFF) && i >= 0 && i < n_raw && j >= 0 && j < n_raw;
  }
  return ok;
}

// derived column d of a raw row: a / b with +-inf and NaN read as 0, or a - b
__device__ __forceinline__ double derived_value(const Derived& dv, int d, const double* row) {
  const double a = row[dv.a[d]], b = row[dv.b[d]];
  double v;
  if (dv.op[d] == DCNR_DERIVED_RATIO) {
    v = a / b;
    if (is_inf(v) || is_nan(v)) v = 0.0;
  } else {
    v = a - b;
  }
  return v;
}

// ---------------------------------------------------------------------------
// Entry-point tails
// the workspace from its first 256-byte boundary (the sizes count 256 bytes for it)
inline void* ws_align(void* ws) { return (void*)(((uintptr_t)ws + 255) & ~(uintptr_t)255); }

// a call without rows: n count words of zeros, on the device and in their mirror
inline dcnr_status zero_counts(int32_t* counts, int32_t* host_counts, int n, hipStream_t s) {
  DCNR_HIP(hipMemsetAsync(counts, 0, (size_t)n * 4, s));
  if (host_counts)
    for (int i = 0; i < n; ++i) host_counts[i] = 0;
  return DCNR_OK;
}

}  // namespace dcnr
