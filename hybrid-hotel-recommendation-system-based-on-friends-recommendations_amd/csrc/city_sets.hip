// City and popular-hotel sets of the /recommendations request (main.py:204-210)
// from the review rows, on the device (dcnr_city_sets_build).
//
// Per main_df row: hotel row, city code, popularity key (user_reviews_count,
// float64) and the row's main_df number (ascending, so position order is row
// order).  Per city c: city(c), the distinct hotel rows; top_rows(c), the first
// `top` rows by (key descending, NaN last, row ascending); popular(c), the
// distinct hotel rows of top_rows(c).
//
//   records   one 16-byte record per row: (~orderable(key), city, position);
//             items, cities and the row order are validated here
//   sort A    the shared stable LSD radix sort (device_prims.h) over the 64 +
//             bits(C - 1) bits of (city, key): every city becomes one segment in
//             served order; ties keep the input's order, which is the rows'
//   bounds    the segments' ends, one lane per sorted record
//   popular   one workgroup per city over its first `top` records: top_rows,
//             and the distinct hotels among them ranked by counting in LDS
//   keys      one 64-bit key per row, city << bits(n_items - 1) | hotel
//   sort B    the same sort, keys only, over bits(C - 1) + bits(n_items - 1) bits
//   heads     a key that differs from its predecessor is a city's next distinct
//             hotel: per-tile head counts, one scan of the tiles, then every
//             head is written at its global rank, which is its place in the
//             CSR because the city sets come first and in city order
//   offsets   one workgroup: the exclusive sum of the 2C set lengths, the
//             overflow bit, the mirrors
//   copy      popular(c) to its place behind the city sets
//
// Nothing depends on how the rows are spread over the cities: a city that
// holds every row is sorted by the whole machine like any other table.  Every
// count is an integer and every output word is written by one lane: the same
// bits on every run.  Workspace: two 16-byte records per row, the sort's unit
// counts, 4 * C * (top + 5) bytes of per-city words and one word per tile.
#include "device_prims.h"

namespace dcnr {

namespace {

using namespace rsort;

constexpr int CS_NT = 256;
constexpr int CS_MAXB = 2048;            // workgroups of the grid-stride kernels
constexpr int CS_TILE_Q = 8;             // a tile of the head kernels: CS_TILE_Q rounds of CS_NT keys
constexpr int CS_TILE = CS_NT * CS_TILE_Q;
constexpr int CS_SCAN_NT = 1024;         // (one lane per run in cs_offsets_kernel)
constexpr int CS_TOP_MAX = 256;          // (one lane per top row in cs_popular_kernel)

struct alignas(16) Rec {
  uint64_t lo;    // ~orderable(key): ascending = key descending, NaN last
  uint32_t hi;    // city
  uint32_t pay;   // position
};

// the digit at `shift` of the 96-bit value hi : lo
__device__ __forceinline__ uint32_t radix_digit(const Rec& r, int shift) {
  if (shift >= 64) return (r.hi >> (shift - 64)) & (uint32_t)(NB - 1);
  uint64_t v = r.lo >> shift;
  if (shift > 64 - RBITS) v |= (uint64_t)r.hi << (64 - shift);
  return (uint32_t)v & (uint32_t)(NB - 1);
}

int bits_of(int64_t n) {   // bits that hold 0 .. n - 1
  int b = 0;
  while (b < 62 && ((int64_t)1 << b) < n) ++b;
  return b;
}

struct Plan {
  int units; int64_t chunk;     // sort units and records per unit (a multiple of 64)
  int ibits, pass_a, pass_b;    // bits of a hotel row, passes of the two sorts
  int64_t tiles;
  int blocks;                   // of the grid-stride kernels
};

Plan make_plan(int64_t M, int64_t n_items, int C) {
  Plan p;
  p.units = (int)std::min<int64_t>(MAX_UNITS, std::max<int64_t>(1, cdiv(M, UNIT_KEYS)));
  p.chunk = rup(cdiv(M, p.units), WAVE);
  const int cbits = bits_of(C);
  p.ibits = bits_of(n_items);
  p.pass_a = (int)cdiv(64 + cbits, RBITS);
  p.pass_b = (int)std::max<int64_t>(1, cdiv(cbits + p.ibits, RBITS));
  p.tiles = cdiv(M, CS_TILE);
  p.blocks = (int)std::min<int64_t>(CS_MAXB, std::max<int64_t>(1, cdiv(M, CS_NT)));
  return p;
}

struct Ws {
  Rec *ra, *rb;           // [M] record ping-pong; sort B's keys live in the same memory
  uint32_t* counts;       // [units][NB]
  uint32_t* tot;          // [NB]
  uint32_t* cwords;       // [4][C] zeroed: cstart, cend (sorted records), cfirst, clast (set_rows)
  uint32_t* popcount;     // [C]
  int32_t* popitems;      // [C][top]
  uint32_t* tilebase;     // [tiles]
  size_t total;
};

Ws carve(const Plan& p, int64_t M, int C, int top, void* base) {
  Bump b(base);
  Ws w;
  w.ra = (Rec*)b.take((size_t)M * sizeof(Rec));
  w.rb = (Rec*)b.take((size_t)M * sizeof(Rec));
  w.counts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.tot = (uint32_t*)b.take((size_t)NB * 4);
  w.cwords = (uint32_t*)b.take((size_t)C * 16);
  w.popcount = (uint32_t*)b.take((size_t)C * 4);
  w.popitems = (int32_t*)b.take((size_t)C * top * 4);
  w.tilebase = (uint32_t*)b.take((size_t)std::max<int64_t>(1, p.tiles) * 4);
  w.total = b.off;
  return w;
}

// IEEE order as an unsigned order, descending, NaN behind everything: -0.0
// takes +0.0's key (integer test: no arithmetic that could flush a denormal)
__device__ __forceinline__ uint64_t desc_key(double x) {
  uint64_t u = (uint64_t)__double_as_longlong(x);
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return ~0ull;   // NaN
  if (u == 0x8000000000000000ull) u = 0ull;
  u ^= (u >> 63) ? ~0ull : 0x8000000000000000ull;
  return ~u;   // (all ones only for a NaN pattern)
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(CS_NT) void cs_records_kernel(const int32_t* item, const int32_t* city,
                                                           const double* key, const int32_t* row,
                                                           int64_t M, int64_t n_items, int C, Rec* out,
                                                           int32_t* status) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * CS_NT + threadIdx.x; i < M; i += (int64_t)gridDim.x * CS_NT) {
    const int c = city[i], h = item[i];
    bad |= c < 0 || c >= C || h < 0 || (int64_t)h >= n_items;
    if (row) bad |= row[i] <= (i ? row[i - 1] : -1);
    Rec r;
    r.lo = desc_key(key[i]);
    r.hi = (uint32_t)clampi(c, C - 1);
    r.pay = (uint32_t)i;
    out[i] = r;
  }
  if (bad) atomicOr(status, DCNR_REQ_BAD_DATA);
}

// cstart[c], cend[c]: city c's segment of the sorted records (both 0: no row)
__global__ __launch_bounds__(CS_NT) void cs_bounds_kernel(const Rec* r, int64_t M, uint32_t* cstart,
                                                          uint32_t* cend) {
  for (int64_t j = (int64_t)blockIdx.x * CS_NT + threadIdx.x; j < M; j += (int64_t)gridDim.x * CS_NT) {
    const uint32_t c = r[j].hi;   // (clamped into [0, C) by cs_records_kernel)
    if (j == 0 || r[j - 1].hi != c) cstart[c] = (uint32_t)j;
    if (j == M - 1 || r[j + 1].hi != c) cend[c] = (uint32_t)(j + 1);
  }
}

// One workgroup per city: top_rows[c][t], and the distinct hotels of those rows
// ascending in popitems[c][0 .. popcount[c]).  A row is kept if no earlier one
// names its hotel; its place is the number of kept hotels below it (both by
// counting over the LDS copy: every lane reads the same word, a broadcast).
__global__ __launch_bounds__(CS_TOP_MAX) void cs_popular_kernel(const Rec* r, const uint32_t* cstart,
                                                                const uint32_t* cend, const int32_t* item,
                                                                const int32_t* row, int64_t M,
                                                                int64_t n_items, int top, int32_t* top_rows,
                                                                int32_t* popitems, uint32_t* popcount) {
  __shared__ int it[CS_TOP_MAX];
  __shared__ int keep[CS_TOP_MAX];
  const int c = blockIdx.x, t = threadIdx.x;
  const int64_t e0 = min((int64_t)cend[c], M), s0 = min((int64_t)cstart[c], e0);
  const int n = (int)min((int64_t)top, e0 - s0);
  int h = 0;
  if (t < n) {
    const int64_t pos = min((int64_t)r[s0 + t].pay, M - 1);
    h = clampi(item[pos], (int)max((int64_t)0, n_items - 1));
    top_rows[(int64_t)c * top + t] = row ? row[pos] : (int32_t)pos;
    it[t] = h;
  } else if (t < top) {
    top_rows[(int64_t)c * top + t] = -1;
  }
  __syncthreads();
  bool first = t < n;
  for (int j = 0; j < t && first; ++j) first = it[j] != h;
  keep[t] = first;
  const int cnt = __syncthreads_count(first);
  if (first) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (keep[j] && it[j] < h) ? 1 : 0;
    popitems[(int64_t)c * top + rank] = h;
  }
  if (t == 0) popcount[c] = (uint32_t)cnt;
}

__global__ __launch_bounds__(CS_NT) void cs_keys_kernel(const int32_t* item, const int32_t* city, int64_t M,
                                                        int64_t n_items, int C, int ibits, uint64_t* keys) {
  const int hmax = (int)max((int64_t)0, n_items - 1);
  for (int64_t i = (int64_t)blockIdx.x * CS_NT + threadIdx.x; i < M; i += (int64_t)gridDim.x * CS_NT)
    keys[i] = ((uint64_t)clampi(city[i], C - 1) << ibits) | (uint64_t)clampi(item[i], hmax);
}

// tilecount[tile] = the keys of the tile that differ from their predecessor
__global__ __launch_bounds__(CS_NT) void cs_head_count_kernel(const uint64_t* k, int64_t M,
                                                              uint32_t* tilecount) {
  const int64_t j0 = (int64_t)blockIdx.x * CS_TILE;
  int n = 0;
#pragma unroll
  for (int q = 0; q < CS_TILE_Q; ++q) {
    const int64_t j = j0 + q * CS_NT + threadIdx.x;
    if (j < M) n += (j == 0 || k[j] != k[j - 1]) ? 1 : 0;
  }
  __shared__ int part[CS_NT / WAVE];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < CS_NT / WAVE; ++w) s += part[w];
    tilecount[blockIdx.x] = (uint32_t)s;
  }
}

// the exclusive sum of one value per lane over the workgroup, through LDS
// (cs_offsets_kernel: a lane sums its run of sets and writes it from there)
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t mine, int64_t* sh) {
  const int t = threadIdx.x;
  sh[t] = mine;
  __syncthreads();
  for (int o = 1; o < CS_SCAN_NT; o <<= 1) {
    const int64_t add = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  return sh[t] - mine;
}

// Every head to set_rows at its global rank (below cap), and per city the rank
// of its first head (cfirst) and the rank behind its last (clast).
__global__ __launch_bounds__(CS_NT) void cs_write_sets_kernel(const uint64_t* k, int64_t M, int C, int ibits,
                                                              const uint32_t* tilebase, int64_t* set_rows,
                                                              int64_t cap, uint32_t* cfirst,
                                                              uint32_t* clast) {
  __shared__ int part[CS_TILE_Q][CS_NT / WAVE];
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  const int64_t j0 = (int64_t)blockIdx.x * CS_TILE;
  const uint64_t imask = (1ull << ibits) - 1ull;
  uint64_t key[CS_TILE_Q], prev[CS_TILE_Q];
  bool head[CS_TILE_Q];
  int below[CS_TILE_Q];
#pragma unroll
  for (int q = 0; q < CS_TILE_Q; ++q) {
    const int64_t j = j0 + q * CS_NT + t;
    key[q] = j < M ? k[j] : 0ull;
    prev[q] = (j < M && j > 0) ? k[j - 1] : ~0ull;   // (no key is all ones: 45 bits at most)
    head[q] = j < M && key[q] != prev[q];
    const uint64_t bal = __ballot(head[q]);
    below[q] = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) part[q][w] = __popcll(bal);
  }
  __syncthreads();
  int64_t run = tilebase[blockIdx.x];
#pragma unroll
  for (int q = 0; q < CS_TILE_Q; ++q) {
    int before = 0, all = 0;
#pragma unroll
    for (int x = 0; x < CS_NT / WAVE; ++x) {
      before += x < w ? part[q][x] : 0;
      all += part[q][x];
    }
    const int64_t j = j0 + q * CS_NT + t;
    if (j < M) {
      const int64_t p = run + before + below[q];   // heads in front of j
      const uint32_t c = min((uint32_t)(key[q] >> ibits), (uint32_t)(C - 1));
      if (head[q]) {
        if (p < cap) set_rows[p] = (int64_t)(key[q] & imask);
        if (j == 0 || (uint32_t)(prev[q] >> ibits) != c) cfirst[c] = (uint32_t)p;
      }
      const bool last = j == M - 1 || (uint32_t)(k[j + 1] >> ibits) != (uint32_t)(key[q] >> ibits);
      if (last) clast[c] = (uint32_t)(p + (head[q] ? 1 : 0));
    }
    run += all;
  }
}

// set_offsets [2C + 2]: the exclusive sum of the city sets' and then the
// popular sets' lengths, the total twice (set 2C is empty); the overflow bit;
// the mirrors with system-scope stores (host memory, or null)
__global__ __launch_bounds__(CS_SCAN_NT) void cs_offsets_kernel(const uint32_t* cfirst, const uint32_t* clast,
                                                                const uint32_t* popcount, int C, int64_t cap,
                                                                int64_t* set_offsets, int32_t* status,
                                                                int64_t* host_offsets, int32_t* host_status) {
  __shared__ int64_t sh[CS_SCAN_NT];
  const int n = 2 * C;
  const int per = (n + CS_SCAN_NT - 1) / CS_SCAN_NT;
  const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
  auto len = [&](int s) -> int64_t {
    return s < C ? (int64_t)(clast[s] - cfirst[s]) : (int64_t)popcount[s - C];
  };
  int64_t sum = 0;
  for (int s = lo; s < hi; ++s) sum += len(s);
  int64_t base = block_exclusive_scan(sum, sh);
  const int64_t total = sh[CS_SCAN_NT - 1];
  auto put = [&](int s, int64_t v) {
    set_offsets[s] = v;
    if (host_offsets) __hip_atomic_store(host_offsets + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  for (int s = lo; s < hi; ++s) {
    put(s, base);
    base += len(s);
  }
  if (threadIdx.x == 0) {
    put(n, total);
    put(n + 1, total);
    int32_t st = *status;
    if (total > cap) st |= DCNR_REQ_OVERFLOW;
    *status = st;
    if (host_status) __hip_atomic_store(host_status, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(CS_TOP_MAX) void cs_popular_copy_kernel(const int32_t* popitems,
                                                                     const uint32_t* popcount,
                                                                     const int64_t* set_offsets, int C, int top,
                                                                     int64_t* set_rows, int64_t cap) {
  const int c = blockIdx.x, t = threadIdx.x;
  const int n = min((int)popcount[c], top);
  const int64_t p = set_offsets[C + c] + t;
  if (t < n && p >= 0 && p < cap) set_rows[p] = (int64_t)popitems[(int64_t)c * top + t];
}

// M = 0: offsets of zeros, top_rows of -1, a clean status
__global__ __launch_bounds__(CS_NT) void cs_empty_kernel(int C, int top, int64_t* set_offsets, int32_t* top_rows,
                                                         int32_t* status, int64_t* host_offsets,
                                                         int32_t* host_status) {
  const int64_t i0 = (int64_t)blockIdx.x * CS_NT + threadIdx.x, step = (int64_t)gridDim.x * CS_NT;
  for (int64_t i = i0; i < 2 * (int64_t)C + 2; i += step) {
    set_offsets[i] = 0;
    if (host_offsets)
      __hip_atomic_store(host_offsets + i, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  for (int64_t i = i0; i < (int64_t)C * top; i += step) top_rows[i] = -1;
  if (i0 == 0) {
    *status = 0;
    if (host_status) __hip_atomic_store(host_status, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

static size_t city_sets_ws_bytes(int64_t M, int64_t n_items, int n_cities, int top) {
  return carve(make_plan(M, n_items, n_cities), M, n_cities, top, nullptr).total;
}

static dcnr_status city_sets_build(const int32_t* item, const int32_t* city, const double* key,
                                   const int32_t* row, int64_t M, int64_t n_items, int C, int top,
                                   int64_t* set_offsets, int64_t* set_rows, int64_t cap, int32_t* top_rows,
                                   int32_t* status, int64_t* host_offsets, int32_t* host_status, void* ws,
                                   hipStream_t s) {
  if (M == 0) {
    const int blocks = (int)std::min<int64_t>(CS_MAXB, cdiv(std::max<int64_t>(2 * (int64_t)C + 2,
                                                                              (int64_t)C * top), CS_NT));
    hipLaunchKernelGGL(cs_empty_kernel, dim3(blocks), dim3(CS_NT), 0, s, C, top, set_offsets, top_rows,
                       status, host_offsets, host_status);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  const Plan p = make_plan(M, n_items, C);
  const Ws w = carve(p, M, C, top, ws);
  uint32_t *cstart = w.cwords, *cend = w.cwords + C, *cfirst = w.cwords + 2 * (size_t)C,
           *clast = w.cwords + 3 * (size_t)C;
  TRY(fill_zero(w.cwords, (size_t)C * 16, s));
  TRY(fill_zero(status, 4, s));
  // ---- top_rows and the popular sets
  hipLaunchKernelGGL(cs_records_kernel, dim3(p.blocks), dim3(CS_NT), 0, s, item, city, key, row, M, n_items,
                     C, w.ra, status);
  DCNR_LAUNCH_CHECK();
  Rec *src = w.ra, *dst = w.rb;
  TRY(sort_passes(src, dst, M, p.units, p.chunk, 0, p.pass_a, w.counts, w.tot, nullptr, s));
  hipLaunchKernelGGL(cs_bounds_kernel, dim3(p.blocks), dim3(CS_NT), 0, s, (const Rec*)src, M, cstart, cend);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cs_popular_kernel, dim3(C), dim3(CS_TOP_MAX), 0, s, (const Rec*)src,
                     (const uint32_t*)cstart, (const uint32_t*)cend, item, row, M, n_items, top, top_rows,
                     w.popitems, w.popcount);
  DCNR_LAUNCH_CHECK();
  // ---- the city sets (the records are done with: their memory holds the keys)
  uint64_t *ka = (uint64_t*)w.ra, *kb = (uint64_t*)w.rb;
  hipLaunchKernelGGL(cs_keys_kernel, dim3(p.blocks), dim3(CS_NT), 0, s, item, city, M, n_items, C, p.ibits,
                     ka);
  DCNR_LAUNCH_CHECK();
  TRY(sort_passes(ka, kb, M, p.units, p.chunk, 0, p.pass_b, w.counts, w.tot, nullptr, s));
  hipLaunchKernelGGL(cs_head_count_kernel, dim3((unsigned)p.tiles), dim3(CS_NT), 0, s, (const uint64_t*)ka,
                     M, w.tilebase);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(tscan::tile_scan_kernel<false>, dim3(1), dim3(tscan::TS_SCAN_NT), 0, s, w.tilebase, p.tiles);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cs_write_sets_kernel, dim3((unsigned)p.tiles), dim3(CS_NT), 0, s, (const uint64_t*)ka,
                     M, C, p.ibits, (const uint32_t*)w.tilebase, set_rows, cap, cfirst, clast);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cs_offsets_kernel, dim3(1), dim3(CS_SCAN_NT), 0, s, (const uint32_t*)cfirst,
                     (const uint32_t*)clast, (const uint32_t*)w.popcount, C, cap, set_offsets, status,
                     host_offsets, host_status);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(cs_popular_copy_kernel, dim3(C), dim3(CS_TOP_MAX), 0, s, (const int32_t*)w.popitems,
                     (const uint32_t*)w.popcount, (const int64_t*)set_offsets, C, top, set_rows, cap);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // namespace dcnr

using namespace dcnr;

extern "C" {

static dcnr_status city_sets_shape(int64_t M, int64_t n_items, int32_t n_cities, int32_t top) {
  if (M < 0 || n_items < 0 || n_cities < 0 || top < 0) return DCNR_BAD_ARG;
  if (top < 1 || top > CS_TOP_MAX || n_cities < 1 || n_cities > 65536 || n_items > ((int64_t)1 << 29) ||
      M >= 2147483647ll)
    return DCNR_UNSUPPORTED_SHAPE;
  return DCNR_OK;
}

size_t dcnr_city_sets_workspace_size(int64_t M, int64_t n_items, int32_t n_cities, int32_t top) {
  if (city_sets_shape(M, n_items, n_cities, top) != DCNR_OK) return 0;
  return city_sets_ws_bytes(M, n_items, n_cities, top) + 256;
}

dcnr_status dcnr_city_sets_build(const int32_t* review_item, const int32_t* review_city,
                                 const double* review_key, const int32_t* review_row, int64_t M,
                                 int64_t n_items, int32_t n_cities, int32_t top, int64_t* set_offsets,
                                 int64_t* set_rows, int64_t cap, int32_t* top_rows, int32_t* status,
                                 int64_t* host_offsets, int32_t* host_status, void* ws, size_t ws_bytes,
                                 dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const dcnr_status shape = city_sets_shape(M, n_items, n_cities, top);
  if (shape == DCNR_BAD_ARG || cap < 0 || !set_offsets || !top_rows || !status ||
      (cap > 0 && !set_rows) || (M > 0 && (!review_item || !review_city || !review_key || !ws))) {
    set_error("dcnr_city_sets_build: bad argument (M=%lld, n_items=%lld, cities=%d, top=%d, cap=%lld)",
              (long long)M, (long long)n_items, n_cities, top, (long long)cap);
    return DCNR_BAD_ARG;
  }
  if (shape != DCNR_OK) {
    set_error("dcnr_city_sets_build: unsupported shape (M=%lld, n_items=%lld, cities=%d, top=%d)",
              (long long)M, (long long)n_items, n_cities, top);
    return shape;
  }
  void* base = ws_align(ws);
  const size_t need = M > 0 ? city_sets_ws_bytes(M, n_items, n_cities, top) : 0;
  if (M > 0 && ws_bytes < need + ((char*)base - (char*)ws)) {
    set_error("dcnr_city_sets_build: workspace too small: %zu < %zu", ws_bytes, need + 256);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TRYP(DCNR_K_SERVE, s, city_sets_build(review_item, review_city, review_key, review_row, M, n_items,
                                        n_cities, top, set_offsets, set_rows, cap, top_rows, status,
                                        host_offsets, host_status, base, s));
  return DCNR_OK;
}

}  // extern "C"
