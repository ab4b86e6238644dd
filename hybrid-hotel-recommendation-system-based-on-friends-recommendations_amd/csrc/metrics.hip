// Validation metrics of the reference's epoch end (train.py:255-265, 366-387)
// on the device: BCE-with-logits (fp64), exact ROC AUC (the midrank
// Mann-Whitney statistic, ties included) and RMSE of sigmoid(z) against y.
//
//   pass 1   one streaming pass over (z, y): the fp64 sums and counters as
//            per-block partials (fixed order), one 33-bit order-preserving key
//            per element, (orderable_u32(z) << 1) | is_pos, and the digit
//            histograms of all radix passes (a digit histogram does not depend
//            on the order of the keys)
//   sort     keys-only LSD radix sort, NPASS passes of RBITS bits.  A "unit"
//            is the contiguous run of keys one wave walks 64 at a time; per
//            pass: per-unit digit counts, a scan over (digit, unit), a stable
//            scatter that ranks equal digits within a wave by match-any over
//            ballots (no atomics: the order within a digit is the input's)
//   AUC      over the sorted keys, negatives first within a tie group: a
//            positive at i contributes negs_before(i) + negs_before(head of
//            i's tie group) to 2U; the second term is the value of the
//            monotone prefix at the last head <= i, carried across blocks as
//            (negatives in the tile, prefix at the tile's last head)
//   final    fixed-order sums of the partials, the struct
//
// Every count is an integer, every fp64 sum has a fixed order that depends on
// n alone: two calls on the same input give the same bits.
#include "dcnr_internal.h"

namespace dcnr {

namespace {

// (tests/metrics_cases.py places n around UNIT_KEYS and AUC_TILE_MIN)
constexpr int KEY_BITS = 33;
constexpr int RBITS = 11;                                  // digit width
constexpr int NPASS = (KEY_BITS + RBITS - 1) / RBITS;      // 3
constexpr int NB = 1 << RBITS;                             // buckets per pass
constexpr int UNIT_KEYS = 4096;                            // keys per unit before MAX_UNITS binds
constexpr int MAX_UNITS = 1024;
constexpr int SORT_NT = 256, SORT_WAVES = SORT_NT / WAVE;  // 4 units per block
constexpr int SORT_UNROLL = 4;                             // 64-key steps loaded ahead
constexpr int SCAN_NT = 1024, SCAN_SEG = SCAN_NT / WAVE;   // 64 buckets x 16 unit segments
constexpr int P1_NT = 1024, P1_KEYS = 8192, P1_MAXB = 1024;
constexpr int AUC_NT = 256, AUC_WAVES = AUC_NT / WAVE, AUC_TILE_MIN = 2048, AUC_MAXB = 1024;
constexpr int FIN_NT = 256;

struct P1Part { double ll, se; long long npos, nbad, nnan; };

struct Plan {
  int units; int64_t chunk;          // sort units and keys per unit (a multiple of 64)
  int p1_blocks;
  int auc_blocks; int64_t auc_tile;  // (a multiple of AUC_NT)
};

Plan make_plan(int64_t n) {
  Plan p;
  p.units = (int)std::min<int64_t>(MAX_UNITS, std::max<int64_t>(1, cdiv(n, UNIT_KEYS)));
  p.chunk = rup(cdiv(n, p.units), WAVE);
  p.p1_blocks = (int)std::min<int64_t>(P1_MAXB, std::max<int64_t>(1, cdiv(n, P1_KEYS)));
  p.auc_tile = std::max<int64_t>(AUC_TILE_MIN, rup(cdiv(n, AUC_MAXB), AUC_NT));
  p.auc_blocks = (int)cdiv(n, p.auc_tile);
  return p;
}

struct Ws {
  uint64_t *ka, *kb;      // [n] key ping-pong
  uint32_t* tot;          // [NPASS][NB] digit totals of the whole input
  uint32_t* counts;       // [units][NB] per-unit digit counts -> scatter offsets
  P1Part* part;           // [p1_blocks]
  long long* summary;     // [auc_blocks][2] negatives in the tile, prefix at its last head (-1: none)
  long long* carry;       // [auc_blocks][2] negatives before the tile, prefix at the last head before it
  long long* u2part;      // [auc_blocks]
  size_t total;
};

Ws carve(const Plan& p, int64_t n, void* base) {
  Bump b(base);
  Ws w;
  w.ka = (uint64_t*)b.take((size_t)n * 8);
  w.kb = (uint64_t*)b.take((size_t)n * 8);
  w.tot = (uint32_t*)b.take((size_t)NPASS * NB * 4);
  w.counts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.part = (P1Part*)b.take((size_t)p.p1_blocks * sizeof(P1Part));
  w.summary = (long long*)b.take((size_t)p.auc_blocks * 16);
  w.carry = (long long*)b.take((size_t)p.auc_blocks * 16);
  w.u2part = (long long*)b.take((size_t)p.auc_blocks * 8);
  w.total = b.off;
  return w;
}

// (orderable_u32(z) << 1) | is_pos.  IEEE equality: -0.0 takes +0.0's key
// (integer test: no arithmetic that could flush a denormal), +-inf and the
// denormals are ordinary values.
__device__ __forceinline__ uint64_t make_key(float z, bool pos) {
  uint32_t u = __float_as_uint(z);
  if (u == 0x80000000u) u = 0u;
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((uint64_t)u << 1) | (pos ? 1u : 0u);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, o, 64);
    const int hi = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), o, 64);
    v += (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
  }
  return v;
}

__global__ __launch_bounds__(P1_NT) void metrics_pass1_kernel(const float* z, const float* y, int64_t n,
                                                              uint64_t* keys, uint32_t* tot,
                                                              P1Part* part) {
  __shared__ uint32_t h[NPASS * NB];
  __shared__ P1Part wp[P1_NT / WAVE];
  const int tid = threadIdx.x;
  for (int j = tid; j < NPASS * NB; j += P1_NT) h[j] = 0u;
  __syncthreads();
  double ll = 0.0, se = 0.0;
  long long npos = 0, nbad = 0, nnan = 0;
  for (int64_t i = (int64_t)blockIdx.x * P1_NT + tid; i < n; i += (int64_t)gridDim.x * P1_NT) {
    const float zz = z[i], yy = y[i];
    const bool pos = yy == 1.0f;
    npos += pos;
    nbad += !(pos || yy == 0.0f);
    nnan += zz != zz;
    const double zd = (double)zz, yd = (double)yy;
    ll += fmax(zd, 0.0) - zd * yd + log1p(exp(-fabs(zd)));
    const float p = (float)(1.0 / (1.0 + exp(-zd)));
    const double d = yd - (double)p;
    se += d * d;
    const uint64_t key = make_key(zz, pos);
    keys[i] = key;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
      atomicAdd(&h[ps * NB + (int)((key >> (ps * RBITS)) & (NB - 1))], 1u);
  }
  // fixed order: lanes of a wave (butterfly), then the waves in order
  ll = wave_sum_f64(ll);
  se = wave_sum_f64(se);
  npos = wave_sum_i64(npos);
  nbad = wave_sum_i64(nbad);
  nnan = wave_sum_i64(nnan);
  if ((tid & 63) == 0) wp[tid >> 6] = P1Part{ll, se, npos, nbad, nnan};
  __syncthreads();
  if (tid == 0) {
    P1Part a = wp[0];
    for (int w = 1; w < P1_NT / WAVE; ++w) {
      a.ll += wp[w].ll; a.se += wp[w].se;
      a.npos += wp[w].npos; a.nbad += wp[w].nbad; a.nnan += wp[w].nnan;
    }
    part[blockIdx.x] = a;
  }
  for (int j = tid; j < NPASS * NB; j += P1_NT) {
    const uint32_t c = h[j];
    if (c) atomicAdd(&tot[j], c);   // integer: any order, same sum
  }
}

// counts[u][d] = keys of unit u whose digit is d
__global__ __launch_bounds__(SORT_NT) void sort_hist_kernel(const uint64_t* keys, int64_t n, int units,
                                                            int64_t chunk, int shift, uint32_t* counts) {
  __shared__ uint32_t h[SORT_WAVES][NB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int u = blockIdx.x * SORT_WAVES + w;
  for (int d = lane; d < NB; d += WAVE) h[w][d] = 0u;
  __syncthreads();
  if (u < units) {
    const int64_t lo = (int64_t)u * chunk, hi = min(n, lo + chunk);
    for (int64_t i0 = lo + lane; i0 < hi; i0 += SORT_UNROLL * WAVE) {
      uint64_t k[SORT_UNROLL];
#pragma unroll
      for (int q = 0; q < SORT_UNROLL; ++q) k[q] = i0 + q * WAVE < hi ? keys[i0 + q * WAVE] : 0ull;
#pragma unroll
      for (int q = 0; q < SORT_UNROLL; ++q)
        if (i0 + q * WAVE < hi) atomicAdd(&h[w][(int)((k[q] >> shift) & (NB - 1))], 1u);
    }
  }
  __syncthreads();
  if (u < units)
    for (int d = lane; d < NB; d += WAVE) counts[(int64_t)u * NB + d] = h[w][d];
}

// counts[u][d] -> first output position of unit u's keys of digit d: the keys
// of lower digits (tot), then the lower units' keys of digit d.  One block
// per 64 digits; thread (j, s) walks digit b0 + j over unit segment s.
__global__ __launch_bounds__(SCAN_NT) void sort_scan_kernel(const uint32_t* tot, uint32_t* counts,
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
__global__ __launch_bounds__(SORT_NT) void sort_scatter_kernel(const uint64_t* in, uint64_t* out,
                                                               int64_t n, int units, int64_t chunk,
                                                               int shift, const uint32_t* counts) {
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
    uint64_t keys[SORT_UNROLL];
    bool valids[SORT_UNROLL];
#pragma unroll
    for (int q = 0; q < SORT_UNROLL; ++q) {
      const int64_t i = i0 + q * WAVE + lane;
      valids[q] = i < hi;
      keys[q] = valids[q] ? in[i] : 0ull;
    }
#pragma unroll
    for (int q = 0; q < SORT_UNROLL; ++q) {
      const bool valid = valids[q];
      const uint64_t key = keys[q];
      const uint32_t d = (uint32_t)((key >> shift) & (NB - 1));
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

// One walk over a tile of the sorted keys.  SUM = false: the tile's summary
// (negatives in it, the tile-local prefix at its last tie-group head or -1).
// SUM = true: given the carry (negatives before the tile, the prefix at the
// last head before it), the tile's part of 2U.
template <bool SUM>
__global__ __launch_bounds__(AUC_NT) void auc_walk_kernel(const uint64_t* k, int64_t n, int64_t tile,
                                                          const long long* carry, long long* outp) {
  __shared__ int wneg[AUC_WAVES], whead[AUC_WAVES];
  __shared__ long long wacc[AUC_WAVES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint64_t lt = (1ull << lane) - 1ull, le = lt | (1ull << lane);
  const int64_t lo = (int64_t)blockIdx.x * tile, hi = min(n, lo + tile);
  long long cneg = SUM ? carry[2 * blockIdx.x] : 0ll;
  long long cH = SUM ? carry[2 * blockIdx.x + 1] : -1ll;
  long long acc = 0;
  for (int64_t i0 = lo; i0 < hi; i0 += AUC_NT) {   // block-uniform trip count
    const int64_t i = i0 + tid;
    const bool valid = i < hi;
    const uint64_t key = valid ? k[i] : 0ull;
    const uint64_t prev = (valid && i > 0) ? k[i - 1] : 0ull;
    const bool neg = valid && !(key & 1ull);
    const bool pos = valid && (key & 1ull);
    const bool head = valid && (i == 0 || (key >> 1) != (prev >> 1));
    const uint64_t negbal = __ballot(neg), headbal = __ballot(head);
    if (lane == 0) {
      wneg[w] = __popcll(negbal);
      whead[w] = headbal ? __popcll(negbal & ((1ull << (63 - __clzll((long long)headbal))) - 1ull)) : -1;
    }
    __syncthreads();
    int pre = 0, tot = 0;
    long long H = cH, nH = cH;
#pragma unroll
    for (int v = 0; v < AUC_WAVES; ++v) {
      if (v == w) { pre = tot; H = nH; }
      if (whead[v] >= 0) nH = cneg + tot + whead[v];
      tot += wneg[v];
    }
    const long long wb = cneg + pre;   // negatives before this wave's 64 keys
    const uint64_t hb = headbal & le;
    if (hb) H = wb + __popcll(negbal & ((1ull << (63 - __clzll((long long)hb))) - 1ull));
    if (SUM && pos) acc += wb + __popcll(negbal & lt) + H;
    __syncthreads();
    cneg += tot;
    cH = nH;
  }
  if (SUM) {
    acc = wave_sum_i64(acc);
    if (lane == 0) wacc[w] = acc;
    __syncthreads();
    if (tid == 0) {
      long long a = 0;
      for (int v = 0; v < AUC_WAVES; ++v) a += wacc[v];
      outp[blockIdx.x] = a;
    }
  } else if (tid == 0) {
    outp[2 * blockIdx.x] = cneg;
    outp[2 * blockIdx.x + 1] = cH;
  }
}

// carry[b] = (negatives before tile b, prefix at the last head before it);
// nb <= AUC_MAXB tiles, one block
__global__ __launch_bounds__(AUC_MAXB) void auc_carry_kernel(const long long* summary, int nb,
                                                             long long* carry) {
  __shared__ long long a[AUC_MAXB], m[AUC_MAXB];
  const int t = threadIdx.x;
  const long long own = t < nb ? summary[2 * t] : 0ll;
  const long long hl = t < nb ? summary[2 * t + 1] : -1ll;
  a[t] = own;
  __syncthreads();
  for (int o = 1; o < AUC_MAXB; o <<= 1) {
    const long long v = t >= o ? a[t - o] : 0ll;
    __syncthreads();
    a[t] += v;
    __syncthreads();
  }
  const long long P = a[t] - own;
  m[t] = hl >= 0 ? P + hl : -1ll;
  __syncthreads();
  for (int o = 1; o < AUC_MAXB; o <<= 1) {
    const long long v = t >= o ? m[t - o] : -1ll;
    __syncthreads();
    m[t] = max(m[t], v);
    __syncthreads();
  }
  if (t < nb) {
    carry[2 * t] = P;
    carry[2 * t + 1] = t > 0 ? m[t - 1] : -1ll;
  }
}

__global__ __launch_bounds__(FIN_NT) void metrics_final_kernel(const P1Part* part, int np,
                                                               const long long* u2part, int nu,
                                                               int64_t n, dcnr_metrics* out) {
  __shared__ P1Part r[FIN_NT];
  __shared__ long long ru[FIN_NT];
  const int t = threadIdx.x;
  P1Part a = P1Part{0.0, 0.0, 0, 0, 0};
  for (int i = t; i < np; i += FIN_NT) {
    const P1Part b = part[i];
    a.ll += b.ll; a.se += b.se; a.npos += b.npos; a.nbad += b.nbad; a.nnan += b.nnan;
  }
  long long u2 = 0;
  for (int i = t; i < nu; i += FIN_NT) u2 += u2part[i];
  r[t] = a;
  ru[t] = u2;
  __syncthreads();
  for (int o = FIN_NT / 2; o > 0; o >>= 1) {
    if (t < o) {
      r[t].ll += r[t + o].ll; r[t].se += r[t + o].se;
      r[t].npos += r[t + o].npos; r[t].nbad += r[t + o].nbad; r[t].nnan += r[t + o].nnan;
      ru[t] += ru[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const long long npos = r[0].npos, nneg = (long long)n - npos;
    dcnr_metrics mm;
    mm.logloss = r[0].ll / (double)n;
    mm.auc = (npos == 0 || nneg == 0) ? __longlong_as_double(0x7ff8000000000000ll)
                                      : (double)ru[0] / (2.0 * (double)npos * (double)nneg);
    mm.rmse = sqrt(r[0].se / (double)n);
    mm.n = n;
    mm.n_pos = npos;
    mm.n_neg = nneg;
    mm.auc_u2 = ru[0];
    mm.n_bad_label = r[0].nbad;
    mm.n_nan = r[0].nnan;
    *out = mm;
  }
}

__global__ void metrics_empty_kernel(dcnr_metrics* out) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  dcnr_metrics mm;
  mm.logloss = qnan; mm.auc = qnan; mm.rmse = qnan;
  mm.n = 0; mm.n_pos = 0; mm.n_neg = 0; mm.auc_u2 = 0; mm.n_bad_label = 0; mm.n_nan = 0;
  *out = mm;
}

}  // namespace

size_t metrics_ws_bytes(int64_t n) {
  if (n <= 0) return 0;
  return carve(make_plan(n), n, nullptr).total;
}

dcnr_status eval_metrics(const float* z, const float* y, int64_t n, dcnr_metrics* out, void* ws,
                         hipStream_t s) {
  if (n == 0) {
    hipLaunchKernelGGL(metrics_empty_kernel, dim3(1), dim3(1), 0, s, out);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  const Plan p = make_plan(n);
  const Ws w = carve(p, n, ws);
  TRY_ST(fill_zero(w.tot, (size_t)NPASS * NB * 4, s));
  hipLaunchKernelGGL(metrics_pass1_kernel, dim3(p.p1_blocks), dim3(P1_NT), 0, s, z, y, n, w.ka, w.tot,
                     w.part);
  DCNR_LAUNCH_CHECK();
  uint64_t *src = w.ka, *dst = w.kb;
  const int sort_blocks = (int)cdiv(p.units, SORT_WAVES);
  for (int ps = 0; ps < NPASS; ++ps) {
    const int shift = ps * RBITS;
    hipLaunchKernelGGL(sort_hist_kernel, dim3(sort_blocks), dim3(SORT_NT), 0, s, src, n, p.units,
                       p.chunk, shift, w.counts);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_scan_kernel, dim3(NB / WAVE), dim3(SCAN_NT), 0, s, w.tot + ps * NB,
                       w.counts, p.units);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(sort_blocks), dim3(SORT_NT), 0, s, src, dst, n,
                       p.units, p.chunk, shift, w.counts);
    DCNR_LAUNCH_CHECK();
    std::swap(src, dst);
  }
  hipLaunchKernelGGL(auc_walk_kernel<false>, dim3(p.auc_blocks), dim3(AUC_NT), 0, s, src, n, p.auc_tile,
                     (const long long*)nullptr, w.summary);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(auc_carry_kernel, dim3(1), dim3(AUC_MAXB), 0, s, w.summary, p.auc_blocks, w.carry);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(auc_walk_kernel<true>, dim3(p.auc_blocks), dim3(AUC_NT), 0, s, src, n, p.auc_tile,
                     w.carry, w.u2part);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(FIN_NT), 0, s, w.part, p.p1_blocks, w.u2part,
                     p.auc_blocks, n, out);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // namespace dcnr
