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
#include "device_prims.h"

namespace dcnr {

namespace {

// (tests/metrics_cases.py places n around UNIT_KEYS and AUC_TILE_MIN)
// the sort's kernels and constants (RBITS, NB, UNIT_KEYS ...): device_prims.h
using namespace rsort;
constexpr int KEY_BITS = 33;
constexpr int NPASS = (KEY_BITS + RBITS - 1) / RBITS;      // 3
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

static size_t metrics_ws_bytes(int64_t n) {
  if (n <= 0) return 0;
  return carve(make_plan(n), n, nullptr).total;
}

static dcnr_status eval_metrics(const float* z, const float* y, int64_t n, dcnr_metrics* out, void* ws,
                                hipStream_t s) {
  if (n == 0) {
    hipLaunchKernelGGL(metrics_empty_kernel, dim3(1), dim3(1), 0, s, out);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  const Plan p = make_plan(n);
  const Ws w = carve(p, n, ws);
  TRY(fill_zero(w.tot, (size_t)NPASS * NB * 4, s));
  hipLaunchKernelGGL(metrics_pass1_kernel, dim3(p.p1_blocks), dim3(P1_NT), 0, s, z, y, n, w.ka, w.tot,
                     w.part);
  DCNR_LAUNCH_CHECK();
  uint64_t *src = w.ka, *dst = w.kb;
  TRY(sort_passes(src, dst, n, p.units, p.chunk, 0, NPASS, w.counts, nullptr, w.tot, s));
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

// ---------------------------------------------------------------------------
// Per-group ranking metrics (dcnr_eval_group_metrics): GAUC, NDCG@k, hit
// rate / recall@k and MRR of every group's list in the order the service
// shows it (descending logit, ties by input position).
//
//   pass 1   one 64-bit key per row, group << 33 | ~orderable(z) << 1 | is_pos
//            (an id outside [0, n_groups) takes the group 2^31 - 1, which no
//            valid row has), the three counters, the digit histograms
//   sort     the same radix sort on bits 1 and up, npass = ceil((32 +
//            bits(n_groups - 1)) / 11) passes: groups become contiguous, each
//            in served order (stable: ties keep input order, the label bit
//            rides along unsorted)
//   heads    per tile: its positives, its last group head and last tie head
//            with the positives before them; one block turns these into what
//            each tile needs of the rows before it
//   walk     per row, from prefixes at the row, at its tie head T and at its
//            group head G (PB = positives before):
//              rank r = i - G + 1
//              2U part of a positive  = negatives in [T, i)
//              2U part of a negative  = positives in [G, i) + positives in [G, T)
//            (a tied pair counts once, at whichever comes later; a pair whose
//            positive scores higher counts twice, at the negative), the first
//            positive's rank, hits and discount[r - 1] per cutoff.  A wave sums
//            these per group with a segmented scan; a group inside one wave's
//            64 rows is finished by its last lane, a group that crosses waves
//            by thread 0 from the waves' first and last partial sums, a group
//            that crosses tiles by the close kernel from the tiles' partials
//            (one wave per tile, 64 following tiles a step).  No group is
//            walked by one wave: a group of all n rows is n / 64 wave steps
//            spread over every tile like any other input.
//   final    fixed-order sums of the per-tile partial means
//
// Every fp64 sum (a group's DCG, the means) is taken in an order fixed by
// where the group boundaries fall in the sorted array: no floating-point
// atomics, the same input gives the same bits.
namespace {

constexpr int GK = 4;                                      // cutoffs
constexpr int G_MAXPASS = (64 - 1 + RBITS - 1) / RBITS;    // 6: bits 1..63
constexpr int GW_NT = AUC_NT, GW_WAVES = AUC_WAVES;
constexpr uint64_t G_SENTINEL = 0x7FFFFFFFull;

struct GKs { int k[GK]; int nk; };

// sums over some rows of one group
struct GSum {
  long long c, fpr;              // 2U part, rank of the first positive (one row has it)
  unsigned long long hA, hB;     // hits[0] | hits[1] << 32, hits[2] | hits[3] << 32 (each <= 2^20)
  double d[GK];
};
__device__ __forceinline__ GSum gsum_zero() { return GSum{0, 0, 0ull, 0ull, {0.0, 0.0, 0.0, 0.0}}; }
__device__ __forceinline__ void gsum_add(GSum& a, const GSum& b) {   // a's rows come first
  a.c += b.c; a.fpr += b.fpr; a.hA += b.hA; a.hB += b.hB;
#pragma unroll
  for (int j = 0; j < GK; ++j) a.d[j] += b.d[j];
}

// a tile's open ends: the rows before its first group head (they belong to a
// group that began in an earlier tile) and the rows from its last head on
struct GTile {
  GSum head, tail;
  long long has_head;
  long long first_g, first_pb;   // index of the first head, positives before it
  long long tail_g, tail_pb;     // index of the last head, positives before it
};

// partial sums of the summary over finished groups
struct GAcc {
  long long present, nauc, ranked, rows_auc, hitg[GK];
  double gauc, macro, mrr, recall[GK], ndcg[GK];
};
__device__ __forceinline__ GAcc gacc_zero() {
  GAcc a;
  a.present = a.nauc = a.ranked = a.rows_auc = 0;
  a.gauc = a.macro = a.mrr = 0.0;
#pragma unroll
  for (int j = 0; j < GK; ++j) { a.hitg[j] = 0; a.recall[j] = 0.0; a.ndcg[j] = 0.0; }
  return a;
}
__device__ __forceinline__ void gacc_add(GAcc& a, const GAcc& b) {
  a.present += b.present; a.nauc += b.nauc; a.ranked += b.ranked; a.rows_auc += b.rows_auc;
  a.gauc += b.gauc; a.macro += b.macro; a.mrr += b.mrr;
#pragma unroll
  for (int j = 0; j < GK; ++j) { a.hitg[j] += b.hitg[j]; a.recall[j] += b.recall[j]; a.ndcg[j] += b.ndcg[j]; }
}
__device__ __forceinline__ void gacc_wave_sum(GAcc& a) {
  a.present = wave_sum_i64(a.present); a.nauc = wave_sum_i64(a.nauc);
  a.ranked = wave_sum_i64(a.ranked); a.rows_auc = wave_sum_i64(a.rows_auc);
  a.gauc = wave_sum_f64(a.gauc); a.macro = wave_sum_f64(a.macro); a.mrr = wave_sum_f64(a.mrr);
#pragma unroll
  for (int j = 0; j < GK; ++j) {
    a.hitg[j] = wave_sum_i64(a.hitg[j]);
    a.recall[j] = wave_sum_f64(a.recall[j]);
    a.ndcg[j] = wave_sum_f64(a.ndcg[j]);
  }
}

int group_passes(int64_t n_groups) {
  int bits = 0;
  for (uint64_t v = (uint64_t)(n_groups - 1); v; v >>= 1) ++bits;
  return (32 + bits + RBITS - 1) / RBITS;
}

struct GWs {
  uint64_t *ka, *kb;             // [n] key ping-pong
  uint32_t* tot;                 // [npass][NB] digit totals, then the 3 counters (4 x 8 B)
  uint32_t* counts;              // [units][NB]
  long long* tsum;               // [tiles][5] positives, last group head, positives before it in
                                 //            the tile, last tie head, positives before it (-1: none)
  long long* tcarry;             // [tiles][5] the same at the tile's first row, absolute
  GTile* tile;                   // [tiles]
  GAcc* part;                    // [2][tiles] of the walk, of the close
  size_t total;
};

size_t gtot_bytes(int npass) { return (size_t)npass * NB * 4 + 32; }

GWs gcarve(const Plan& p, int npass, int64_t n, void* base) {
  Bump b(base);
  GWs w;
  w.ka = (uint64_t*)b.take((size_t)n * 8);
  w.kb = (uint64_t*)b.take((size_t)n * 8);
  w.tot = (uint32_t*)b.take(gtot_bytes(npass));
  w.counts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.tsum = (long long*)b.take((size_t)p.auc_blocks * 40);
  w.tcarry = (long long*)b.take((size_t)p.auc_blocks * 40);
  w.tile = (GTile*)b.take((size_t)p.auc_blocks * sizeof(GTile));
  w.part = (GAcc*)b.take((size_t)2 * p.auc_blocks * sizeof(GAcc));
  w.total = b.off;
  return w;
}

__global__ __launch_bounds__(P1_NT) void group_pass1_kernel(const float* z, const float* y,
                                                            const int64_t* g, int64_t n,
                                                            int64_t n_groups, int npass, uint64_t* keys,
                                                            uint32_t* tot) {
  __shared__ uint32_t h[G_MAXPASS * NB];
  __shared__ unsigned long long cnt[3];
  const int tid = threadIdx.x;
  for (int j = tid; j < npass * NB; j += P1_NT) h[j] = 0u;
  if (tid < 3) cnt[tid] = 0ull;
  __syncthreads();
  int nbad = 0, nnan = 0, nbadg = 0;
  for (int64_t i = (int64_t)blockIdx.x * P1_NT + tid; i < n; i += (int64_t)gridDim.x * P1_NT) {
    const float zz = z[i], yy = y[i];
    const int64_t gg = g[i];
    const bool pos = yy == 1.0f;
    const bool gok = gg >= 0 && gg < n_groups;
    nbad += !(pos || yy == 0.0f);
    nnan += zz != zz;
    nbadg += !gok;
    // descending score: the complement of the ascending 32-bit field
    const uint64_t asc = make_key(zz, false) >> 1;
    const uint64_t key = ((gok ? (uint64_t)gg : G_SENTINEL) << 33) | ((~asc & 0xFFFFFFFFull) << 1) |
                         (pos ? 1ull : 0ull);
    keys[i] = key;
    for (int ps = 0; ps < npass; ++ps)
      atomicAdd(&h[ps * NB + (int)((key >> (1 + ps * RBITS)) & (NB - 1))], 1u);
  }
  if (nbad) atomicAdd(&cnt[0], (unsigned long long)nbad);
  if (nnan) atomicAdd(&cnt[1], (unsigned long long)nnan);
  if (nbadg) atomicAdd(&cnt[2], (unsigned long long)nbadg);
  __syncthreads();
  for (int j = tid; j < npass * NB; j += P1_NT) {
    const uint32_t c = h[j];
    if (c) atomicAdd(&tot[j], c);   // integer: any order, same sum
  }
  unsigned long long* gc = (unsigned long long*)(tot + (size_t)npass * NB);
  if (tid < 3 && cnt[tid]) atomicAdd(&gc[tid], cnt[tid]);
}

// tsum[b] of one tile of the sorted keys
__global__ __launch_bounds__(GW_NT) void group_heads_kernel(const uint64_t* k, int64_t n, int64_t tile,
                                                            long long* tsum) {
  __shared__ int lastg, lastt;          // offsets in the tile, -1: none
  __shared__ int np, npg, npt;
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * tile, hi = min(n, lo + tile);
  if (tid == 0) { lastg = -1; lastt = -1; np = 0; npg = 0; npt = 0; }
  __syncthreads();
  int mg = -1, mt = -1;
  for (int64_t i = lo + tid; i < hi; i += GW_NT) {
    const uint64_t key = k[i], prev = i > 0 ? k[i - 1] : 0ull;
    if (i == 0 || (key >> 33) != (prev >> 33)) mg = (int)(i - lo);
    if (i == 0 || (key >> 1) != (prev >> 1)) mt = (int)(i - lo);
  }
  if (mg >= 0) atomicMax(&lastg, mg);
  if (mt >= 0) atomicMax(&lastt, mt);
  __syncthreads();
  const int lg = lastg, lt = lastt;
  int a = 0, ag = 0, at = 0;
  for (int64_t i = lo + tid; i < hi; i += GW_NT) {
    const int pos = (int)(k[i] & 1ull), off = (int)(i - lo);
    a += pos;
    ag += pos && off < lg;
    at += pos && off < lt;
  }
  if (a) atomicAdd(&np, a);
  if (ag) atomicAdd(&npg, ag);
  if (at) atomicAdd(&npt, at);
  __syncthreads();
  if (tid == 0) {
    long long* o = tsum + 5 * (int64_t)blockIdx.x;
    o[0] = np;
    o[1] = lg >= 0 ? lo + lg : -1ll;
    o[2] = lg >= 0 ? npg : -1ll;
    o[3] = lt >= 0 ? lo + lt : -1ll;
    o[4] = lt >= 0 ? npt : -1ll;
  }
}

// tcarry[b] = (positives before tile b; the last group head before it and
// the positives before that head; the same for the last tie head): an
// exclusive sum and four running maxima (a later head has the larger index
// and no fewer positives before it).  nb <= AUC_MAXB tiles, one block.
__global__ __launch_bounds__(AUC_MAXB) void group_carry_kernel(const long long* tsum, int nb,
                                                               long long* tcarry) {
  __shared__ long long a[AUC_MAXB], m[AUC_MAXB];
  const int t = threadIdx.x;
  const long long own = t < nb ? tsum[5 * t] : 0ll;
  a[t] = own;
  __syncthreads();
  for (int o = 1; o < AUC_MAXB; o <<= 1) {
    const long long v = t >= o ? a[t - o] : 0ll;
    __syncthreads();
    a[t] += v;
    __syncthreads();
  }
  const long long P = a[t] - own;
  if (t < nb) tcarry[5 * t] = P;
  for (int f = 1; f < 5; ++f) {
    const long long v0 = t < nb ? tsum[5 * t + f] : -1ll;
    // indices (f odd) are absolute already, counts are relative to the tile
    m[t] = v0 < 0 ? -1ll : ((f & 1) ? v0 : P + v0);
    __syncthreads();
    for (int o = 1; o < AUC_MAXB; o <<= 1) {
      const long long v = t >= o ? m[t - o] : -1ll;
      __syncthreads();
      m[t] = max(m[t], v);
      __syncthreads();
    }
    if (t < nb) tcarry[5 * t + f] = t > 0 ? m[t - 1] : -1ll;
    __syncthreads();
  }
}

// The finished group whose rows are [G, E) of the sorted keys, PBG / PBE
// positives before them: its record and its terms of the summary.
__device__ __forceinline__ void group_finish(const GSum& s, long long G, long long PBG, long long E,
                                             long long PBE, const uint64_t* k, int64_t n_groups,
                                             const GKs& ks, const double* ideal,
                                             dcnr_group_record* per_group, GAcc& acc) {
  const uint64_t gid = k[G] >> 33;
  if (gid >= (uint64_t)n_groups) return;   // rows whose id was out of range
  const long long nu = E - G, P = PBE - PBG, N = nu - P;
  const long long hits[GK] = {(long long)(s.hA & 0xFFFFFFFFull), (long long)(s.hA >> 32),
                              (long long)(s.hB & 0xFFFFFFFFull), (long long)(s.hB >> 32)};
  if (per_group) {
    dcnr_group_record r;
    r.n = nu; r.n_pos = P; r.auc_u2 = s.c; r.first_pos_rank = s.fpr;
#pragma unroll
    for (int j = 0; j < GK; ++j) { r.hits[j] = hits[j]; r.dcg[j] = s.d[j]; }
    per_group[gid] = r;
  }
  acc.present += 1;
  if (P > 0 && N > 0) {
    const double auc = (double)s.c / (2.0 * (double)P * (double)N);
    acc.nauc += 1;
    acc.rows_auc += nu;
    acc.gauc += (double)nu * auc;
    acc.macro += auc;
  }
  if (P > 0) {
    acc.ranked += 1;
    acc.mrr += 1.0 / (double)s.fpr;
#pragma unroll
    for (int j = 0; j < GK; ++j)
      if (j < ks.nk) {
        acc.hitg[j] += hits[j] > 0;
        acc.recall[j] += (double)hits[j] / (double)P;
        acc.ndcg[j] += s.d[j] / ideal[min((long long)ks.k[j], P) - 1];
      }
  }
}

// per wave and 64-row step, by lane 0 (positives counted within the wave)
struct GWaveMeta {
  int npos;
  int first_l, first_pb;   // lane of the first group head (-1: none), positives before it
  int last_l, last_pb;     // of the last group head
  int tie_l, tie_pb;       // of the last tie head
};

__device__ __forceinline__ uint64_t below(int lane) { return (1ull << lane) - 1ull; }   // lane < 64

__global__ __launch_bounds__(GW_NT) void group_walk_kernel(const uint64_t* k, int64_t n, int64_t tile,
                                                           const long long* tcarry, int64_t n_groups,
                                                           GKs ks, const double* discount,
                                                           const double* ideal,
                                                           dcnr_group_record* per_group, GTile* tiles,
                                                           GAcc* part) {
  __shared__ GWaveMeta meta[2][GW_WAVES];
  __shared__ GSum whead[2][GW_WAVES], wtail[2][GW_WAVES];
  __shared__ GAcc wacc[GW_WAVES];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const uint64_t lt = below(lane), le = lt | (1ull << lane);
  const int64_t lo = (int64_t)blockIdx.x * tile, hi = min(n, lo + tile);
  const long long* cr = tcarry + 5 * (int64_t)blockIdx.x;
  // at the step's first row: positives before it, the last group head and
  // tie head before it with the positives before them
  long long cPB = cr[0], cG = cr[1], cPBG = cr[2], cT = cr[3], cPBT = cr[4];
  const int kmax = ks.nk > 0 ? ks.k[ks.nk - 1] : 0;
  GAcc acc = gacc_zero();
  // thread 0: the group open at the step's first row
  GSum open = gsum_zero();
  long long oG = -1, oPBG = 0;
  bool before_first = true;      // no head of this tile seen yet
  GTile out;
  out.head = gsum_zero(); out.tail = gsum_zero();
  out.has_head = 0; out.first_g = -1; out.first_pb = 0; out.tail_g = -1; out.tail_pb = 0;
  int par = 0;
  for (int64_t i0 = lo; i0 < hi; i0 += GW_NT, par ^= 1) {   // block-uniform trip count
    const int64_t base = i0 + w * WAVE, i = base + lane;
    const bool valid = i < hi;
    const uint64_t key = valid ? k[i] : 0ull;
    const uint64_t prev = (valid && i > 0) ? k[i - 1] : 0ull;
    const bool pos = valid && (key & 1ull);
    const bool ghead = valid && (i == 0 || (key >> 33) != (prev >> 33));
    const bool thead = valid && (i == 0 || (key >> 1) != (prev >> 1));
    const uint64_t posbal = __ballot(pos), gbal = __ballot(ghead), tbal = __ballot(thead);
    if (lane == 0) {
      GWaveMeta mm;
      mm.npos = __popcll(posbal);
      mm.first_l = gbal ? __ffsll((unsigned long long)gbal) - 1 : -1;
      mm.first_pb = gbal ? __popcll(posbal & below(mm.first_l)) : 0;
      mm.last_l = gbal ? 63 - __clzll((long long)gbal) : -1;
      mm.last_pb = gbal ? __popcll(posbal & below(mm.last_l)) : 0;
      mm.tie_l = tbal ? 63 - __clzll((long long)tbal) : -1;
      mm.tie_pb = tbal ? __popcll(posbal & below(mm.tie_l)) : 0;
      meta[par][w] = mm;
    }
    __syncthreads();
    // what this wave's first row sees, and the carry of the next step
    long long wPB = cPB, wG = cG, wPBG = cPBG, wT = cT, wPBT = cPBT;
    long long nPB = cPB, nG = cG, nPBG = cPBG, nT = cT, nPBT = cPBT;
#pragma unroll
    for (int v = 0; v < GW_WAVES; ++v) {
      if (v == w) { wPB = nPB; wG = nG; wPBG = nPBG; wT = nT; wPBT = nPBT; }
      const GWaveMeta mm = meta[par][v];
      if (mm.last_l >= 0) { nG = i0 + v * WAVE + mm.last_l; nPBG = nPB + mm.last_pb; }
      if (mm.tie_l >= 0) { nT = i0 + v * WAVE + mm.tie_l; nPBT = nPB + mm.tie_pb; }
      nPB += mm.npos;
    }
    // this row's prefixes
    const long long PB = wPB + __popcll(posbal & lt);
    long long G = wG, PBG = wPBG, T = wT, PBT = wPBT;
    const uint64_t gb = gbal & le, tb = tbal & le;
    int seg0 = 0;                                  // first lane of this row's segment of the wave
    if (gb) {
      seg0 = 63 - __clzll((long long)gb);
      G = base + seg0;
      PBG = wPB + __popcll(posbal & below(seg0));
    }
    if (tb) {
      const int tl = 63 - __clzll((long long)tb);
      T = base + tl;
      PBT = wPB + __popcll(posbal & below(tl));
    }
    GSum s = gsum_zero();
    if (valid) {
      const long long r = (long long)i - G + 1;
      if (pos) {
        s.c = ((long long)i - T) - (PB - PBT);
        s.fpr = PB == PBG ? r : 0;
        if (r <= kmax) {
          const double dv = discount[r - 1];
#pragma unroll
          for (int j = 0; j < GK; ++j)
            if (j < ks.nk && r <= ks.k[j]) {
              s.d[j] = dv;
              if (j < 2) s.hA += 1ull << (32 * j);
              else s.hB += 1ull << (32 * (j - 2));
            }
        }
      } else {
        s.c = (PB - PBG) + (PBT - PBG);
      }
    }
    // inclusive sums over [seg0, lane]
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      GSum u;
      u.c = __shfl_up(s.c, o, WAVE); u.fpr = __shfl_up(s.fpr, o, WAVE);
      u.hA = __shfl_up(s.hA, o, WAVE); u.hB = __shfl_up(s.hB, o, WAVE);
#pragma unroll
      for (int j = 0; j < GK; ++j) u.d[j] = __shfl_up(s.d[j], o, WAVE);
      if (lane - o >= seg0) { gsum_add(u, s); s = u; }   // the lower rows first
    }
    const bool seg_last = lane == 63 || ((gbal >> (lane + 1)) & 1ull);
    if (valid && gb && lane < 63 && seg_last)     // a group that begins and ends in these 64 rows
      group_finish(s, G, PBG, (long long)i + 1, PB + (pos ? 1 : 0), k, n_groups, ks, ideal, per_group,
                   acc);
    const int fl = gbal ? __ffsll((unsigned long long)gbal) - 1 : WAVE;
    if (fl == 0) { if (lane == 0) whead[par][w] = gsum_zero(); }
    else if (lane == fl - 1) whead[par][w] = s;
    if (gbal && lane == 63) wtail[par][w] = s;
    __syncthreads();
    if (tid == 0) {
      long long pre = cPB;
#pragma unroll
      for (int v = 0; v < GW_WAVES; ++v) {
        const GWaveMeta mm = meta[par][v];
        gsum_add(open, whead[par][v]);
        if (mm.first_l >= 0) {
          const long long E = i0 + v * WAVE + mm.first_l, PBE = pre + mm.first_pb;
          if (before_first) {
            out.head = open; out.has_head = 1; out.first_g = E; out.first_pb = PBE;
            before_first = false;
          } else {
            group_finish(open, oG, oPBG, E, PBE, k, n_groups, ks, ideal, per_group, acc);
          }
          open = wtail[par][v];
          oG = i0 + v * WAVE + mm.last_l;
          oPBG = pre + mm.last_pb;
        }
        pre += mm.npos;
      }
    }
    cPB = nPB; cG = nG; cPBG = nPBG; cT = nT; cPBT = nPBT;
  }
  if (tid == 0) {
    if (before_first) out.head = open;
    else { out.tail = open; out.tail_g = oG; out.tail_pb = oPBG; }
    tiles[blockIdx.x] = out;
  }
  gacc_wave_sum(acc);
  if (lane == 0) wacc[w] = acc;
  __syncthreads();
  if (tid == 0) {
    GAcc a = wacc[0];
    for (int v = 1; v < GW_WAVES; ++v) gacc_add(a, wacc[v]);
    part[blockIdx.x] = a;
  }
}

// The last group of tile b (one wave per tile): its rows in tile b, then the
// head rows of the tiles after it up to the first one that has a head of its
// own, 64 tiles a step.
__global__ __launch_bounds__(WAVE) void group_close_kernel(const uint64_t* k, int64_t n, int nb,
                                                           const long long* tsum,
                                                           const long long* tcarry, const GTile* tiles,
                                                           int64_t n_groups, GKs ks, const double* ideal,
                                                           dcnr_group_record* per_group, GAcc* part2) {
  const int b = blockIdx.x, lane = threadIdx.x;
  GAcc acc = gacc_zero();
  if (tiles[b].has_head) {                        // wave-uniform
    GSum R = tiles[b].tail;
    long long E = n, PBE = tcarry[5 * (nb - 1)] + tsum[5 * (nb - 1)];
    for (int u0 = b + 1; u0 < nb; u0 += WAVE) {
      const int u = u0 + lane;
      const bool in = u < nb;
      const bool hh = in && tiles[u].has_head;
      const uint64_t bal = __ballot(hh);
      const int stop = bal ? __ffsll((unsigned long long)bal) - 1 : WAVE;   // the last lane to take
      GSum s = (in && lane <= stop) ? tiles[u].head : gsum_zero();
      // inclusive sums in tile order; lane 63 holds the step's total
#pragma unroll
      for (int o = 1; o < WAVE; o <<= 1) {
        GSum v;
        v.c = __shfl_up(s.c, o, WAVE); v.fpr = __shfl_up(s.fpr, o, WAVE);
        v.hA = __shfl_up(s.hA, o, WAVE); v.hB = __shfl_up(s.hB, o, WAVE);
#pragma unroll
        for (int j = 0; j < GK; ++j) v.d[j] = __shfl_up(s.d[j], o, WAVE);
        if (lane >= o) { gsum_add(v, s); s = v; }
      }
      GSum tot;
      tot.c = __shfl(s.c, 63, WAVE); tot.fpr = __shfl(s.fpr, 63, WAVE);
      tot.hA = __shfl(s.hA, 63, WAVE); tot.hB = __shfl(s.hB, 63, WAVE);
#pragma unroll
      for (int j = 0; j < GK; ++j) tot.d[j] = __shfl(s.d[j], 63, WAVE);
      gsum_add(R, tot);
      if (bal) {
        E = tiles[u0 + stop].first_g;
        PBE = tiles[u0 + stop].first_pb;
        break;
      }
    }
    if (lane == 0)
      group_finish(R, tiles[b].tail_g, tiles[b].tail_pb, E, PBE, k, n_groups, ks, ideal, per_group, acc);
  }
  if (lane == 0) part2[b] = acc;
}

__global__ __launch_bounds__(FIN_NT) void group_final_kernel(const GAcc* part, int np, int64_t n,
                                                             const uint32_t* tot, int npass, GKs ks,
                                                             dcnr_group_summary* out) {
  __shared__ GAcc wacc[FIN_NT / WAVE];
  const int t = threadIdx.x;
  GAcc a = gacc_zero();
  for (int i = t; i < np; i += FIN_NT) gacc_add(a, part[i]);
  gacc_wave_sum(a);
  if ((t & 63) == 0) wacc[t >> 6] = a;
  __syncthreads();
  if (t == 0) {
    a = wacc[0];
    for (int v = 1; v < FIN_NT / WAVE; ++v) gacc_add(a, wacc[v]);
    const unsigned long long* gc = (const unsigned long long*)(tot + (size_t)npass * NB);
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    dcnr_group_summary m;
    m.n = n;
    m.n_groups_present = a.present;
    m.n_groups_auc = a.nauc;
    m.n_groups_ranked = a.ranked;
    m.n_rows_auc = a.rows_auc;
    m.n_bad_label = (int64_t)gc[0];
    m.n_nan = (int64_t)gc[1];
    m.n_bad_group = (int64_t)gc[2];
    m.gauc = a.nauc ? a.gauc / (double)a.rows_auc : qnan;
    m.auc_macro = a.nauc ? a.macro / (double)a.nauc : qnan;
    m.mrr = a.ranked ? a.mrr / (double)a.ranked : qnan;
    for (int j = 0; j < GK; ++j) {
      const bool on = j < ks.nk && a.ranked;
      m.hit_groups[j] = j < ks.nk ? a.hitg[j] : 0;
      m.hit_rate[j] = on ? (double)a.hitg[j] / (double)a.ranked : qnan;
      m.recall[j] = on ? a.recall[j] / (double)a.ranked : qnan;
      m.ndcg[j] = on ? a.ndcg[j] / (double)a.ranked : qnan;
    }
    *out = m;
  }
}

__global__ void group_empty_kernel(dcnr_group_summary* out) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  dcnr_group_summary m;
  m.n = m.n_groups_present = m.n_groups_auc = m.n_groups_ranked = m.n_rows_auc = 0;
  m.n_bad_label = m.n_nan = m.n_bad_group = 0;
  m.gauc = m.auc_macro = m.mrr = qnan;
  for (int j = 0; j < GK; ++j) {
    m.hit_groups[j] = 0;
    m.hit_rate[j] = m.recall[j] = m.ndcg[j] = qnan;
  }
  *out = m;
}

}  // namespace

static size_t group_metrics_ws_bytes(int64_t n, int64_t n_groups) {
  if (n <= 0 || n_groups < 1) return 0;
  return gcarve(make_plan(n), group_passes(n_groups), n, nullptr).total;
}

static dcnr_status eval_group_metrics(const float* z, const float* y, const int64_t* g, int64_t n,
                                      int64_t n_groups, const int32_t* ks_host, int32_t n_k,
                                      const double* discount, const double* ideal, dcnr_group_summary* out,
                                      dcnr_group_record* per_group, void* ws, hipStream_t s) {
  if (per_group) TRY(fill_zero(per_group, (size_t)n_groups * sizeof(dcnr_group_record), s));
  if (n == 0) {
    hipLaunchKernelGGL(group_empty_kernel, dim3(1), dim3(1), 0, s, out);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  GKs ks;
  ks.nk = n_k;
  for (int j = 0; j < GK; ++j) ks.k[j] = j < n_k ? ks_host[j] : 0;
  const Plan p = make_plan(n);
  const int npass = group_passes(n_groups);
  const GWs w = gcarve(p, npass, n, ws);
  const int nb = p.auc_blocks;
  TRY(fill_zero(w.tot, gtot_bytes(npass), s));
  hipLaunchKernelGGL(group_pass1_kernel, dim3(p.p1_blocks), dim3(P1_NT), 0, s, z, y, g, n, n_groups,
                     npass, w.ka, w.tot);
  DCNR_LAUNCH_CHECK();
  uint64_t *src = w.ka, *dst = w.kb;
  TRY(sort_passes(src, dst, n, p.units, p.chunk, 1, npass, w.counts, nullptr, w.tot, s));
  hipLaunchKernelGGL(group_heads_kernel, dim3(nb), dim3(GW_NT), 0, s, src, n, p.auc_tile, w.tsum);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_carry_kernel, dim3(1), dim3(AUC_MAXB), 0, s, w.tsum, nb, w.tcarry);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_walk_kernel, dim3(nb), dim3(GW_NT), 0, s, src, n, p.auc_tile, w.tcarry,
                     n_groups, ks, discount, ideal, per_group, w.tile, w.part);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_close_kernel, dim3(nb), dim3(WAVE), 0, s, src, n, nb, w.tsum, w.tcarry,
                     w.tile, n_groups, ks, ideal, per_group, w.part + nb);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(group_final_kernel, dim3(1), dim3(FIN_NT), 0, s, w.part, 2 * nb, n, w.tot, npass,
                     ks, out);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

// ---------------------------------------------------------------------------
// List metrics (dcnr_eval_list_metrics): what the served lists look like.
// List r is rows[offsets[r] .. offsets[r] + counts[r]), measured on its first
// m = min(count, at) positions.
//
//   lists    a team of TEAM threads per list (a wave for at <= 32, four lists
//            a workgroup; the whole workgroup above): thread t < m owns
//            position t (its row, score, weight, membership in the held-out
//            set by binary search, one int32 atomic on the exposure count
//            c[row]); the m rows, each times its inverse norm, are staged in
//            LDS (16-byte loads and row stride d + 4 where d % 4 == 0 and
//            the table is 16-byte aligned, else stride d | 1); pair q of the m (m - 1) / 2 goes to
//            thread q mod TEAM as (i, (i + s) mod m), s = 1 .. m / 2, an fp32
//            dot of d fmas, summed per thread in fp64, then lanes (butterfly),
//            then waves in order.  A workgroup walks lists blockIdx, blockIdx
//            + gridDim, ... and keeps its sums of the summary in that order.
//   counts   h[v] = items with c == v for v <= R (int32 atomics; the zeros
//            counted per wave first); an item may exceed R only when a list
//            repeats a row, and fewer than `at` items can: those counts go to
//            a list of at most 128, sorted by the final kernel
//   final    one workgroup: the workgroups' partial sums in a fixed order, the
//            ascending scan of h up to the largest count seen,
//            gini_num = sum_v v h_v (2 before_v + h_v - n_items), the struct
//
// Every integer comes from integer atomics or fixed-order sums, every fp64 sum
// has an order fixed by (R, at): the same input gives the same bits.
namespace {

constexpr int LM_NT = 256;
constexpr int LM_MAXB = 2048;          // workgroups of the list kernel (partials of the summary)
constexpr int LM_OVER = 128;           // counts above R kept aside (fewer than `at` exist)
constexpr int LC_BINS = 1024, LC_MAXB = 512;   // the counts kernel: LDS bins, workgroups
constexpr int LF_NT = 256;             // the final kernel's workgroup

struct LAcc {
  long long scored, pairs, marked, bad, entries, rel_lists, hitl[GK];
  double ild, score, info, mrr, recall[GK], ndcg[GK];
};
__device__ __forceinline__ LAcc lacc_zero() {
  LAcc a;
  a.scored = a.pairs = a.marked = a.bad = a.entries = a.rel_lists = 0;
  a.ild = a.score = a.info = a.mrr = 0.0;
#pragma unroll
  for (int j = 0; j < GK; ++j) { a.hitl[j] = 0; a.recall[j] = 0.0; a.ndcg[j] = 0.0; }
  return a;
}
__device__ __forceinline__ void lacc_add(LAcc& a, const LAcc& b) {
  a.scored += b.scored; a.pairs += b.pairs; a.marked += b.marked; a.bad += b.bad;
  a.entries += b.entries; a.rel_lists += b.rel_lists;
  a.ild += b.ild; a.score += b.score; a.info += b.info; a.mrr += b.mrr;
#pragma unroll
  for (int j = 0; j < GK; ++j) { a.hitl[j] += b.hitl[j]; a.recall[j] += b.recall[j]; a.ndcg[j] += b.ndcg[j]; }
}
__device__ __forceinline__ void lacc_wave_sum(LAcc& a) {
  a.scored = wave_sum_i64(a.scored); a.pairs = wave_sum_i64(a.pairs);
  a.marked = wave_sum_i64(a.marked); a.bad = wave_sum_i64(a.bad);
  a.entries = wave_sum_i64(a.entries); a.rel_lists = wave_sum_i64(a.rel_lists);
  a.ild = wave_sum_f64(a.ild); a.score = wave_sum_f64(a.score);
  a.info = wave_sum_f64(a.info); a.mrr = wave_sum_f64(a.mrr);
#pragma unroll
  for (int j = 0; j < GK; ++j) {
    a.hitl[j] = wave_sum_i64(a.hitl[j]);
    a.recall[j] = wave_sum_f64(a.recall[j]);
    a.ndcg[j] = wave_sum_f64(a.ndcg[j]);
  }
}

// one list's sums over its positions and pairs
struct LRed {
  double pc, sc, inf, dcg[GK];
  int hits[GK], fhr;                   // fhr: the first hit's rank, INT_MAX for none
};
__device__ __forceinline__ void lred_add(LRed& a, const LRed& b) {
  a.pc += b.pc; a.sc += b.sc; a.inf += b.inf;
#pragma unroll
  for (int j = 0; j < GK; ++j) { a.dcg[j] += b.dcg[j]; a.hits[j] += b.hits[j]; }
  a.fhr = min(a.fhr, b.fhr);
}
__device__ __forceinline__ void lred_wave_sum(LRed& a) {
  a.pc = wave_sum_f64(a.pc); a.sc = wave_sum_f64(a.sc); a.inf = wave_sum_f64(a.inf);
#pragma unroll
  for (int j = 0; j < GK; ++j) a.dcg[j] = wave_sum_f64(a.dcg[j]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
#pragma unroll
    for (int j = 0; j < GK; ++j) a.hits[j] += __shfl_xor(a.hits[j], o, 64);
    a.fhr = min(a.fhr, __shfl_xor(a.fhr, o, 64));
  }
}

struct LWs {
  uint32_t* c;        // [n_items] exposure counts
  uint32_t* h;        // [R + 1] items per count
  uint32_t* misc;     // [2 + LM_OVER] the largest count <= R seen, entries of over, over
  LAcc* part;         // [LM_MAXB]
  size_t clear, total;   // the first `clear` bytes are zeroed by the call
};

LWs lcarve(int64_t R, int64_t n_items, void* base) {
  Bump b(base);
  LWs w;
  w.c = (uint32_t*)b.take((size_t)n_items * 4);
  w.h = (uint32_t*)b.take((size_t)(R + 1) * 4);
  w.misc = (uint32_t*)b.take((size_t)(2 + LM_OVER) * 4);
  w.clear = b.off;
  w.part = (LAcc*)b.take((size_t)LM_MAXB * sizeof(LAcc));
  w.total = b.off;
  return w;
}

struct LArgs {
  const int64_t* rows; int64_t n;
  const int64_t* offsets; const int32_t* counts; int64_t R; int at;
  const float* table; const float* inv; int d; int64_t n_items;
  const float* scores; const double* info;
  const int64_t* rel_rows; int64_t n_rel_rows; const int64_t* rel_offsets;
  GKs ks; const double* discount; const double* ideal;
  dcnr_list_record* per_list;
};

// Floats between two staged rows: with 16-byte accesses (VEC = 4, d % 4 == 0)
// d + 4, so that rows stay 16-byte aligned and consecutive rows start 4 banks
// apart; otherwise d | 1, odd, so that lanes reading different rows at one
// column hit different banks.
__host__ __device__ inline int list_row_stride(int d, int vec) { return vec == 4 ? d + 4 : (d | 1); }

// TEAM threads per list, LM_NT / TEAM lists per workgroup step.  Every
// __syncthreads below is reached by every thread: the loop bounds and the
// branches around them do not depend on the list.
template <int TEAM, int VEC>
__global__ __launch_bounds__(LM_NT) void list_metrics_kernel(LArgs a, uint32_t* c, LAcc* part) {
  constexpr int SU = 8;                             // loads in flight per thread while staging
  constexpr int LPB = LM_NT / TEAM;                 // lists per step
  constexpr int KT = TEAM == WAVE ? 32 : 128;       // positions a team holds
  constexpr int TW = TEAM / WAVE;                   // waves per team
  extern __shared__ __attribute__((aligned(16))) float lm_emb[];   // [LPB][at][dp]
  __shared__ int s_row[LPB * KT];
  __shared__ float s_inv[LPB * KT];
  __shared__ int s_flag[LPB];                       // 1: a row outside the table, 2: the list is marked
  __shared__ LRed s_red[LM_NT / WAVE];
  __shared__ LAcc s_acc[LPB];
  const int tid = threadIdx.x, team = tid / TEAM, t = tid % TEAM, lane = tid & 63;
  const int dp = list_row_stride(a.d, VEC);
  float* emb = lm_emb + (size_t)team * a.at * dp;
  int* row = s_row + team * KT;
  float* rinv = s_inv + team * KT;
  LAcc acc = lacc_zero();                           // kept by the team's thread 0
  for (int64_t base = (int64_t)blockIdx.x * LPB; base < a.R; base += (int64_t)gridDim.x * LPB) {
    const int64_t r = base + team;
    const bool live = r < a.R;
    // ---- the segment, checked against lengths passed by value
    int m = 0;
    int64_t o = 0, ro = 0, nrel = 0;
    bool bad = false, seg_rows = false;             // seg_rows: the segment holds a row
    if (live) {
      o = a.offsets[r];
      const int64_t o1 = a.offsets[r + 1];
      bad = o < 0 || o1 < o || o1 > a.n;
      seg_rows = !bad && o1 > o;
      int64_t cnt = bad ? 0 : o1 - o;
      if (!bad && a.counts) {
        cnt = (int64_t)a.counts[r];
        bad = cnt < 0 || cnt > o1 - o;
      }
      if (!bad && a.rel_offsets) {
        ro = a.rel_offsets[r];
        const int64_t ro1 = a.rel_offsets[r + 1];
        bad = ro < 0 || ro1 < ro || ro1 > a.n_rel_rows;
        nrel = bad ? 0 : ro1 - ro;
      }
      m = bad ? 0 : (int)min(cnt, (int64_t)a.at);
    }
    if (t == 0) s_flag[team] = 0;
    __syncthreads();
    // (a marked answer has out_count 0: the mark is read from the segment's
    // first row whatever the count says)
    int64_t myrow = -1;
    if (t < m || (t == 0 && seg_rows)) {
      myrow = a.rows[o + t];
      if (t == 0 && myrow == -1) atomicOr(&s_flag[team], 2);
      else if (t < m && (myrow < 0 || myrow >= a.n_items)) atomicOr(&s_flag[team], 1);
      else if (t < m) rinv[t] = a.inv[myrow];
      if (t < m) row[t] = (int)myrow;
    }
    __syncthreads();
    const int flag = s_flag[team];
    const bool marked = (flag & 2) != 0;
    bad = bad || (!marked && (flag & 1));
    if (bad || marked) m = 0;
    // ---- position t: score, weight, exposure, membership
    LRed red;
    red.pc = red.sc = red.inf = 0.0;
#pragma unroll
    for (int j = 0; j < GK; ++j) { red.dcg[j] = 0.0; red.hits[j] = 0; }
    red.fhr = 0x7fffffff;
    if (t < m) {
      atomicAdd(&c[myrow], 1u);
      if (a.scores) red.sc = (double)a.scores[o + t];
      if (a.info) red.inf = a.info[myrow];
      if (nrel > 0) {
        int64_t lo = ro, hi = ro + nrel;            // first entry >= myrow
        while (lo < hi) {
          const int64_t mid = lo + ((hi - lo) >> 1);
          if (a.rel_rows[mid] < myrow) lo = mid + 1; else hi = mid;
        }
        if (lo < ro + nrel && a.rel_rows[lo] == myrow) {
          red.fhr = t + 1;
#pragma unroll
          for (int j = 0; j < GK; ++j)
            if (j < a.ks.nk && t < a.ks.k[j]) { red.hits[j] = 1; red.dcg[j] = a.discount[t]; }
        }
      }
    }
    // ---- the m rows, normalised, into LDS
    // (units of VEC floats, unit e = (row e / dv, column VEC (e % dv)); SU
    // loads are issued before the first is used: the rows are random 4 d
    // byte reads and their latency is the cost of this kernel)
    {
      typedef float VT __attribute__((ext_vector_type(VEC)));
      const int dv = a.d / VEC, total = m * dv;
      for (int e0 = t; e0 < total; e0 += TEAM * SU) {
        VT v[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int e = min(e0 + u * TEAM, total - 1);      // (a clamped unit is loaded, not stored)
          const int i = e / dv, cv = e - i * dv;
          v[u] = *(const VT*)(a.table + (size_t)row[i] * a.d + cv * VEC);
        }
#pragma unroll
        for (int u = 0; u < SU; ++u) {
          const int e = e0 + u * TEAM;
          if (e < total) {
            const int i = e / dv, cv = e - i * dv;
            const float w = rinv[i];
            *(VT*)(emb + i * dp + cv * VEC) = v[u] * w;
          }
        }
      }
    }
    __syncthreads();
    // ---- pair q = (i, (i + s) mod m), i = q mod m, s = q / m + 1.  Odd m: (m - 1) / 2
    // rounds of m pairs.  Even m: m / 2 - 1 rounds of m and a last one, s = m / 2, of the
    // m / 2 pairs i < m / 2: m (m / 2 - 1) + m / 2 = m (m - 1) / 2.  So q < m (m - 1) / 2
    // names every unordered pair exactly once.
    if (m >= 2) {
      const int npairs = m * (m - 1) / 2;
      for (int q = t; q < npairs; q += TEAM) {
        const int s1 = q / m, i = q - s1 * m;
        int j = i + s1 + 1;
        if (j >= m) j -= m;
        const float* x = emb + i * dp;
        const float* y = emb + j * dp;
        float dot = 0.0f;                           // (the same order of fmas for either VEC)
        if (VEC == 4) {
#pragma unroll 4
          for (int e = 0; e < a.d; e += 4) {
            const f32x4 xv = *(const f32x4*)(x + e), yv = *(const f32x4*)(y + e);
            dot = fmaf(xv.x, yv.x, dot); dot = fmaf(xv.y, yv.y, dot);
            dot = fmaf(xv.z, yv.z, dot); dot = fmaf(xv.w, yv.w, dot);
          }
        } else {
#pragma unroll 8
          for (int e = 0; e < a.d; ++e) dot = fmaf(x[e], y[e], dot);
        }
        red.pc += (double)dot;
      }
    }
    // ---- the team's sums: lanes, then waves in order
    lred_wave_sum(red);
    if (TW > 1) {
      if (lane == 0) s_red[tid >> 6] = red;
      __syncthreads();
      if (t == 0)
        for (int v = 1; v < TW; ++v) lred_add(red, s_red[team * TW + v]);
    }
    if (t == 0 && live) {
      dcnr_list_record rec;
      rec.m = m; rec.n_rel = (bad || marked) ? 0 : nrel;
      rec.first_hit_rank = red.fhr == 0x7fffffff ? 0 : red.fhr;
#pragma unroll
      for (int j = 0; j < GK; ++j) { rec.hits[j] = red.hits[j]; rec.dcg[j] = red.dcg[j]; }
      rec.pair_cos_sum = red.pc; rec.score_sum = red.sc; rec.info_sum = red.inf;
      if (a.per_list) a.per_list[r] = rec;
      if (bad) acc.bad += 1;
      else if (marked) acc.marked += 1;
      else {
        acc.scored += m >= 1;
        acc.entries += m;
        acc.score += red.sc;
        acc.info += red.inf;
        if (m >= 2) {
          acc.pairs += 1;
          acc.ild += 1.0 - red.pc / (double)(m * (m - 1) / 2);
        }
        if (nrel > 0) {
          acc.rel_lists += 1;
          if (rec.first_hit_rank) acc.mrr += 1.0 / (double)rec.first_hit_rank;
#pragma unroll
          for (int j = 0; j < GK; ++j)
            if (j < a.ks.nk) {
              acc.hitl[j] += red.hits[j] > 0;
              acc.recall[j] += (double)red.hits[j] / (double)nrel;
              acc.ndcg[j] += red.dcg[j] / a.ideal[min((int64_t)a.ks.k[j], nrel) - 1];
            }
        }
      }
    }
    __syncthreads();                                // LDS is rewritten by the next step
  }
  if (t == 0) s_acc[team] = acc;
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < LPB; ++v) lacc_add(acc, s_acc[v]);
    part[blockIdx.x] = acc;
  }
}

__global__ __launch_bounds__(LM_NT) void list_counts_kernel(const uint32_t* c, int64_t n_items, int64_t R,
                                                           uint32_t* h, uint32_t* misc) {
  // Most items share a handful of counts (all of them 1 at small R): the
  // counts below LC_BINS are tallied in LDS and reach h once per workgroup,
  // or every item would queue on the same few words of h.
  __shared__ uint32_t bins[LC_BINS];
  for (int j = threadIdx.x; j < LC_BINS; j += LM_NT) bins[j] = 0u;
  __syncthreads();
  long long zeros = 0;
  uint32_t vmax = 0;
  for (int64_t i = (int64_t)blockIdx.x * LM_NT + threadIdx.x; i < n_items;
       i += (int64_t)gridDim.x * LM_NT) {
    const uint32_t v = c[i];
    if (v == 0) ++zeros;
    else if ((int64_t)v <= R) {
      if (v < (uint32_t)LC_BINS) atomicAdd(&bins[v], 1u); else atomicAdd(&h[v], 1u);
      vmax = max(vmax, v);
    } else {
      const uint32_t at = atomicAdd(&misc[1], 1u);
      if (at < (uint32_t)LM_OVER) misc[2 + at] = v;
    }
  }
  zeros = wave_sum_i64(zeros);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
  if ((threadIdx.x & 63) == 0) {
    if (zeros) atomicAdd(&h[0], (uint32_t)zeros);
    if (vmax) atomicMax(&misc[0], vmax);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < LC_BINS; j += LM_NT)       // (j <= R: only such counts were tallied)
    if (bins[j]) atomicAdd(&h[j], bins[j]);
}

__global__ __launch_bounds__(LF_NT) void list_final_kernel(const LAcc* part, int np, int64_t R,
                                                          int64_t n_items, const uint32_t* h,
                                                          const uint32_t* misc, GKs ks, int has_scores,
                                                          int has_info, dcnr_list_summary* out) {
  __shared__ LAcc wacc[LF_NT / WAVE];
  __shared__ long long s_cnt[LF_NT];
  __shared__ long long s_term[LF_NT / WAVE];
  const int t = threadIdx.x;
  LAcc a = lacc_zero();
  for (int i = t; i < np; i += LF_NT) lacc_add(a, part[i]);
  lacc_wave_sum(a);
  if ((t & 63) == 0) wacc[t >> 6] = a;
  // ---- counts ascending: thread t owns v in [t * chunk, (t + 1) * chunk) of [0, vmax]
  const int64_t nv = (int64_t)misc[0] + 1;
  const int64_t chunk = (nv + LF_NT - 1) / LF_NT;
  const int64_t v0 = min(nv, (int64_t)t * chunk), v1 = min(nv, v0 + chunk);
  long long mine = 0;
  for (int64_t v = v0; v < v1; ++v) mine += h[v];
  s_cnt[t] = mine;
  __syncthreads();
  for (int o = 1; o < LF_NT; o <<= 1) {               // inclusive scan of the threads' item counts
    const long long add = t >= o ? s_cnt[t - o] : 0;
    __syncthreads();
    s_cnt[t] += add;
    __syncthreads();
  }
  long long before = s_cnt[t] - mine, term = 0;
  for (int64_t v = v0; v < v1; ++v) {
    const long long hv = h[v];
    term += (long long)v * hv * (2 * before + hv - (long long)n_items);
    before += hv;
  }
  term = wave_sum_i64(term);
  if ((t & 63) == 0) s_term[t >> 6] = term;
  __syncthreads();
  if (t == 0) {
    a = wacc[0];
    for (int v = 1; v < LF_NT / WAVE; ++v) lacc_add(a, wacc[v]);
    long long gnum = 0;
    for (int v = 0; v < LF_NT / WAVE; ++v) gnum += s_term[v];
    // the few counts above R, ascending, one item each
    long long before_o = s_cnt[LF_NT - 1];
    const int no = (int)min(misc[1], (uint32_t)LM_OVER);
    uint32_t prev = 0;
    for (int k = 0; k < no; ++k) {                    // selection in ascending order (no <= 128)
      uint32_t best = 0xffffffffu;
      int nbest = 0;
      for (int e = 0; e < no; ++e) {
        const uint32_t v = misc[2 + e];
        if (v > prev && v < best) { best = v; nbest = 1; }
        else if (v == best) ++nbest;
      }
      if (!nbest) break;
      gnum += (long long)best * nbest * (2 * before_o + nbest - (long long)n_items);
      before_o += nbest;
      prev = best;
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    dcnr_list_summary m;
    m.n_lists = R;
    m.n_lists_scored = a.scored;
    m.n_lists_pairs = a.pairs;
    m.n_marked = a.marked;
    m.n_bad_list = a.bad;
    m.n_entries = a.entries;
    m.n_distinct_items = n_items - (long long)h[0];
    m.gini_num = gnum;
    m.n_rel_lists = a.rel_lists;
    m.ild = a.pairs ? a.ild / (double)a.pairs : qnan;
    m.mean_score = has_scores && a.entries ? a.score / (double)a.entries : qnan;
    m.mean_info = has_info && a.entries ? a.info / (double)a.entries : qnan;
    m.mrr = a.rel_lists ? a.mrr / (double)a.rel_lists : qnan;
    m.coverage = (double)m.n_distinct_items / (double)n_items;
    m.gini = a.entries ? (double)gnum / ((double)n_items * (double)a.entries) : qnan;
#pragma unroll
    for (int j = 0; j < GK; ++j) {
      const bool on = j < ks.nk && a.rel_lists;
      m.hit_lists[j] = j < ks.nk ? a.hitl[j] : 0;
      m.hit_rate[j] = on ? (double)a.hitl[j] / (double)a.rel_lists : qnan;
      m.recall[j] = on ? a.recall[j] / (double)a.rel_lists : qnan;
      m.ndcg[j] = on ? a.ndcg[j] / (double)a.rel_lists : qnan;
    }
    *out = m;
  }
}

__global__ void list_empty_kernel(dcnr_list_summary* out) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  dcnr_list_summary m;
  m.n_lists = m.n_lists_scored = m.n_lists_pairs = m.n_marked = m.n_bad_list = 0;
  m.n_entries = m.n_distinct_items = m.gini_num = m.n_rel_lists = 0;
  m.ild = m.mean_score = m.mean_info = m.mrr = m.gini = qnan;
  m.coverage = 0.0;
  for (int j = 0; j < GK; ++j) {
    m.hit_lists[j] = 0;
    m.hit_rate[j] = m.recall[j] = m.ndcg[j] = qnan;
  }
  *out = m;
}

}  // namespace

static size_t list_metrics_ws_bytes(int64_t R, int64_t n_items) {
  if (R <= 0 || n_items < 1) return 0;
  return lcarve(R, n_items, nullptr).total;
}

static dcnr_status eval_list_metrics(const int64_t* rows, int64_t n, const int64_t* offsets,
                                     const int32_t* counts, int64_t R, int32_t at, const float* table,
                                     const float* inv_norms, int32_t d, int64_t n_items, const float* scores,
                                     const double* info, const int64_t* rel_rows, int64_t n_rel_rows,
                                     const int64_t* rel_offsets, const int32_t* ks_host, int32_t n_k,
                                     const double* discount, const double* ideal, dcnr_list_summary* out,
                                     dcnr_list_record* per_list, void* ws, hipStream_t s) {
  if (R == 0) {
    hipLaunchKernelGGL(list_empty_kernel, dim3(1), dim3(1), 0, s, out);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  LArgs a;
  a.rows = rows; a.n = n; a.offsets = offsets; a.counts = counts; a.R = R; a.at = at;
  a.table = table; a.inv = inv_norms; a.d = d; a.n_items = n_items;
  a.scores = scores; a.info = info;
  a.rel_rows = rel_rows; a.n_rel_rows = n_rel_rows; a.rel_offsets = rel_offsets;
  a.ks.nk = rel_offsets ? n_k : 0;
  for (int j = 0; j < GK; ++j) a.ks.k[j] = j < a.ks.nk ? ks_host[j] : 0;
  a.discount = discount; a.ideal = ideal; a.per_list = per_list;
  const LWs w = lcarve(R, n_items, ws);
  TRY(fill_zero(ws, w.clear, s));
  const bool wave = at <= 32;
  const int lpb = wave ? LM_NT / WAVE : 1;
  const int nb = (int)std::min<int64_t>(LM_MAXB, cdiv(R, lpb));
  // 16-byte loads where every row of the table starts on 16 bytes
  const bool vec = d % 4 == 0 && (uintptr_t)table % 16 == 0;
  const size_t lds = (size_t)lpb * at * list_row_stride(d, vec ? 4 : 1) * sizeof(float);
#define DCNR_LIST_LAUNCH(TEAM, VEC)                                                              \
  do {                                                                                           \
    TRY(set_max_dyn_lds((const void*)list_metrics_kernel<TEAM, VEC>, lds));                   \
    hipLaunchKernelGGL((list_metrics_kernel<TEAM, VEC>), dim3(nb), dim3(LM_NT), lds, s, a, w.c,  \
                       w.part);                                                                  \
  } while (0)
  if (wave && vec) DCNR_LIST_LAUNCH(WAVE, 4);
  else if (wave) DCNR_LIST_LAUNCH(WAVE, 1);
  else if (vec) DCNR_LIST_LAUNCH(LM_NT, 4);
  else DCNR_LIST_LAUNCH(LM_NT, 1);
#undef DCNR_LIST_LAUNCH
  DCNR_LAUNCH_CHECK();
  const int cb = (int)std::min<int64_t>(LC_MAXB, cdiv(n_items, LM_NT));
  hipLaunchKernelGGL(list_counts_kernel, dim3(cb), dim3(LM_NT), 0, s, w.c, n_items, R, w.h, w.misc);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(list_final_kernel, dim3(1), dim3(LF_NT), 0, s, w.part, nb, R, n_items, w.h, w.misc,
                     a.ks, scores != nullptr, info != nullptr, out);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // namespace dcnr

using namespace dcnr;

// the workspace check of the three entries: too small, then null
static dcnr_status metrics_ws_check(const char* who, const void* ws, size_t ws_bytes, size_t need) {
  if (ws_bytes < need) {
    set_error("%s: workspace too small: %zu < %zu", who, ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  if (need && !ws) {
    set_error("%s: null workspace", who);
    return DCNR_BAD_ARG;
  }
  return DCNR_OK;
}

extern "C" {

size_t dcnr_eval_metrics_workspace_size(int64_t n) { return metrics_ws_bytes(n); }

dcnr_status dcnr_eval_metrics(const float* logits, const float* labels, int64_t n, dcnr_metrics* out,
                              void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  if (n < 0 || n >= ((int64_t)1 << 31) || !out || (n > 0 && (!logits || !labels))) {
    set_error("dcnr_eval_metrics: bad argument");
    return DCNR_BAD_ARG;
  }
  TRY(metrics_ws_check("dcnr_eval_metrics", ws, ws_bytes, metrics_ws_bytes(n)));
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: the inputs once, the keys written and read once per sort pass
  TRYB(DCNR_K_HEAD, s, 8.0 * (double)n + 3.0 * 16.0 * (double)n,
       eval_metrics(logits, labels, n, out, ws, s));
  return DCNR_OK;
}

static bool group_metrics_sizes_ok(int64_t n, int64_t n_groups) {
  return n >= 0 && n < ((int64_t)1 << 31) && n_groups >= 1 && n_groups <= ((int64_t)1 << 31) - 1;
}

size_t dcnr_eval_group_metrics_workspace_size(int64_t n, int64_t n_groups) {
  return group_metrics_sizes_ok(n, n_groups) ? group_metrics_ws_bytes(n, n_groups) : 0;
}

dcnr_status dcnr_eval_group_metrics(const float* logits, const float* labels, const int64_t* groups,
                                    int64_t n, int64_t n_groups, const int32_t* ks, int32_t n_k,
                                    const double* discount, const double* ideal,
                                    dcnr_group_summary* out, dcnr_group_record* per_group, void* ws,
                                    size_t ws_bytes, dcnr_stream_t stream) {
  bool ok = group_metrics_sizes_ok(n, n_groups) && out && n_k >= 0 && n_k <= DCNR_GROUP_MAX_K &&
            (n == 0 || (logits && labels && groups)) && (n_k == 0 || (ks && discount && ideal));
  for (int j = 0; ok && j < n_k; ++j)
    ok = ks[j] >= 1 && ks[j] <= (1 << 20) && (j == 0 || ks[j] > ks[j - 1]);
  if (!ok) {
    set_error("dcnr_eval_group_metrics: bad argument");
    return DCNR_BAD_ARG;
  }
  TRY(metrics_ws_check("dcnr_eval_group_metrics", ws, ws_bytes, group_metrics_ws_bytes(n, n_groups)));
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: the inputs once, the keys written and read once per sort pass
  // and read by the two walks
  const double passes = (double)group_passes(n_groups);
  TRYB(DCNR_K_HEAD, s, 16.0 * (double)n + (passes + 1.0) * 16.0 * (double)n,
       eval_group_metrics(logits, labels, groups, n, n_groups, ks, n_k, discount, ideal, out,
                          per_group, ws, s));
  return DCNR_OK;
}

static bool list_metrics_shape_ok(int64_t R, int64_t n_items) {
  return R <= ((int64_t)1 << 22) && n_items < ((int64_t)1 << 31);
}

size_t dcnr_eval_list_metrics_workspace_size(int64_t R, int64_t n_items) {
  return list_metrics_shape_ok(R, n_items) ? list_metrics_ws_bytes(R, n_items) : 0;
}

dcnr_status dcnr_eval_list_metrics(const int64_t* rows, int64_t n, const int64_t* offsets,
                                   const int32_t* counts, int64_t R, int32_t at,
                                   const float* table, const float* inv_norms, int32_t d,
                                   int64_t n_items, const float* scores, const double* info,
                                   const int64_t* rel_rows, int64_t n_rel_rows,
                                   const int64_t* rel_offsets, const int32_t* ks, int32_t n_k,
                                   const double* discount, const double* ideal,
                                   dcnr_list_summary* out, dcnr_list_record* per_list, void* ws,
                                   size_t ws_bytes, dcnr_stream_t stream) {
  bool ok = R >= 0 && n >= 0 && n_rel_rows >= 0 && n_items >= 1 && at >= 1 && at <= 128 && d >= 1 &&
            d <= 256 && out && n_k >= 0 && n_k <= DCNR_GROUP_MAX_K &&
            (R == 0 || (offsets && table && inv_norms)) && (R == 0 || n == 0 || rows) &&
            (!rel_offsets || n_rel_rows == 0 || rel_rows) && (n_k == 0 || ks) &&
            (n_k == 0 || !rel_offsets || (discount && ideal));
  for (int j = 0; ok && j < n_k; ++j) ok = ks[j] >= 1 && ks[j] <= at && (j == 0 || ks[j] > ks[j - 1]);
  if (!ok) {
    set_error("dcnr_eval_list_metrics: bad argument");
    return DCNR_BAD_ARG;
  }
  if (!list_metrics_shape_ok(R, n_items) || n > ((int64_t)1 << 30)) {
    set_error("dcnr_eval_list_metrics: R %lld > 2^22, n %lld > 2^30 or n_items %lld >= 2^31",
              (long long)R, (long long)n, (long long)n_items);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  TRY(metrics_ws_check("dcnr_eval_list_metrics", ws, ws_bytes, list_metrics_ws_bytes(R, n_items)));
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: the measured rows of the table at most once each, the
  // row ids, the counts cleared, written and read
  TRYB(DCNR_K_HEAD, s, (double)std::min<int64_t>(n, R * at) * (4.0 * d + 12.0) + 12.0 * (double)n_items,
       eval_list_metrics(rows, n, offsets, counts, R, at, table, inv_norms, d, n_items, scores, info,
                         rel_rows, n_rel_rows, rel_offsets, ks, n_k, discount, ideal, out, per_list,
                         ws, s));
  return DCNR_OK;
}

}  // extern "C"
