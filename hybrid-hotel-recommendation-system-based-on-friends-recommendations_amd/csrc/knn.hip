// Cosine k-nearest-neighbour search over the item-embedding table
// (candidate generation, main.py:196-203 and /similar_items main.py:299-302,
// replacing sklearn NearestNeighbors(metric='cosine', algorithm='brute')).
//
//   dist(q, x) = clip(1 - <q/|q|, x/|x|>, 0, 2)          (fp32)
//   result: k smallest per query, ascending by (dist, row index)
//
// Four scans, chosen per shape in cosine_topk():
//  * scan v4 (d = 32 / 64, k <= 32; every N and Q but single queries over
//    small tables): a bf16-MFMA coarse
//    cosine over a fit-time bf16 copy of the normalised rows, with an
//    admission bound that provably keeps every true neighbour, then exact
//    fp32 distances of the admitted rows and an exact selection -- the
//    production path of configs[4] (section "scan v4" below);
//  * scan v3 (Q >= 16, d % 16 == 0, d not 32 / 64): exact fp32-MFMA scan
//    into per-slice k-lists;
//  * scan v2 (d <= 64, k <= 32): exact VALU scan with wave-register lists --
//    small Q (v4's per-query exact fallback is the same scan inside one
//    block, the same distance arithmetic);
//  * scan v1 (the rest, k <= 64): the original streaming scan below --
//    each workgroup scans one contiguous row slice; every thread owns one
//    row per step (16-B loads), computes QT dots against the LDS-resident
//    normalised queries, and appends rows that beat the query's running
//    k-th-best threshold into a per-query LDS candidate buffer, compacted
//    by an in-LDS bitonic sort (ties by index: deterministic).
// v1-v3 end in merge_kernel (the slices' k-lists per query).
//
// cosine_topk_within() is the same search over a listed subset of the rows (a
// city's hotels), per segment of queries: scan v2's / v1's loops over a row
// list, merge_kernel's block at the end (section behind cosine_topk).
//
// neighbor_table() builds the item neighbour table from these: every table
// row's own top-k, chunk by chunk, scan v3 left out (section at the end).
#include "dcnr_internal.h"

#include <cfloat>
#include <climits>
#include <type_traits>

namespace dcnr {
namespace {

constexpr int NT = 256;
constexpr int QT = 8;          // queries per workgroup tile
constexpr int CAP = 512;       // candidate buffer per query (>= k + NT)
constexpr int KMAX = 64;

struct Cand { float d; int i; };

__device__ __forceinline__ bool cless(float da, int ia, float db, int ib) {
  return da < db || (da == db && (unsigned)ia < (unsigned)ib);
}

struct CandLess {
  __device__ bool operator()(float da, int ia, float db, int ib) const { return cless(da, ia, db, ib); }
};

// bitonic sort of n2 (a power of two) entries in LDS, ascending by less (by
// default (d, i)); all NTB threads of the block participate
template <int NTB = NT, class I = int, class Less = CandLess>
__device__ void bitonic(float* cd, I* ci, int n2 = CAP, Less less = Less{}) {
  for (int k2 = 2; k2 <= n2; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n2 / 2; t += NTB) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i + j;
        const bool asc = (i & k2) == 0;
        const float a = cd[i], b = cd[p];
        const I ia = ci[i], ib = ci[p];
        const bool sw = asc ? less(b, ib, a, ia) : less(a, ia, b, ib);
        if (sw) { cd[i] = b; cd[p] = a; ci[i] = ib; ci[p] = ia; }
      }
      __syncthreads();
    }
  }
}

// The k best of nv candidates in LDS (room for the next power of two), sorted,
// to idx / dist; slots past nv read (-1, FLT_MAX) (merge_kernel's rule;
// rescore_kernel, which wrote ci / cd as they stood, always has nv >= k: at
// least k of its n >= k distances lie at or under the k-th's bin).  All NTB
// threads.
template <int NTB>
__device__ void sort_emit(float* cd, int* ci, int nv, int k, int64_t* idx, float* dist) {
  int n2 = 2;
  while (n2 < nv) n2 <<= 1;
  for (int t = nv + threadIdx.x; t < n2; t += NTB) { cd[t] = FLT_MAX; ci[t] = INT_MAX; }
  __syncthreads();
  bitonic<NTB>(cd, ci, n2);
  for (int t = threadIdx.x; t < k; t += NTB) {
    const bool ok = t < nv;
    idx[t] = ok ? (int64_t)ci[t] : -1;
    dist[t] = ok ? cd[t] : FLT_MAX;
  }
}

// Keep the best k of buffer q: sort, pad the rest with +inf, reset count/threshold.
__device__ void compact(float* cd, int* ci, int* cnt, float* thr, int k) {
  const int n = *cnt;
  for (int t = threadIdx.x; t < CAP; t += NT)
    if (t >= n) { cd[t] = FLT_MAX; ci[t] = INT_MAX; }
  __syncthreads();
  bitonic(cd, ci);
  if (threadIdx.x == 0) {
    int kept = n < k ? n : k;
    *cnt = kept;
    *thr = kept == k ? cd[k - 1] : FLT_MAX;
  }
  __syncthreads();
}


// The exact cosine distance's arithmetic, spelled out: x . q per float4
// chunk with the contraction fixed (fma(w, fma(z, fma(x, y-product)))), then
// 1 - s / |x| as one fma, clamped to [0, 2].  Written as plain expressions,
// the compiler picked which product to fuse -- and packed some chunks into
// v_pk_mul / v_pk_add, unfused -- differently at different call sites, so
// two scans could give one row distances an ulp apart.  Every exact-distance
// site (scan v1 / v2, the k-th bound, scan v4's epilogue, the exact
// fallbacks) sums dot4 over the chunks in order and ends with cos_dist.
__device__ __forceinline__ float dot4(const float4 x, const float4 q) {
  return fmaf(x.w, q.w, fmaf(x.z, q.z, fmaf(x.x, q.x, x.y * q.y)));
}
// dot4 of one row chunk x against two queries at once on packed fp32 math:
// qa = {q0.x, q1.x, q0.y, q1.y}, qb = {q0.z, q1.z, q0.w, q1.w} (the
// batched fallback's interleaved query layout); each lane of the result is
// dot4(x, q) bit for bit (v_pk_mul / v_pk_fma are pairs of the same ops)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 dot4_q2(const float4 x, const float4 qa, const float4 qb) {
  f32x2 p = f32x2{x.y, x.y} * f32x2{qa.z, qa.w};
  p = __builtin_elementwise_fma(f32x2{x.x, x.x}, f32x2{qa.x, qa.y}, p);
  p = __builtin_elementwise_fma(f32x2{x.z, x.z}, f32x2{qb.x, qb.y}, p);
  p = __builtin_elementwise_fma(f32x2{x.w, x.w}, f32x2{qb.z, qb.w}, p);
  return p;
}
__device__ __forceinline__ float cos_dist(float s, float ir) {
  return fminf(fmaxf(fmaf(-s, ir, 1.f), 0.f), 2.f);
}

// one table row (d = 4 DV) as float4 chunks: its DV loads in flight together
template <int DV>
__device__ __forceinline__ void load_row(const float* __restrict__ tab, int64_t r, float4 (&x)[DV]) {
  const float4* rp = reinterpret_cast<const float4*>(tab + r * DV * 4);
#pragma unroll
  for (int v = 0; v < DV; ++v) x[v] = rp[v];
}
// scan v2's exact distance of one row (x, its inverse norm ir) to one
// normalised query (qv): the one expression every exact path uses, so they
// agree bit for bit
template <int DV>
__device__ __forceinline__ float exact_dist(const float4 (&x)[DV], const float4* qv, float ir) {
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < DV; ++v) {
    const float4 q = qv[v];
    s += dot4(x[v], q);
  }
  return cos_dist(s, ir);
}

template <int MAXV>
__global__ __launch_bounds__(NT) void scan_kernel(const float* __restrict__ tab,
                                                  const float* __restrict__ inv, int64_t N, int d,
                                                  const float* __restrict__ q, int64_t Q, int k,
                                                  int64_t rows_per_slice, Cand* out) {
  __shared__ __attribute__((aligned(16))) float qs[QT][MAXV * 4];
  __shared__ float cd[QT][CAP];
  __shared__ int ci[QT][CAP];
  __shared__ int cnt[QT];
  __shared__ float thr[QT];
  const int slice = blockIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * QT;
  const int nq = (int)min<int64_t>(QT, Q - q0);
  // normalised queries (sklearn normalize(): zero norm -> unchanged)
  for (int i = threadIdx.x; i < QT * MAXV * 4; i += NT) (&qs[0][0])[i] = 0.f;
  __syncthreads();
  for (int qq = threadIdx.x >> 6; qq < nq; qq += NT / 64) {
    const int lane = threadIdx.x & 63;
    float s = 0.f;
    for (int i = lane; i < d; i += 64) { float v = q[(q0 + qq) * d + i]; s += v * v; }
    s = wave_sum(s);
    float in = s > 0.f ? 1.f / sqrtf(s) : 1.f;
    for (int i = lane; i < d; i += 64) qs[qq][i] = q[(q0 + qq) * d + i] * in;
  }
  if (threadIdx.x < QT) { cnt[threadIdx.x] = 0; thr[threadIdx.x] = FLT_MAX; }
  __syncthreads();

  const int64_t r0 = (int64_t)slice * rows_per_slice;
  const int64_t r1 = min(N, r0 + rows_per_slice);
  const int dv = d >> 2;
  for (int64_t base = r0; base < r1; base += NT) {
    const int64_t r = base + threadIdx.x;
    if (r < r1) {
      float4 x[MAXV];
      const float4* rp = reinterpret_cast<const float4*>(tab + r * d);
#pragma unroll
      for (int v = 0; v < MAXV; ++v) if (v < dv) x[v] = rp[v];
      const float ir = inv[r];
      for (int qq = 0; qq < nq; ++qq) {
        const float4* qp = reinterpret_cast<const float4*>(qs[qq]);
        float s = 0.f;
#pragma unroll
        for (int v = 0; v < MAXV; ++v)
          if (v < dv) {
            float4 w = qp[v];
            s += dot4(x[v], w);
          }
        float dist = cos_dist(s, ir);
        if (dist <= thr[qq]) {
          int pos = atomicAdd(&cnt[qq], 1);
          cd[qq][pos] = dist;
          ci[qq][pos] = (int)r;
        }
      }
    }
    __syncthreads();
    for (int qq = 0; qq < nq; ++qq) {
      if (cnt[qq] > CAP - NT) compact(cd[qq], ci[qq], &cnt[qq], &thr[qq], k);
    }
  }
  for (int qq = 0; qq < nq; ++qq) {
    compact(cd[qq], ci[qq], &cnt[qq], &thr[qq], k);
    Cand* o = out + ((q0 + qq) * gridDim.x + slice) * k;
    for (int t = threadIdx.x; t < k; t += NT) {
      bool ok = t < cnt[qq];
      o[t] = Cand{ok ? cd[qq][t] : FLT_MAX, ok ? ci[qq][t] : INT_MAX};
    }
  }
}

// ---------------------------------------------------------------- scan v2
// Wave-private candidate lists (no block barriers in the scan): a block owns a
// contiguous row slice and a tile of up to K2_QT queries; each wave takes 64
// rows per step (one row per lane, in registers), computes the distance to
// every query of the tile (normalised queries broadcast from LDS), and
// appends rows that beat its running k-th best for that query with
// ballot + mbcnt (no atomics).  A full list (K2_CAP) is compacted by a
// 64-lane register bitonic sort that keeps the k best and sets the threshold.
// Rows arrive in increasing index order per wave, so the strict test
// "dist < threshold" keeps ties ordered by row index.  Output: one k-list per
// (query, block, wave), merged by merge_kernel.  Block -> (slice, query tile)
// is XCD-grouped: the blocks that share a row slice run on one XCD, whose L2
// serves the repeated reads of the slice.
constexpr int K2_NT = 256, K2_WPB = K2_NT / 64, K2_QT = 32, K2_CAP = 64, K2_KMAX = 32;
// queries from which the fp32-MFMA scan (v3) is used: measured on one box
// (tools/ab_knn.sh, 1M x 64, k = 11), the VALU scan is faster up to Q = 8
// (Q=4: 73 vs 104 us, Q=8: 97 vs 116 us), the MFMA scan from Q = 16
// (138 vs 153 us; Q=32: 189 vs 265 us)
constexpr int MFMA_MIN_Q = 16;

__device__ __forceinline__ void wave_sort64(float& d, int& i, int lane) {
#pragma unroll
  for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const float od = __shfl_xor(d, j, 64);
      const int oi = __shfl_xor(i, j, 64);
      const bool up = (lane & k2) == 0, lower = (lane & j) == 0;
      const bool other_less = cless(od, oi, d, i);
      if ((lower == up) == other_less) { d = od; i = oi; }
    }
  }
}

// Keep the k best of one wave's list: sorted into slots [0, k).  Returns the
// new count; *kth = the k-th best distance (FLT_MAX while fewer than k).
// The list is written and read by different lanes of one wave: the wavefront
// fences order those LDS accesses for the compiler (the hardware keeps one
// wave's LDS operations in order).
__device__ __forceinline__ int wave_compact(float* cd, int* ci, int c, int k, int lane,
                                            float* kth) {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  float d = lane < c ? cd[lane] : FLT_MAX;
  int i = lane < c ? ci[lane] : INT_MAX;
  wave_sort64(d, i, lane);
  if (lane < k) { cd[lane] = d; ci[lane] = i; }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const float kd = __shfl(d, k - 1, 64);
  *kth = c >= k ? kd : FLT_MAX;
  return c < k ? c : k;
}

// admit (dd, r) into one wave's k-list (K2_CAP LDS slots, compacted when
// full) while strictly under its k-th best: the per-wave list protocol of
// scan v2 and the exact fallbacks
__device__ __forceinline__ void wave_admit(float* lcd, int* lci, int& c, float& th, int k, int lane,
                                           bool ok, float dd, int64_t r) {
  bool pass = ok && dd < th;
  uint64_t m = __ballot(pass);
  while (m) {
    const int room = K2_CAP - c;
    if (room == 0) {
      c = wave_compact(lcd, lci, c, k, lane, &th);
      pass = pass && dd < th;
      m = __ballot(pass);
      continue;
    }
    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
    if (pass && rank < room) {
      lcd[c + rank] = dd;
      lci[c + rank] = (int)r;
    }
    const int n = __popcll(m);
    c += n < room ? n : room;
    pass = pass && rank >= room;
    m = __ballot(pass);
  }
}

// merge NW sorted k-lists held in LDS (list ww at cd / ci + ww * lstride, its
// count at cnt[ww * cstride]) in one wave, two lists per 64-lane sort
// (k <= 32): the k best by (distance, row) in lanes [0, k)
template <int NW>
__device__ __forceinline__ void wave_merge_lists(const float* cd, const int* ci, const int* cnt, int lstride,
                                                 int cstride, int k, int lane, float& d, int& i) {
  d = FLT_MAX;
  i = INT_MAX;
  for (int ww = 0; ww < NW; ++ww) {
    const int cw = cnt[ww * cstride];
    const int sl = ww == 0 ? lane : lane - k;
    if (ww == 0 || lane >= k) {
      const bool has = sl >= 0 && sl < k && sl < cw;
      d = has ? cd[ww * lstride + sl] : FLT_MAX;
      i = has ? ci[ww * lstride + sl] : INT_MAX;
    }
    if (ww > 0) wave_sort64(d, i, lane);
  }
}

// the same merge over nl k-lists of one query in global memory (list l at
// pd / pi + l * k; a list of fewer than k rows is padded with FLT_MAX, whose
// row id reads as INT_MAX)
__device__ __forceinline__ Cand wave_merge_global_lists(const float* pd, const int64_t* pi, int64_t l0, int nl,
                                                        int k, int lane) {
  float d = FLT_MAX;
  int i = INT_MAX;
  for (int l = 0; l < nl; ++l) {
    const int sl = l == 0 ? lane : lane - k;
    if (l == 0 || lane >= k) {
      const bool has = sl >= 0 && sl < k;
      const float dv = has ? pd[(l0 + l) * k + sl] : FLT_MAX;
      const int64_t iv = has ? pi[(l0 + l) * k + sl] : (int64_t)INT_MAX;
      d = dv;
      i = dv == FLT_MAX ? INT_MAX : (int)iv;
    }
    if (l > 0) wave_sort64(d, i, lane);
  }
  return Cand{d, i};
}

template <int DV>
__global__ __launch_bounds__(K2_NT) void scan2_kernel(const float* __restrict__ tab,
                                                      const float* __restrict__ inv, int64_t N,
                                                      const float* __restrict__ qn, int64_t Q,
                                                      int k, int64_t rows_per_block, int nslices,
                                                      int qtiles, Cand* out,
                                                      const float* __restrict__ thr0) {
  __shared__ float cd[K2_WPB][K2_QT][K2_CAP];
  __shared__ int ci[K2_WPB][K2_QT][K2_CAP];
  __shared__ int cntl[K2_WPB][K2_QT];
  const int bid = blockIdx.x;
  const int tile = (bid / 8) % qtiles;
  const int slice = (bid % 8) + 8 * (bid / (8 * qtiles));
  if (slice >= nslices) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t q0 = (int64_t)tile * K2_QT;
  const int nq = (int)min<int64_t>(K2_QT, Q - q0);
  // the normalised queries are read with wave-uniform addresses: scalar
  // loads into SGPRs, one FMA operand each (no LDS broadcast traffic)
  const float4* qv = reinterpret_cast<const float4*>(qn + q0 * DV * 4);
  // per-query list count and threshold of this wave: lane qq holds query qq's;
  // bound0: the admission bound (kth_bound_kernel), lane qq holding query qq's
  int cntv = 0;
  float thrv = FLT_MAX;
  const float bound0 = lane < nq ? thr0[q0 + lane] : FLT_MAX;
  const int64_t r0 = (int64_t)slice * rows_per_block;
  const int64_t r1 = min(N, r0 + rows_per_block);
  for (int64_t base = r0 + 64 * w; base < r1; base += 64 * K2_WPB) {
    const int64_t r = base + lane;
    const bool ok = r < r1;
    const int64_t rc = ok ? r : r0;
    float4 x[DV];
    load_row<DV>(tab, rc, x);
    const float ir = inv[rc];
    for (int qq = 0; qq < nq; ++qq) {
      const float dist = exact_dist<DV>(x, qv + qq * DV, ir);
      float th = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thrv), qq));
      const float b0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bound0), qq));
      const bool cand = ok && dist <= b0;
      if (!__ballot(cand && dist < th)) continue;   // (nothing to append: the usual case)
      int c = __builtin_amdgcn_readlane(cntv, qq);
      wave_admit(cd[w][qq], ci[w][qq], c, th, k, lane, cand, dist, r);
      cntv = lane == qq ? c : cntv;
      thrv = lane == qq ? th : thrv;
    }
  }
  // each wave sorts its lists; then wave (qq mod 4) merges the four k-lists of
  // query qq in registers (2k <= 64 lanes per step) into the block's list
  for (int qq = 0; qq < nq; ++qq) {
    float th;
    const int c = wave_compact(cd[w][qq], ci[w][qq], __builtin_amdgcn_readlane(cntv, qq), k,
                               lane, &th);
    if (lane == 0) cntl[w][qq] = c;
  }
  __syncthreads();
  for (int qq = w; qq < nq; qq += K2_WPB) {
    float d;
    int i;
    wave_merge_lists<K2_WPB>(cd[0][qq], ci[0][qq], &cntl[0][qq], K2_QT * K2_CAP, K2_QT, k, lane, d, i);
    Cand* o = out + ((q0 + qq) * nslices + slice) * (int64_t)k;
    if (lane < k) o[lane] = Cand{d, i};
  }
}

// ---------------------------------------------------------------- scan v3
// fp32 MFMA scoring (v_mfma_f32_16x16x4_f32, exact f32 products and sums):
// per wave, 16-row tiles of the table (A operand) against K3_QT queries
// (B operand, resident in registers, 16 per column block).  The dot product
// is order-free in k, so lane (r, g) feeds k = 16 s + 4 g + j from the float4
// chunk 4 s + g of its row: every A/B fragment comes from one 16-B load, no
// shuffles.  Output lane (q, g) holds rows 4 g .. 4 g + 3 for query q.  The
// candidate lists are the per-(wave, query) LDS lists of scan v2; appends use
// ballot over the four lanes of a query; a list above K2_CAP - 16 entries is
// compacted before the next tile (at most 16 appends per tile).
constexpr int K3_QT = 32, K3_CB = K3_QT / 16;

template <int DV>
__global__ __launch_bounds__(K2_NT) void scan3_kernel(const float* __restrict__ tab,
                                                      const float* __restrict__ inv, int64_t N,
                                                      const float* __restrict__ qn, int64_t Q,
                                                      int k, int64_t rows_per_block, int nslices,
                                                      int qtiles, Cand* out,
                                                      const float* __restrict__ thr0) {
  constexpr int S4 = DV / 4;
  __shared__ float cd[K2_WPB][K3_QT][K2_CAP];
  __shared__ int ci[K2_WPB][K3_QT][K2_CAP];
  __shared__ int cntl[K2_WPB][K3_QT];
  const int bid = blockIdx.x;
  const int tile = (bid / 8) % qtiles;
  const int slice = (bid % 8) + 8 * (bid / (8 * qtiles));
  if (slice >= nslices) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t q0 = (int64_t)tile * K3_QT;
  const int nq = (int)min<int64_t>(K3_QT, Q - q0);
  float4 bq[K3_CB][S4];
#pragma unroll
  for (int cb = 0; cb < K3_CB; ++cb) {
    const int64_t qi = q0 + 16 * cb + r16;
#pragma unroll
    for (int s = 0; s < S4; ++s)
      bq[cb][s] = qi < Q ? reinterpret_cast<const float4*>(qn + qi * DV * 4)[4 * s + g]
                         : float4{0.f, 0.f, 0.f, 0.f};
  }
  float thr[K3_CB], bnd[K3_CB];
  int cnt[K3_CB];
#pragma unroll
  for (int cb = 0; cb < K3_CB; ++cb) {
    thr[cb] = FLT_MAX;
    cnt[cb] = 0;
    const int64_t qi = q0 + 16 * cb + r16;
    bnd[cb] = qi < Q ? thr0[qi] : FLT_MAX;
  }
  const uint64_t qmask = 0x0001000100010001ull << r16;
  const uint64_t below = (1ull << lane) - 1;
  const int64_t r0 = (int64_t)slice * rows_per_block;
  const int64_t r1 = min(N, r0 + rows_per_block);
  // one-tile software pipeline: the next tile's rows are in flight while this
  // tile's MFMAs and appends run
  auto load_tile = [&](int64_t b, float4 (&x)[S4], float (&v)[4]) {
    const int64_t ra = b + r16;
    const int64_t rac = ra < r1 ? ra : r0;
#pragma unroll
    for (int s = 0; s < S4; ++s) x[s] = reinterpret_cast<const float4*>(tab + rac * DV * 4)[4 * s + g];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = inv[b + 4 * g + i < r1 ? b + 4 * g + i : r0];
  };
  float4 xa[S4];
  float iv[4];
  if (r0 + 16 * w < r1) load_tile(r0 + 16 * w, xa, iv);
  for (int64_t base = r0 + 16 * w; base < r1; base += 16 * K2_WPB) {
    float4 xn[S4];
    float ivn[4];
    if (base + 16 * K2_WPB < r1) load_tile(base + 16 * K2_WPB, xn, ivn);
    const int64_t rb = base + 4 * g;
#pragma unroll
    for (int cb = 0; cb < K3_CB; ++cb) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < S4; ++s) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s].x, bq[cb][s].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s].y, bq[cb][s].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s].z, bq[cb][s].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s].w, bq[cb][s].w, acc, 0, 0, 0);
      }
      float* lcd = cd[w][16 * cb + r16];
      int* lci = ci[w][16 * cb + r16];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float dist = fminf(fmaxf(1.f - acc[i] * iv[i], 0.f), 2.f);
        const bool pass = rb + i < r1 && dist < thr[cb] && dist <= bnd[cb] && 16 * cb + r16 < nq;
        const uint64_t m = __ballot(pass);
        if (!m) continue;
        const uint64_t mq = m & qmask;
        if (pass) {
          const int slot = cnt[cb] + __popcll(mq & below);
          lcd[slot] = dist;
          lci[slot] = (int)(rb + i);
        }
        cnt[cb] += __popcll(mq);
      }
      // keep room for the next tile's (at most 16) appends per query
      uint64_t need = __ballot(lane < 16 && cnt[cb] > K2_CAP - 16);
      while (need) {
        const int q = __builtin_ctzll(need);
        need &= need - 1;
        float th;
        const int c2 = wave_compact(cd[w][16 * cb + q], ci[w][16 * cb + q],
                                    __builtin_amdgcn_readlane(cnt[cb], q), k, lane, &th);
        if (r16 == q) { cnt[cb] = c2; thr[cb] = th; }
      }
    }
#pragma unroll
    for (int s = 0; s < S4; ++s) xa[s] = xn[s];
#pragma unroll
    for (int i = 0; i < 4; ++i) iv[i] = ivn[i];
  }
#pragma unroll
  for (int cb = 0; cb < K3_CB; ++cb)
    for (int q = 0; q < 16 && 16 * cb + q < nq; ++q) {
      float th;
      const int c = wave_compact(cd[w][16 * cb + q], ci[w][16 * cb + q],
                                 __builtin_amdgcn_readlane(cnt[cb], q), k, lane, &th);
      if (lane == 0) cntl[w][16 * cb + q] = c;
    }
  __syncthreads();
  for (int qq = w; qq < nq; qq += K2_WPB) {
    float d;
    int i;
    wave_merge_lists<K2_WPB>(cd[0][qq], ci[0][qq], &cntl[0][qq], K3_QT * K2_CAP, K3_QT, k, lane, d, i);
    Cand* o = out + ((q0 + qq) * nslices + slice) * (int64_t)k;
    if (lane < k) o[lane] = Cand{d, i};
  }
}

// Per-query admission bound for the scans: the k-th smallest distance over
// the first TH_S rows of the table (+ TH_MARGIN, covering rounding differences
// between this pass and the scan kernels).  Every row of the true top-k has a
// distance <= the k-th best of any subset, so rows above the bound are never
// appended: the wave lists then see a handful of rows instead of refilling
// and re-sorting while their own thresholds converge.
constexpr int TH_S = 512;   // sample rows: the bound sits near quantile k / TH_S
constexpr float TH_MARGIN = 1e-5f;

// k-th smallest of a block's keys -- the bits of non-negative floats, which
// order like the values -- by a 2-pass radix select over exponent + 7
// mantissa bits: returns the upper edge of the selected bin (>= the exact
// k-th value, within 2^-7 relative), or 0xffffffff when the block holds
// nkeys < k keys (block-uniform; as the callers' own checks said before).
// count(hist, mask, prefix, sh) adds the calling thread's keys with
// (key & mask) == prefix to hist[(key >> sh) & 255]: the callers hold their
// keys differently (registers, LDS) and count them accordingly.
// Every thread of a block of at least 256 threads (the bins are zeroed one
// per thread) calls it.  The LDS words are static: one set per kernel, shared
// by every call in it, so the barrier at the end lets a kernel call it again.
template <class Count>
__device__ __forceinline__ unsigned radix_select_kth(int k, int nkeys, Count count) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sel_prefix, sel_need;
  if (threadIdx.x == 0) { sel_prefix = 0; sel_need = (unsigned)k; }
  unsigned mask = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int sh = 24 - 8 * pass;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    const unsigned prefix = sel_prefix;
    count(hist, mask, prefix, sh);
    __syncthreads();
    // wave 0 scans the bins (4 per lane), picks the one holding the need-th
    // key and narrows prefix / need to it
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      const unsigned need = sel_need;
      unsigned h[4], sum = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) { h[b] = hist[4 * lane + b]; sum += h[b]; }
      unsigned incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
      }
      unsigned cum = incl - sum;
      if (cum < need && need <= incl) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          if (cum + h[b] >= need) {
            sel_prefix = prefix | ((unsigned)(4 * lane + b) << sh);
            sel_need = need - cum;
            break;
          }
          cum += h[b];
        }
      }
    }
    mask |= 255u << sh;
    __syncthreads();
  }
  const unsigned r = nkeys < k ? 0xffffffffu : (sel_prefix | 0xffffu);
  __syncthreads();
  return r;
}

// Block qq: normalises query qq (sklearn normalize(): zero norm -> unchanged;
// written to qn for the scan) and takes the k-th smallest sample distance
// (radix_select_kth: an upper bound within 2^-7 relative of the exact k-th
// value; a sample of fewer than k rows has the bound +inf).
template <int DV, int NTB = 256>
__global__ __launch_bounds__(NTB) void kth_bound_kernel(const float* __restrict__ tab,
                                                        const float* __restrict__ inv, int64_t N,
                                                        const float* __restrict__ q, float* qn,
                                                        int k, float* thr0) {
  constexpr int PT = TH_S / NTB;
  constexpr int d = DV * 4;   // <= 64: one element per lane
  __shared__ __attribute__((aligned(16))) float qs[d];
  const int64_t qq = blockIdx.x;
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const float v = lane < d ? q[qq * d + lane] : 0.f;
    const float ss = wave_sum(v * v);
    const float in = ss > 0.f ? 1.f / sqrtf(ss) : 1.f;
    if (lane < d) {
      qs[lane] = v * in;
      qn[qq * d + lane] = v * in;
    }
  }
  __syncthreads();
  const float4* qv = reinterpret_cast<const float4*>(qs);
  const int S = (int)min<int64_t>(N, TH_S);
  unsigned key[PT];
#pragma unroll 4
  for (int j = 0; j < PT; ++j) {
    const int t = threadIdx.x + j * NTB;
    float dist = FLT_MAX;
    if (t < S) {
      float4 x[DV];
      load_row<DV>(tab, t, x);
      // exact_dist's expression, written out: through the call -- the
      // inverse norm loaded before the dot or after it -- the kernel took up
      // to 98 VGPRs for 66 (occupancy 4 for 7 at DV = 16)
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const float4 q = qv[v];
        s += dot4(x[v], q);
      }
      dist = cos_dist(s, inv[t]);
    }
    key[j] = __float_as_uint(dist) & 0x7fffffffu;   // >= 0: bits order like values
  }
  const unsigned tk = radix_select_kth(k, S, [&](unsigned* hist, unsigned mask, unsigned prefix, int sh) {
#pragma unroll
    for (int j = 0; j < PT; ++j)
      if ((key[j] & mask) == prefix) atomicAdd(&hist[(key[j] >> sh) & 255u], 1u);
  });
  if (threadIdx.x == 0) {
    const float kth = __uint_as_float(tk);   // (NaN: S < k)
    thr0[qq] = !(kth < 2.5f) ? FLT_MAX : kth + TH_MARGIN;
  }
}

// ---------------------------------------------------------------- scan v4
// Every table and query count (d = 32 or 64): bf16-MFMA coarse scoring of
// every (row, query) pair + exact fp32 re-scoring of the rows it admits.
//
// The coarse cosine is sum_i bf16(x_i * inv_r) * bf16(q_i / |q|), fp32
// accumulation (v_mfma_f32_16x16x32_bf16: 16x the fp32-MFMA rate).  bf16
// keeps 8 significant bits, so each factor carries a relative rounding error
// <= 2^-8 (1 + 2^-8 rounds to 1 or to 1 + 2^-7), each product <= 2^-7 + 2^-16
// and, with xh = x inv_r and qh = q / |q|,
//   |coarse - exact| <= (2^-7 + 2^-16) sum_i |xh_i qh_i| + fp32 slack
//                    <= 2^-7 + 2^-16 + fp32 slack < V4_EPS
// on the distance: the sum is <= |xh| |qh| = 1 (Cauchy-Schwarz), and the
// bound is approached when every element sits just off a bf16 midpoint with
// the errors' signs aligned (tests/knn_rounding_cases.py builds such rows:
// 0.0064 at d = 32; random tables stay near 4e-4, the errors cancelling).
// The fp32 slack -- the MFMA's accumulation of d <= 64 exact bf16 products,
// the exact distance's own d fmas, the rounding of x inv_r and q / |q|, each a
// few 2^-24 -- stays under 2e-5; V4_EPS leaves 7e-5 for it.
// Every row of the exact top-k has exact distance <= E_k (the k-th best)
// <= T0 (the k-th best of a V4_S-row exact sample: any subset's k-th best
// bounds the table's), hence coarse distance <= T0 + V4_EPS: admitting the
// rows under that bound keeps every true neighbour, ties included.  T0 comes
// from bound5_kernel (exact distances of the sample rows, per-block k-lists,
// merged by the last-arriving block).  The admitted rows (~N k / V4_S per
// query) are appended to a per-query list with their exact fp32 distances
// (scan v2's arithmetic, computed in scan4's epilogue); rescore_kernel
// selects the k best by (distance, row) -- however many rows share the
// k-th's bin, the whole list at most.  A query whose list overflows V4_CAP
// (the count word carries V4_OVF when a block's wave list ran out of room)
// is answered by an exact scan of the whole table in rescore blocks (scan
// v2's per-wave lists and arithmetic; split over up to V4_FMAX blocks per
// query for Q <= V4_FQ): no batch-wide flag, no gated launches behind the
// chain.  Three launches per call: bound5, scan4, rescore.
constexpr float V4_EPS = 0.0079f;   // > 2^-7 + 2^-16 = 0.0078278 (+ the fp32 slack)
static_assert(V4_EPS > 0.0078125f + 0.0000152587890625f + 2e-5f, "V4_EPS covers 2^-8 per bf16 factor");
constexpr int V4_S = 65536;     // sample rows for the admission bound
constexpr int V4_WPS = 3;       // min waves per SIMD of scan4 for NQB > 4
constexpr int V4_CAP = 4096;     // admitted rows per query
constexpr int V4_OVF = 1 << 30;  // count-word mark: a block dropped some of this query's rows
constexpr int V4_QC = 256;       // queries per block (LDS: V4_QC x d bf16)
// table rows per block: few query blocks -> long blocks (the per-block
// prologue and epilogue amortised; measured 69 vs 78 us at Q = 32).  Many
// (NQB > 4: 16-32 KB of query fragments staged per block) -> about two blocks
// per CU, 512-2048 rows: Q = 256 over 1M rows 134 us against 146 at a fixed
// 512 (1954 blocks), 145 at 1024, 180 at 4096 (245 blocks, CUs left idle);
// profiles/lab/r04zz_knn_rpb_ab.txt.  A wave's list fill (rows x queries x
// admission rate, ~50 of 512 at 2048 rows) stays well inside V4_WL.
inline int v4_rpb(int nqb, int64_t N) {
  return nqb <= 4 ? 2048 : (int)std::min<int64_t>(2048, std::max<int64_t>(512, rup(cdiv(N, 512), 64)));
}
constexpr int64_t V4_Q1_N = 800000;   // a single query takes scan v2 below this many rows
                                      // (from Q = 2: 60-66 us for Q <= 8 against 65-98 on scan v2)

// k-th smallest of n distances (>= 0) held in LDS (radix_select_kth: the
// upper edge of the k-th's bin, or 0xffffffff when n < k).  Every thread of
// the block calls it.
template <int NTB>
__device__ unsigned block_select_kth(const float* v, int n, int k) {
  return radix_select_kth(k, n, [&](unsigned* hist, unsigned mask, unsigned prefix, int sh) {
    // distances crowd into a few bins (one exponent spans a factor of 2), so
    // equal bins of a wave are counted with one atomic (up to 4 bins per
    // wave-instruction; the rest of the lanes add one each): plain per-lane
    // atomics serialised ~n times on the hottest bin
    const int lane = threadIdx.x & 63;
    for (int i0 = threadIdx.x - lane; i0 < n; i0 += NTB) {
      const int i = i0 + lane;
      const unsigned key = i < n ? __float_as_uint(v[i]) : 0u;
      const bool valid = i < n && (key & mask) == prefix;
      const unsigned bin = (key >> sh) & 255u;
      uint64_t act = __ballot(valid);
      for (int it = 0; act && it < 4; ++it) {
        const int leader = __builtin_ctzll(act);
        const unsigned lb = (unsigned)__shfl((int)bin, leader, 64);
        const uint64_t same = __ballot(valid && bin == lb) & act;
        if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
        act &= ~same;
      }
      if ((act >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
    }
  });
}

constexpr int B4_T = 1024;   // threads of the per-query v4 kernels

// one 16-row x 32-k bf16 A fragment of lane (r16, g): row r, k in
// [32 ks + 8 g, +8), scaled by the row's inverse norm
template <int KS>
__device__ __forceinline__ void v4_load_rows(const float* __restrict__ tab, int64_t r, float4 (&x)[KS][2],
                                             int g) {
  const float4* rp = reinterpret_cast<const float4*>(tab + r * (KS * 32));
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    x[ks][0] = rp[ks * 8 + 2 * g];
    x[ks][1] = rp[ks * 8 + 2 * g + 1];
  }
}

// ------------------------------------------------- scan v4 admission bound
// Replaces the round-4 sample chain (512-row bound -> sample scan -> sample
// rescore, three launches).  bound5_kernel: B5_G blocks per group of 16
// queries each score B5_C of the first V4_S table rows with scan4's coarse
// bf16 MFMA cosine and store each query's smallest coarse distance over them;
// v4_kth_bound then takes the k-th smallest M of those block minima.  k
// distinct rows (one per block) have coarse distance <= M, hence exact
// distance <= M + V4_EPS, so E_k <= T0 = M + V4_EPS: the same kind of bound
// the exact sample k-th gave (scan4 admits coarse <= T0 + V4_EPS), a rank or
// two looser when two of the sample's k best share a block.  The minima are
// merged where they are used -- in scan4's prologue for up to V4_MQ queries,
// by bound5_merge_kernel above that -- so no block waits on another (a
// last-arriving-block merge cost a device-scope release per block: 140 us
// at Q = 256, profiles/lab/r05_knn_bound_lab.txt).  Blocks of column 0 also
// write the normalised fp32 / bf16 queries (kth_bound_kernel's arithmetic)
// and zero the list counts for scan4.
constexpr int B5_C = 512;           // sample rows per block (4 waves x 8 row tiles)
constexpr int B5_G = V4_S / B5_C;   // blocks per query group (<= 128: two minima per lane)
constexpr int B5_QG = 4;            // 16-query groups per block past V4_MQ queries (rows loaded once
                                    // for them; at or under V4_MQ one group per block)
constexpr int V4_MQ = 32;           // queries up to which scan4 merges the minima itself
static_assert(B5_G <= 128, "the merge holds two block minima per lane");

// one query's ng block minima as two per lane (block g: lane g % 64, slot g / 64)
struct Mins2 { unsigned u0, u1; };
__device__ __forceinline__ Mins2 v4_load_mins(const float* mq, int ng, int lane) {
  return Mins2{lane < ng ? __float_as_uint(mq[lane]) : 0x7f7fffffu,
               lane + 64 < ng ? __float_as_uint(mq[lane + 64]) : 0x7f7fffffu};
}
// wave-wide: the admission bounds of MQ queries from their block minima:
// the k-th smallest by a bitwise search over their non-negative float bits,
// down to 10 mantissa bits, and the upper edge of that bin (>= the k-th,
// within 2^-10 relative: 5e-4 at the usual bounds against V4_EPS = 0.0079).
// The MQ searches are interleaved (each step's ballot -> count -> select is
// otherwise one dependent chain).  Every lane returns the bounds.
constexpr int V4_LOWBIT = 13;
template <int MQ>
__device__ __forceinline__ void v4_kth_bounds(const Mins2 (&m)[MQ], int ng, int k, float (&out)[MQ]) {
  unsigned ans[MQ];
#pragma unroll
  for (int j = 0; j < MQ; ++j) ans[j] = 0;
  for (int b = 30; b >= V4_LOWBIT; --b) {
#pragma unroll
    for (int j = 0; j < MQ; ++j) {
      const unsigned t = ans[j] | (1u << b);
      if (__popcll(__ballot(m[j].u0 < t)) + __popcll(__ballot(m[j].u1 < t)) < k) ans[j] = t;
    }
  }
#pragma unroll
  for (int j = 0; j < MQ; ++j) {
    const float M = __uint_as_float(ans[j] | ((1u << V4_LOWBIT) - 1));
    out[j] = ng >= k && M < 2.5f ? M + V4_EPS + TH_MARGIN : FLT_MAX;
  }
}

template <int KS, bool PK, int QG>
__global__ __launch_bounds__(256) void bound5_kernel(const float* __restrict__ tab, const float* __restrict__ inv,
                                                     const bf16* __restrict__ tb, int64_t N,
                                                     const float* __restrict__ q, int64_t Q, float* qn,
                                                     bf16* qb, int* qcnt, float* mins) {
  constexpr int D = KS * 32;    // 32 or 64: one query element per lane
  constexpr int U = B5_C / 64;  // row tiles per wave
  constexpr int QB = 16 * QG;
  __shared__ __attribute__((aligned(16))) float qs[QB][D];
  __shared__ float wbest[4][QB];
  const int g = blockIdx.x;
  const int64_t q0 = (int64_t)blockIdx.y * QB;
  const int nq = (int)min<int64_t>(QB, Q - q0);
  const int ngr = (nq + 15) / 16;   // 16-query groups present
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, gl = lane >> 4;
  const int64_t S = min<int64_t>(N, V4_S);
  // the block's row tiles first (wave w: rows r0 + 16 u + r16), as scan4 loads them
  const int64_t r0 = (int64_t)g * B5_C + (B5_C / 4) * w;
  using Frag = typename std::conditional<PK, bf16x8[KS], float4[KS][2]>::type;
  Frag x[U];
  float iv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t r = min<int64_t>(r0 + 16 * u + r16, S - 1);
    if constexpr (PK) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) x[u][ks] = *reinterpret_cast<const bf16x8*>(tb + r * D + ks * 32 + 8 * gl);
    } else {
      v4_load_rows<KS>(tab, r, x[u], gl);
      iv[u] = inv[r];
    }
  }
  // kth_bound_kernel's normalisation, the wave's query loads all in flight first
  float qv[QB / 4];
#pragma unroll
  for (int j = 0; j < QB / 4; ++j) {
    const int qq = w + 4 * j;
    qv[j] = qq < nq && lane < D ? q[(q0 + qq) * D + lane] : 0.f;
  }
#pragma unroll
  for (int j = 0; j < QB / 4; ++j) {
    const int qq = w + 4 * j;
    if (qq >= 16 * ngr) break;
    const float v = qv[j];
    const float ss = wave_sum(v * v);
    const float in = ss > 0.f ? 1.f / sqrtf(ss) : 1.f;
    if (lane < D) {
      qs[qq][lane] = v * in;
      if (g == 0 && qq < nq) {
        qn[(q0 + qq) * D + lane] = v * in;
        qb[(q0 + qq) * D + lane] = (bf16)(v * in);
      }
    }
    if (g == 0 && qq < nq && lane == 0) {
      qcnt[q0 + qq] = 0;
      qcnt[Q + 1 + q0 + qq] = 0;   // the fallbacks' arrival counters (rescore_kernel)
      if (q0 + qq == 0) {          // the overflow word and the batched fallback's 8 queues
        qcnt[Q] = 0;
        for (int j = 0; j < 8; ++j) qcnt[2 * Q + 2 + j] = 0;
      }
    }
  }
  __syncthreads();
  // the row tiles' A fragments (bf16, as scan4 rounds them)
  bf16x8 a[U][KS];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (PK) {
        a[u][ks] = x[u][ks];
      } else {
        const float4 p = x[u][ks][0], v = x[u][ks][1];
        const float sc = iv[u];
        a[u][ks] = bf16x8{(bf16)(p.x * sc), (bf16)(p.y * sc), (bf16)(p.z * sc), (bf16)(p.w * sc),
                          (bf16)(v.x * sc), (bf16)(v.y * sc), (bf16)(v.z * sc), (bf16)(v.w * sc)};
      }
    }
  for (int gr = 0; gr < ngr; ++gr) {
    // B fragment of lane (c = r16, gl): query 16 gr + c's k-chunk [32 ks + 8 gl, +8)
    bf16x8 bq[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4 lo = *reinterpret_cast<const float4*>(&qs[16 * gr + r16][ks * 32 + 8 * gl]);
      const float4 hi = *reinterpret_cast<const float4*>(&qs[16 * gr + r16][ks * 32 + 8 * gl + 4]);
      bq[ks] = bf16x8{(bf16)lo.x, (bf16)lo.y, (bf16)lo.z, (bf16)lo.w, (bf16)hi.x, (bf16)hi.y, (bf16)hi.z, (bf16)hi.w};
    }
    // best coarse cosine of each query over the block's rows
    float best = -FLT_MAX;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[u][ks], bq[ks], acc, 0, 0, 0);
      // lane (c, gl): rows r0 + 16 u + 4 gl + i of query c
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (r0 + 16 * u + 4 * gl + i < S) best = fmaxf(best, acc[i]);
    }
    best = fmaxf(best, __shfl_xor(best, 16, 64));
    best = fmaxf(best, __shfl_xor(best, 32, 64));
    if (lane < 16) wbest[w][16 * gr + lane] = best;
  }
  __syncthreads();
  if (threadIdx.x < nq) {
    const int c = threadIdx.x;
    const float bc = fmaxf(fmaxf(wbest[0][c], wbest[1][c]), fmaxf(wbest[2][c], wbest[3][c]));
    // (clamped at 0, which only raises a minimum and so keeps the bound valid)
    mins[(q0 + c) * B5_G + g] = fmaxf(1.f - bc, 0.f);
  }
}

// more than V4_MQ queries: one wave per query merges its minima into thr0
__global__ __launch_bounds__(256) void bound5_merge_kernel(const float* __restrict__ mins, int ng, int64_t Q,
                                                           int k, float* thr0) {
  const int64_t qq = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qq >= Q) return;
  const Mins2 m[1] = {v4_load_mins(mins + qq * B5_G, ng, threadIdx.x & 63)};
  float t[1];
  v4_kth_bounds<1>(m, ng, k, t);
  if ((threadIdx.x & 63) == 0) thr0[qq] = t[0];
}

// Admissions go to a wave-private LDS list whose fill count is wave-uniform
// (ballots + mbcnt, no atomic at all inside the loop: a returning global
// atomic there put its contended round trip in every tile, a returning LDS
// atomic ~100 cycles per admitting check).  At the end the block counts its
// entries per query, reserves each query's range with one global atomic per
// (block, query), and scatters.
constexpr int V4_LIST = 2048;    // admitted (query, row) pairs per block
constexpr int V4_WL = V4_LIST / 4;   // ... per wave
constexpr int V4_PF = 4;        // packed row tiles in flight per wave

// (NQB > 4: at least 3 waves per SIMD -- left alone the compiler unrolled
// its way to 284 registers and one wave per SIMD, 1.7x slower)
template <int KS, int NQB, bool PK>
__global__ __launch_bounds__(256, NQB > 4 ? V4_WPS : 1) void scan4_kernel(const float* __restrict__ tab,
                                                    const float* __restrict__ inv,
                                                    const bf16* __restrict__ tb, int64_t N, int rpb,
                                                    const bf16* __restrict__ qb,
                                                    const float* __restrict__ thr0,
                                                    const float* __restrict__ qn, int64_t Q, int* qcnt,
                                                    int* rows, float* dists,
                                                    const float* __restrict__ bmins, int ng, int k) {
  constexpr int D = KS * 32;
  // up to 4 query blocks the B fragments live in registers; beyond that
  // (64+ KS x 4 VGPRs) in LDS, stored in fragment order -- entry (b, ks,
  // lane) is lane's 16 B, so a wave's ds_read_b128 is one contiguous 1 KB
  // with no bank conflicts.  (Left to itself the compiler re-loaded the
  // register copy from global memory every tile.)
  constexpr bool BL = NQB > 4;
  __shared__ int lq[V4_LIST];     // admitted (query, row) pairs of the block
  __shared__ int lr[V4_LIST];
  __shared__ int qn_[NQB * 16];   // per-query counts, then this block's bases
  __shared__ float thl[NQB * 16]; // (bmins) the block's admission bounds
  __shared__ int wcnt[4];
  __shared__ bf16x8 bqs[BL ? NQB * KS * 64 : 1];
  const int64_t qc0 = (int64_t)blockIdx.y * (NQB * 16);
  const int nq = (int)min<int64_t>(NQB * 16, Q - qc0);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = min(N, r0 + rpb);
  // A fragments of the next PF row tiles in flight per wave (a register
  // ring, static indices): fp32 rows scaled and rounded here, or (PK) the
  // fit-time bf16 copy loaded as is.  The first PF loads go out before the
  // query fragments are staged.
  constexpr int PF = PK && NQB <= 4 ? V4_PF : 2;
  using Frag = typename std::conditional<PK, bf16x8[KS], float4[KS][2]>::type;
  Frag x[PF];
  float iv[PF];
  auto load = [&](int64_t bse, Frag& xx, float& ivv) {
    if (bse < r1) {
      const int64_t r = bse + r16 < r1 ? bse + r16 : r0;
      if constexpr (PK) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xx[ks] = *reinterpret_cast<const bf16x8*>(tb + r * D + ks * 32 + 8 * g);
      } else {
        v4_load_rows<KS>(tab, r, xx, g);
        ivv = inv[r];
      }
    }
  };
  // (bound5 minima to merge: loaded before everything else, so the merge
  // waits for them alone and runs under the row tiles' loads)
  constexpr int MWMAX = NQB * 16 <= V4_MQ ? NQB * 16 / 4 : 1;
  Mins2 mm[MWMAX];
  if constexpr (NQB * 16 <= V4_MQ) if (bmins) {
#pragma unroll
    for (int j = 0; j < MWMAX; ++j) mm[j] = v4_load_mins(bmins + (qc0 + min(w + 4 * j, nq - 1)) * B5_G, ng, lane);
  }
  const int64_t first = r0 + 16 * w;
#pragma unroll
  for (int u = 0; u < PF; ++u) load(first + 64 * u, x[u], iv[u]);
  int wc = 0;   // this wave's list fill (wave-uniform)
  // lane (c = r16, g) of B fragment (b, ks): query 16 b + c's k-chunk
  // [32 ks + 8 g, +8)
  bf16x8 bq[BL ? 1 : NQB][KS];
  float th[NQB];
  // (clamped indices + selects: all of these loads are in flight at once --
  // as guarded loads the compiler issued them one round trip at a time,
  // 16 serial misses in the prologue of every NQB = 16 block)
#pragma unroll
  for (int b = 0; b < NQB; ++b) {
    const int qi = 16 * b + r16;
    const int64_t qs = qc0 + min(qi, nq - 1);
    if constexpr (!BL) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(qb + qs * D + ks * 32 + 8 * g);
        bq[b][ks] = qi < nq ? v : bf16x8{};
      }
    }
    if (!bmins) {
      const float t = thr0[qs];   // (bound5_merge_kernel's)
      // a row passes iff its coarse cosine is >= 1 - bound; the 1e-6 below
      // covers the rounding of 1 - bound (query slots past nq: 2, never)
      th[b] = qi < nq ? (1.f - (t + V4_EPS)) - 1e-6f : 2.f;
    }
  }
  // few queries (V4_MQ: NQB = 2): merge their bound5 minima here, a wave per query
  if constexpr (NQB * 16 <= V4_MQ) if (bmins) {
    auto merge = [&](auto mw_c) {
      constexpr int MW = decltype(mw_c)::value;   // queries per wave
      Mins2 m2[MW];
#pragma unroll
      for (int j = 0; j < MW; ++j) m2[j] = mm[j];
      float tj[MW];
      v4_kth_bounds<MW>(m2, ng, k, tj);
#pragma unroll
      for (int j = 0; j < MW; ++j) {
        const int qq = w + 4 * j;
        if (qq < nq && lane == 0) thl[qq] = tj[j];
      }
    };
    if (nq <= 4) merge(std::integral_constant<int, 1>{});
    else if (nq <= 16) merge(std::integral_constant<int, 4>{});
    else merge(std::integral_constant<int, NQB * 16 / 4>{});
  }
  if constexpr (BL) {
    constexpr int PER = NQB * KS * 64 / 256;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = threadIdx.x + 256 * j;
      const int l = e & 63, ks = (e >> 6) % KS, b = (e >> 6) / KS;
      const int qi = 16 * b + (l & 15);
      const bf16x8 v = *reinterpret_cast<const bf16x8*>(qb + (qc0 + min(qi, nq - 1)) * D + ks * 32 + 8 * (l >> 4));
      bqs[e] = qi < nq ? v : bf16x8{};
    }
  }
  for (int i = threadIdx.x; i < NQB * 16; i += 256) qn_[i] = 0;
  __syncthreads();
  if constexpr (NQB * 16 <= V4_MQ) if (bmins) {
#pragma unroll
    for (int b = 0; b < NQB; ++b) {
      const int qi = 16 * b + r16;
      th[b] = qi < nq ? (1.f - (thl[qi] + V4_EPS)) - 1e-6f : 2.f;
    }
  }
  for (int64_t b0 = first; b0 < r1; b0 += 64 * PF) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int64_t base = b0 + 64 * u;
      if (base >= r1) break;
      bf16x8 a[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if constexpr (PK) {
          a[ks] = x[u][ks];
        } else {
          const float4 p = x[u][ks][0], v = x[u][ks][1];
          const float s = iv[u];
          a[ks] = bf16x8{(bf16)(p.x * s), (bf16)(p.y * s), (bf16)(p.z * s), (bf16)(p.w * s),
                         (bf16)(v.x * s), (bf16)(v.y * s), (bf16)(v.z * s), (bf16)(v.w * s)};
        }
      }
      load(base + 64 * PF, x[u], iv[u]);
      // every query block's MFMAs first, back to back (interleaving each
      // block's admission checks serialised LDS read -> MFMA -> result ->
      // ballot per block: 146 us for 256 queries), then one ballot per block
      // on the best of its 4 rows -- usually empty -- before the per-row
      // ones.  A check compares the coarse cosine with 1 - (bound + V4_EPS):
      // with |coarse - exact| <= 2^-7 + 2^-16 (2^-8 per bf16 factor) + fp32
      // accumulation error (< 2e-5 here) < V4_EPS = 0.0079 the admitted set
      // contains every row whose exact distance is <= the bound.
      // (LDS fragments: block b + 1's read is issued before block b's MFMAs)
      f32x4 acc[NQB];
      bf16x8 nb[KS];
      if constexpr (BL) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) nb[ks] = bqs[ks * 64 + lane];
      }
#pragma unroll
      for (int b = 0; b < NQB; ++b) {
        bf16x8 cb[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cb[ks] = BL ? nb[ks] : bq[BL ? 0 : b][ks];
        if constexpr (BL) {
          if (b + 1 < NQB) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) nb[ks] = bqs[((b + 1) * KS + ks) * 64 + lane];
          }
        }
        acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], cb[ks], acc[b], 0, 0, 0);
      }
      const bool full = base + 16 <= r1;   // (wave-uniform) no row of the tile past r1
      const int rb = (int)base + 4 * g;
#pragma unroll
      for (int b = 0; b < NQB; ++b) {
        // lane (c = r16, g): rows rb + i, query 16 b + c
        const float mx = fmaxf(fmaxf(acc[b][0], acc[b][1]), fmaxf(acc[b][2], acc[b][3]));
        if (!__ballot(mx >= th[b])) continue;
        // one block adds at most 256 entries: room is checked once here (a
        // full list reads as overflowed, and the batch takes the exact path)
        if (wc > V4_WL - 256) { wc = V4_WL + 1; continue; }
        int* lqw = lq + w * V4_WL;
        int* lrw = lr + w * V4_WL;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool pass = acc[b][i] >= th[b] && (full || rb + i < r1);
          const uint64_t m = __ballot(pass);
          if (pass) {
            const int p = wc + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            lqw[p] = 16 * b + r16;
            lrw[p] = rb + i;
          }
          wc += __popcll(m);
        }
      }
    }
  }
  if (lane == 0) wcnt[w] = wc;
  __syncthreads();
  const int c0 = wcnt[0], c1 = wcnt[1], c2 = wcnt[2], c3 = wcnt[3];
  if (max(max(c0, c1), max(c2, c3)) > V4_WL) {   // a wave's list overflowed: every query
    for (int q = threadIdx.x; q < nq; q += 256)     // of the block takes the exact path
      atomicOr(&qcnt[qc0 + q], V4_OVF);
    if (threadIdx.x == 0) qcnt[Q] = 1;              // the call's overflow word
    return;
  }
  // entry j of the block (waves' lists back to back) -> its LDS slot
  const int s1 = c0, s2 = c0 + c1, s3 = c0 + c1 + c2, n = s3 + c3;
  auto slot = [&](int j) {
    return j < s1 ? j : j < s2 ? V4_WL + j - s1 : j < s3 ? 2 * V4_WL + j - s2 : 3 * V4_WL + j - s3;
  };
  for (int e = threadIdx.x; e < n; e += 256) atomicAdd(&qn_[lq[slot(e)]], 1);
  __syncthreads();
  for (int q = threadIdx.x; q < nq; q += 256) {
    const int c = qn_[q];
    qn_[q] = c ? atomicAdd(&qcnt[qc0 + q], c) : 0;   // this block's range of query q's list
    if (c && qn_[q] + c > V4_CAP) qcnt[Q] = 1;       // the list overflowed: the call's overflow word
  }
  __syncthreads();
  // exact fp32 distance of every admitted pair, here rather than in the
  // per-query rescore: the row gathers then overlap the other blocks'
  // streaming instead of forming a one-block-per-query latency chain.  One
  // lane per pair, the float4 chunks summed in order: scan v2's arithmetic,
  // expression for expression, so v2 and v4 give a row the same distance
  // bit for bit (a row-sharded index, whose small shards may take v2, then
  // returns the single index's answer).
  constexpr int DV = KS * 8;
  const float4* tab4 = reinterpret_cast<const float4*>(tab);
  const float4* qn4 = reinterpret_cast<const float4*>(qn);
  for (int e = threadIdx.x; e < n; e += 256) {
    const int sl = slot(e);
    const int qe = lq[sl], re = lr[sl];
    const float4* rp = tab4 + (int64_t)re * DV;
    const float4* qp = qn4 + (qc0 + qe) * DV;
    float4 x[DV];
#pragma unroll
    for (int v = 0; v < DV; ++v) x[v] = rp[v];
    const float ir = inv[re];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const float4 q = qp[v];
      s += dot4(x[v], q);
    }
    const float dist = cos_dist(s, ir);
    const int pos = atomicAdd(&qn_[qe], 1);
    if (pos < V4_CAP) {   // (past it the query's count exceeds V4_CAP: exact path)
      const int64_t o = (qc0 + qe) * V4_CAP + pos;
      rows[o] = re;
      dists[o] = dist;
    }
  }
}


// Exact top-k of one query over the whole table inside one B4_T-thread block:
// scan v2's per-wave lists (rows in increasing order per wave, admitted while
// strictly under the wave's k-th best, compacted by a register bitonic sort)
// and its distance arithmetic expression for expression, then wave 0 merges
// the waves' sorted k-lists.  The same (distance, row) order as every other
// scan, so a query that lands here returns what scan v2 returns.  Needs
// k <= 32 (two k-lists per 64-lane merge step) and 16 * 64 * 8 B of LDS.
template <int DV>
__device__ void exact_query_topk(const float* __restrict__ tab, const float* __restrict__ inv, int64_t lo,
                                 int64_t N, const float* __restrict__ qrow, int k, float* lds, int64_t* idx,
                                 float* dist) {
  constexpr int NW = B4_T / 64;
  __shared__ int cntl[NW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float* lcd = lds + w * 64;
  int* lci = reinterpret_cast<int*>(lds + NW * 64) + w * 64;
  // wave-uniform addresses: the query comes in through scalar loads
  const float4* qv = reinterpret_cast<const float4*>(qrow);
  int c = 0;
  float th = FLT_MAX;
  for (int64_t base = lo + 64 * w; base < N; base += 64 * NW) {   // rows [lo, N)
    const int64_t r = base + lane;
    const bool ok = r < N;
    const int64_t rc = ok ? r : 0;
    float4 x[DV];
    load_row<DV>(tab, rc, x);
    const float dd = exact_dist<DV>(x, qv, inv[rc]);
    wave_admit(lcd, lci, c, th, k, lane, ok, dd, r);
  }
  c = wave_compact(lcd, lci, c, k, lane, &th);
  if (lane == 0) cntl[w] = c;
  __syncthreads();
  if (w == 0) {
    float d;
    int i;
    wave_merge_lists<NW>(lds, reinterpret_cast<const int*>(lds + NW * 64), cntl, 64, 1, k, lane, d, i);
    if (lane < k) {
      idx[lane] = (int64_t)i;
      dist[lane] = d;
    }
  }
}

// The batched exact fallback (Q > V4_FQ): work item (group h of V4_BQ
// queries, row chunk f) scans rows [lo, hi) once for every overflowed query
// of the group -- each wave holds a row in registers and scores it against
// each of them (exact_dist: the single-query scan's bits), one k-list per
// (query, wave) -- then the block's waves merge query qi's wave lists into
// the item's k-list for that query.  The table is read once per group
// of V4_BQ queries instead of once per query.
constexpr int V4_BQ = 8;      // queries per batch work item
template <int DV, int BT>
__device__ void exact_batch_item(const float* __restrict__ tab, const float* __restrict__ inv, int64_t lo,
                                 int64_t hi, const float* __restrict__ qg, unsigned act, int k,
                                 float* bcd, int* bci, int* bcnt, float* bq, float* pd, int64_t* pi,
                                 int64_t lstride) {
  constexpr int NW = BT / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // the group's queries, interleaved by pairs: chunk v of pair pr at
  // bq[(pr DV + v) 8 ..] = q0.x q1.x q0.y q1.y q0.z q1.z q0.w q1.w
  for (int e = threadIdx.x; e < V4_BQ * DV * 4; e += BT) {
    const int pr = e / (DV * 8), r = e % (DV * 8), v = r / 8, c = (r % 8) / 2, o = r % 2;
    bq[e] = qg[(2 * pr + o) * DV * 4 + v * 4 + c];
  }
  __syncthreads();
  // query qi's list count and k-th best live in lane qi (two VGPRs, not
  // 2 x V4_BQ scalars: the kernel's SGPRs are already full)
  int cv = 0;
  float thv = FLT_MAX;
  for (int64_t base = lo + 64 * w; base < hi; base += 64 * NW) {
    const int64_t r = base + lane;
    const bool ok = r < hi;
    const int64_t rc = ok ? r : lo;
    const float4* rp = reinterpret_cast<const float4*>(tab + rc * DV * 4);
    const float ir = ((const __attribute__((address_space(1))) float*)inv)[rc];
    // the V4_BQ distances, float4 chunk by chunk (each query's sum in
    // exact_dist's order: dot4 per chunk, in order; two queries per packed
    // op); the queries come from the LDS copy (uniform-address reads into
    // VGPRs: as scalar loads the compiler hoists them into 4 DV V4_BQ SGPRs
    // and spills)
    float sq[V4_BQ];
#pragma unroll
    for (int qi = 0; qi < V4_BQ; ++qi) sq[qi] = 0.f;
    // the whole row first: its DV loads in flight together (global address
    // space: a flat load would also count against the LDS reads' waits)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) f32x4v gf32x4;
    float4 x[DV];
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const f32x4v t = ((gf32x4*)rp)[v];
      x[v] = make_float4(t.x, t.y, t.z, t.w);
    }
    const float4* bq4 = reinterpret_cast<const float4*>(bq);
#pragma unroll
    for (int v = 0; v < DV; ++v) {
      const float4 xv = x[v];
#pragma unroll
      for (int pr = 0; pr < V4_BQ / 2; ++pr) {
        const f32x2 p = dot4_q2(xv, bq4[(pr * DV + v) * 2], bq4[(pr * DV + v) * 2 + 1]);
        sq[2 * pr] += p.x;
        sq[2 * pr + 1] += p.y;
      }
    }
#pragma unroll
    for (int qi = 0; qi < V4_BQ; ++qi) sq[qi] = cos_dist(sq[qi], ir);
#pragma unroll 1
    for (int qi = 0; qi < V4_BQ; ++qi) {
      if (!((act >> qi) & 1u)) continue;   // (uniform)
      float dd = sq[0];
#pragma unroll
      for (int j = 1; j < V4_BQ; ++j) dd = qi == j ? sq[j] : dd;
      int c = __builtin_amdgcn_readlane(cv, qi);
      float th = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thv), qi));
      wave_admit(bcd + (qi * NW + w) * 64, bci + (qi * NW + w) * 64, c, th, k, lane, ok, dd, r);
      cv = lane == qi ? c : cv;
      thv = lane == qi ? th : thv;
    }
  }
#pragma unroll
  for (int qi = 0; qi < V4_BQ; ++qi) {
    if (!((act >> qi) & 1u)) continue;
    float th = 0.f;
    const int cc = wave_compact(bcd + (qi * NW + w) * 64, bci + (qi * NW + w) * 64,
                                __builtin_amdgcn_readlane(cv, qi), k, lane, &th);
    if (lane == 0) bcnt[qi * NW + w] = cc;
  }
  __syncthreads();
  for (int qi = w; qi < V4_BQ; qi += NW) {
    if (!((act >> qi) & 1u)) continue;
    float d;
    int i;
    wave_merge_lists<NW>(bcd + qi * NW * 64, bci + qi * NW * 64, bcnt + qi * NW, 64, 1, k, lane, d, i);
    if (lane < k) {
      pd[qi * lstride + lane] = d;
      pi[qi * lstride + lane] = (int64_t)i;
    }
  }
}

// The batched fallback's work pool (Q > V4_FQ).  scan4 raises the call's
// overflow word (qcnt[Q]) when any query's list overflows; then every
// rescore block, its own query done, pulls work items from a queue word
// (qcnt[2Q + 1]) until they run out.  Item it = (row chunk it / H, group
// it % H): consecutive items share a chunk, so blocks pulling together read
// the same rows.  An item scans its chunk for the group's overflowed queries
// (exact_batch_item); the last of a group's FB items merges each overflowed
// query's FB k-lists.  Not inlined, so the per-query path keeps its
// registers (inlined, the kernel spilled SGPRs).  A call with nothing
// overflowed never enters it: no extra blocks, one extra word read per block.
template <int DV>
__device__ __attribute__((noinline)) void batch_fallback_pool(
    const int* qcnt, int* heads, int k, int64_t* idx, float* dist, const float* __restrict__ tab,
    const float* __restrict__ inv, int64_t N, const float* __restrict__ qn, int64_t Q, int FB, float* pd,
    int64_t* pi, int* pcnt, float* bcd, int* bci, int* bcnt, float* bq, int* slot) {
  constexpr int NW = B4_T / 64;
  const int64_t H = (Q + V4_BQ - 1) / V4_BQ;
  // queue g = blockIdx % 8 holds the chunks f = g (mod 8): blocks sharing an
  // XCD share its queue, so a chunk (<= ~2 MB) is read from HBM once and its
  // groups' items hit that XCD's L2 (speed only: every queue has blocks
  // -- Q > 16 -- and every block joins when the overflow word is up)
  const int g = (int)(blockIdx.x % 8);
  const int64_t items = H * (FB / 8);
  for (;;) {
    __syncthreads();   // (the LDS lists and the slot word are reused)
    if (threadIdx.x == 0) *slot = atomicAdd(heads + g, 1);
    __syncthreads();
    const int64_t it = *slot;
    if (it >= items) return;
    const int fb = g + 8 * (int)(it / H);
    const int64_t h = it % H, q0 = h * V4_BQ;
    unsigned act = 0;
    for (int qi = 0; qi < V4_BQ && q0 + qi < Q; ++qi) {
      const int n = qcnt[q0 + qi];
      if (n > V4_CAP || n < k) act |= 1u << qi;
    }
    if (!act) continue;
    const int64_t lo = N * fb / FB, hi = N * (fb + 1) / FB;
    exact_batch_item<DV, B4_T>(tab, inv, lo, hi, qn + q0 * DV * 4, act, k, bcd, bci, bcnt, bq,
                               pd + (q0 * FB + fb) * k, pi + (q0 * FB + fb) * k, (int64_t)FB * k);
    if (last_arriver(pcnt + h, FB, slot)) {
      // the group's last item: its waves merge the overflowed queries' FB k-lists
      const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
      for (int qi = w; qi < V4_BQ; qi += NW) {
        if (!((act >> qi) & 1u)) continue;
        const int64_t qq = q0 + qi;
        const Cand c = wave_merge_global_lists(pd, pi, qq * FB, FB, k, lane);
        if (lane < k) {
          idx[qq * k + lane] = (int64_t)c.i;
          dist[qq * k + lane] = c.d;
        }
      }
    }
  }
}

// One block per query: the exact distances of its admitted rows (computed
// by scan4's epilogue), the k-th smallest by block_select_kth, then a bitonic
// sort of the rows at or under the selected bin by (distance, row).  A query
// whose list overflowed takes exact_query_topk (DV = d / 4) -- with few
// queries (F > 1: blocks q + Q f, f = 1 .. F-1, that return at once unless
// q's list overflowed) split over F blocks, each scanning 1/F of the table
// into a k-list, the last-arriving one merging them: the all-overflow call
// (a table with thousands of duplicates per query) no longer puts the whole
// table through one CU (the merge keeps the (distance,
// row) order, so the answer is the single block's bit for bit).
constexpr int V4_FMAX = 64;        // fallback blocks per query
constexpr int V4_FQ = 16;          // queries up to which the fallback is split
inline int v4_fallback_split(int64_t Q) {
  return Q <= V4_FQ ? (int)std::min<int64_t>(V4_FMAX, 256 / Q) : 1;
}
// Q > V4_FQ: row chunks of the batched fallback (about V4_BI work items,
// 8..128 chunks, a multiple of 8); 0: none.  Few large items: all-overflow
// Q = 256 over 1M x 64 took 1.27 / 1.34 / 1.57 / 1.93 / 2.67 ms at 256 / 512 /
// 1024 / 2048 / 4096 items (profiles/lab/r06_knn_batch_lab.txt).  The
// k-lists: Q x chunks x 32 x 12 B, ~12 MB at most.
constexpr int V4_BI = 256;
inline int v4_batch_chunks(int64_t Q) {
  if (Q <= V4_FQ) return 0;
  const int64_t H = (Q + V4_BQ - 1) / V4_BQ;
  return (int)std::max<int64_t>(8, std::min<int64_t>(128, (V4_BI / H) / 8 * 8));
}
// k-lists per query of either fallback form
inline int v4_lists(int64_t Q) {
  const int F = v4_fallback_split(Q);
  return F > 1 ? F : v4_batch_chunks(Q);
}
template <int DV>
__global__ __launch_bounds__(B4_T) void rescore_kernel(const float* __restrict__ dists, const int* qcnt,
                                                       const int* rows, int k, int64_t* idx,
                                                       float* dist, const float* __restrict__ tab,
                                                       const float* __restrict__ inv, int64_t N,
                                                       const float* __restrict__ qn, int64_t Q, int F,
                                                       int FB, float* pd, int64_t* pi, int* pcnt) {
  // one LDS image: dl / cd / ci of the per-query path, or the batched
  // fallback's (query, wave) lists (FB > 0: blocks from Q on, which answer
  // the overflowed queries)
  constexpr int NW = B4_T / 64;
  constexpr int BL = V4_BQ * NW * 64;
  constexpr int SMW = 3 * V4_CAP > 2 * BL ? 3 * V4_CAP : 2 * BL;
  __shared__ float smem[SMW];
  __shared__ int bcnt[V4_BQ * NW];
  __shared__ float bq[V4_BQ * 64];   // the batched fallback's queries (d <= 64)
  float* dl = smem;
  float* cd = smem + V4_CAP;   // the rows at or under the k-th's bin: all of the list at most
  int* ci = reinterpret_cast<int*>(smem + 2 * V4_CAP);
  __shared__ int cnt;
  __shared__ int last;
  static_assert(V4_CAP >= 2 * B4_T, "exact fallback lists live in dl");
  // FB > 0: the batched fallback's pool, entered after this block's own
  // query when scan4 raised the overflow word (or this query overflowed)
  const bool pool = FB > 0 && qcnt[Q] != 0;
  auto join_pool = [&]() {
    batch_fallback_pool<DV>(qcnt, const_cast<int*>(qcnt) + 2 * Q + 2, k, idx, dist, tab, inv, N, qn, Q, FB, pd,
                            pi, pcnt, smem, reinterpret_cast<int*>(smem + BL), bcnt, bq, &last);
  };
  const int64_t qq = blockIdx.x % Q;
  const int f = (int)(blockIdx.x / Q);
  auto fail = [&]() {
    __syncthreads();   // (dl is reused)
    exact_query_topk<DV>(tab, inv, 0, N, qn + qq * DV * 4, k, dl, idx + qq * k, dist + qq * k);
  };
  // the split fallback: rows [N f / F, N (f+1) / F) -> k-list f of the query,
  // then the last of its F blocks merges the F lists (wave 0)
  auto split = [&]() {
    __syncthreads();
    const int64_t lo = N * f / F, hi = N * (f + 1) / F;
    float* pdq = pd + (qq * F + f) * k;
    int64_t* piq = pi + (qq * F + f) * k;
    exact_query_topk<DV>(tab, inv, lo, hi, qn + qq * DV * 4, k, dl, piq, pdq);
    if (!last_arriver(pcnt + qq, F, &last)) return;
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      const Cand c = wave_merge_global_lists(pd, pi, qq * F, F, k, lane);
      if (lane < k) {
        idx[qq * k + lane] = (int64_t)c.i;
        dist[qq * k + lane] = c.d;
      }
    }
  };
  if (f > 0) {   // a split-fallback block: only for an overflowed list
    const int n = qcnt[qq];
    if (n > V4_CAP || n < k) split();
    return;
  }
  const int* rl = rows + qq * V4_CAP;
  const float* dq = dists + qq * V4_CAP;
  // the list's first B4_T entries are read beside its count (the slots
  // exist whatever the count; the ones past it are ignored): one round trip
  const float d0 = dq[threadIdx.x];
  const int i0 = rl[threadIdx.x];
  const int n = qcnt[qq];
  if (n > V4_CAP || n < k) {   // overflow (fewer than k admitted rows only when N < k)
    if (F > 1) split();
    else if (FB == 0) fail();
    else join_pool();   // (the pool answers it)
    return;
  }
  if (threadIdx.x == 0) cnt = 0;
  if ((int)threadIdx.x < n) dl[threadIdx.x] = d0;
  for (int e = threadIdx.x + B4_T; e < n; e += B4_T) dl[e] = dq[e];
  __syncthreads();
  const unsigned tk = block_select_kth<B4_T>(dl, n, k);   // upper edge of the k-th's bin
  for (int e = threadIdx.x; e < n; e += B4_T)
    if (__float_as_uint(dl[e]) <= tk) {
      const int pos = atomicAdd(&cnt, 1);
      cd[pos] = dl[e];
      ci[pos] = e < B4_T ? i0 : rl[e];
    }
  __syncthreads();
  // (many rows sharing the k-th's bin -- duplicates -- are sorted here too,
  // up to the whole list: round 5 sent a bin of more than 256 rows to the
  // exact table scan, 9.9 ms for 256 such queries over 1M rows)
  const int nv = cnt;
  if (nv <= 64) {   // (the usual case) one wave's register sort, no more barriers
    if (threadIdx.x < 64) {
      const int lane = threadIdx.x;
      float d = lane < nv ? cd[lane] : FLT_MAX;
      int i = lane < nv ? ci[lane] : INT_MAX;
      wave_sort64(d, i, lane);
      if (lane < k) {
        idx[qq * k + lane] = (int64_t)i;
        dist[qq * k + lane] = d;
      }
    }
    if (pool) join_pool();
    return;
  }
  sort_emit<B4_T>(cd, ci, nv, k, idx + qq * k, dist + qq * k);
  if (pool) join_pool();
}

// Per query: the k best of nslices k-lists.  All of a chunk's candidates are
// loaded up front (MT per thread, one round trip), then filtered against the
// running k-th best and compacted in LDS.
constexpr int MT = 16;
constexpr int FT = 24;   // fast path: candidates loaded per thread per round
// (the block's work: one query's lists c [nl][k] -> idx / dist [k]; shared by
// merge_kernel and the set-scoped search's merge, whose output rows are strided)
__device__ __forceinline__ void merge_block(const Cand* c, int nl, int k, int64_t* idx, float* dist) {
  __shared__ float cd[CAP];
  __shared__ int ci[CAP];
  __shared__ int cnt;
  __shared__ float thr;
  const int total = nl * k;
  // fast path 0 (one load round, up to 4 lists per thread): the k-th smallest
  // of the lists' minima bounds the k-th best overall (k lists each hold a
  // candidate at or under it), so only the candidates at or under that bound
  // -- radix_select_kth over the nl minima, which fails with fewer than k
  // lists -- are sorted.  Same result as sorting them all: every candidate of
  // the k best passes.
  if (total <= NT * FT && nl <= 4 * NT) {
    Cand e[FT];
#pragma unroll
    for (int j = 0; j < FT; ++j) {
      const int t = j * NT + threadIdx.x;
      e[j] = t < total ? c[t] : Cand{FLT_MAX, INT_MAX};
    }
    // distances are >= 0: their bits order like the values
    auto key = [](float x) { return __float_as_uint(fmaxf(x, 0.f)); };
    unsigned mk[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int l = threadIdx.x + r * NT;
      float m = FLT_MAX;
      if (l < nl)
        for (int j = 0; j < k; ++j) m = fminf(m, c[(int64_t)l * k + j].d);
      mk[r] = l < nl ? key(m) : 0xffffffffu;
    }
    if (threadIdx.x == 0) cnt = 0;   // (the select's barriers order it before the appends)
    const unsigned tk = radix_select_kth(k, nl, [&](unsigned* hist, unsigned mask, unsigned prefix, int sh) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (mk[r] != 0xffffffffu && (mk[r] & mask) == prefix) atomicAdd(&hist[(mk[r] >> sh) & 255u], 1u);
    });
    if (tk != 0xffffffffu) {
      constexpr int SCAP = 128;
#pragma unroll
      for (int j = 0; j < FT; ++j)
        if (e[j].i != INT_MAX && key(e[j].d) <= tk) {
          const int pos = atomicAdd(&cnt, 1);
          if (pos < SCAP) { cd[pos] = e[j].d; ci[pos] = e[j].i; }
        }
      __syncthreads();
      const int nv = cnt;
      if (nv <= SCAP) {
        sort_emit<NT>(cd, ci, nv, k, idx, dist);
        return;
      }
    }
    __syncthreads();
  }
  // fast path: the valid candidates (with admission bounds, a few per query)
  // fit the buffer -> one gather and one sort
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int base = 0; base < total; base += NT * FT) {
    Cand e[FT];   // all loads of a round in flight together
#pragma unroll
    for (int j = 0; j < FT; ++j) {
      const int t = base + j * NT + threadIdx.x;
      e[j] = t < total ? c[t] : Cand{FLT_MAX, INT_MAX};
    }
#pragma unroll
    for (int j = 0; j < FT; ++j)
      if (e[j].i != INT_MAX) {
        const int pos = atomicAdd(&cnt, 1);
        if (pos < CAP) { cd[pos] = e[j].d; ci[pos] = e[j].i; }
      }
  }
  __syncthreads();
  const int nv = cnt;
  if (nv <= CAP) {
    sort_emit<NT>(cd, ci, nv, k, idx, dist);
    return;
  }
  __syncthreads();
  if (threadIdx.x == 0) { cnt = 0; thr = FLT_MAX; }
  __syncthreads();
  for (int base = 0; base < total; base += NT * MT) {
    Cand e[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      const int t = base + j * NT + threadIdx.x;
      e[j] = t < total ? c[t] : Cand{FLT_MAX, INT_MAX};
    }
#pragma unroll
    for (int j = 0; j < MT; ++j) {
      if (e[j].i != INT_MAX && e[j].d <= thr) {
        int pos = atomicAdd(&cnt, 1);
        cd[pos] = e[j].d;
        ci[pos] = e[j].i;
      }
      __syncthreads();
      if (cnt > CAP - NT) compact(cd, ci, &cnt, &thr, k);
    }
  }
  compact(cd, ci, &cnt, &thr, k);
  for (int t = threadIdx.x; t < k; t += NT) {
    const bool ok = t < cnt;
    idx[t] = ok ? (int64_t)ci[t] : -1;
    dist[t] = ok ? cd[t] : FLT_MAX;
  }
}

__global__ __launch_bounds__(NT) void merge_kernel(const Cand* in, int nl, int k, int64_t* idx,
                                                   float* dist) {
  const int64_t qq = blockIdx.x;
  merge_block(in + qq * (int64_t)nl * k, nl, k, idx + qq * k, dist + qq * k);
}

// Per query: the k best of `lists` k-lists [lists][Q][k] (dist, int64 row),
// ascending by (dist, row as unsigned); padding entries (FLT_MAX, -1) sort
// last.  One block per query, all lists*k <= TM_CAP candidates sorted in LDS.
constexpr int TM_CAP = 2048;
__global__ __launch_bounds__(NT) void topk_merge_kernel(const float* dist, const int64_t* idx,
                                                        int lists, int64_t Q, int k,
                                                        int64_t* out_idx, float* out_dist) {
  __shared__ float cd[TM_CAP];
  __shared__ uint64_t ci[TM_CAP];
  const int64_t qq = blockIdx.x;
  const int n = lists * k;
  int n2 = 2;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += NT) {
    if (t < n) {
      const int64_t src = ((int64_t)(t / k) * Q + qq) * k + t % k;
      cd[t] = dist[src];
      ci[t] = (uint64_t)idx[src];
    } else {
      cd[t] = FLT_MAX;
      ci[t] = ~0ull;
    }
  }
  __syncthreads();
  bitonic<NT>(cd, ci, n2, [](float da, uint64_t ia, float db, uint64_t ib) {
    return da < db || (da == db && ia < ib);
  });
  for (int t = threadIdx.x; t < k; t += NT) {
    out_idx[qq * k + t] = (int64_t)ci[t];
    out_dist[qq * k + t] = cd[t];
  }
}

__global__ void inv_norm_kernel(const float* t, int64_t N, int d, float* out) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
  for (int64_t r = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); r < N; r += nw) {
    float s = 0.f;
    for (int i = lane; i < d; i += 64) { float v = t[r * d + i]; s += v * v; }
    s = wave_sum(s);
    if (lane == 0) out[r] = s > 0.f ? 1.f / sqrtf(s) : 1.f;
  }
}

void plan(int64_t N, int64_t Q, int* nslices, int64_t* rows_per_slice) {
  int64_t qtiles = cdiv(Q, QT);
  int64_t want = std::max<int64_t>(1, 2048 / qtiles);
  int64_t ns = std::min<int64_t>(want, std::max<int64_t>(1, cdiv(N, 2048)));
  *rows_per_slice = cdiv(N, ns);
  *nslices = (int)cdiv(N, *rows_per_slice);
}

// The fit-time bf16 copy read by scan v4: out[r][c] = bf16(t[r][c] * inv[r])
// (fp32 product, round to nearest even -- the rounding scan v4 otherwise
// applies to the fp32 rows on the fly).  8 elements per thread, d % 8 == 0.
__global__ void pack_rows_kernel(const float* __restrict__ t, const float* __restrict__ inv, int64_t N, int d,
                                 bf16* __restrict__ out) {
  const int64_t n8 = N * d / 8;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n8; e += (int64_t)gridDim.x * blockDim.x) {
    const float iv = inv[e * 8 / d];
    const float4 u = reinterpret_cast<const float4*>(t)[2 * e], v = reinterpret_cast<const float4*>(t)[2 * e + 1];
    reinterpret_cast<bf16x8*>(out)[e] = bf16x8{(bf16)(u.x * iv), (bf16)(u.y * iv), (bf16)(u.z * iv), (bf16)(u.w * iv),
                                               (bf16)(v.x * iv), (bf16)(v.y * iv), (bf16)(v.z * iv), (bf16)(v.w * iv)};
  }
}

}  // namespace

bool use_v2(int d, int k) { return d % 4 == 0 && d >= 4 && d <= 64 && k <= K2_KMAX; }

// v2 plan: up to 512 row slices (2 blocks per CU per query tile), slices a
// multiple of 64 rows
void plan2(int64_t N, int* nslices, int64_t* rows_per_block) {
  const int64_t want = std::min<int64_t>(512, std::max<int64_t>(1, cdiv(N, 256)));
  *rows_per_block = rup(cdiv(N, want), 64);
  *nslices = (int)cdiv(N, *rows_per_block);
}

bool use_v4(int64_t N, int64_t Q, int d, int k) {
  // Any table size: one of at most V4_S rows is its own sample (pass 1 is
  // then the whole search).  A single query over fewer than V4_Q1_N rows takes scan
  // v2, whose one pass beats v4's fixed chain (29 vs 50 us at 20000 rows, 65
  // vs 61 at 1M); v4's exact distances use v2's arithmetic, so the choice
  // never changes an answer.
  return use_v2(d, k) && Q >= 1 && d % 32 == 0 && (Q > 1 || N >= V4_Q1_N);
}

// The scratch of one search, carved once (null base: `total` is the size).
// Scan v1: the per-slice k-lists.  v2 / v3: cands | qn [Q][d] | thr0 [Q].
// v4 after those: bf16 queries [Q][d] | qcnt: [Q] list counts, the overflow
// word, [Q] fallback arrival counters, a spare word, the batched fallback's
// 8 queue heads | admitted rows [Q][V4_CAP] | their exact distances | the
// bound's block minima [Q][B5_G] | the fallbacks' k-lists (k <= 32)
struct TopkWs {
  int ns; int64_t rps;   // the scan's row slices
  Cand* cands;
  float *qn, *thr0;
  bf16* qb; int* qcnt; int* rows; float* dists; float* bmins; float* split_d; int64_t* split_i;
  size_t total;
};
TopkWs carve_topk(void* ws, int64_t N, int64_t Q, int k, int d) {
  TopkWs w{};
  Bump b(ws);
  const bool v2 = use_v2(d, k);
  if (v2) plan2(N, &w.ns, &w.rps);
  else plan(N, Q, &w.ns, &w.rps);
  w.cands = (Cand*)b.take((size_t)Q * w.ns * k * sizeof(Cand));
  w.total = b.off;
  if (!v2) return w;
  w.qn = (float*)b.take((size_t)Q * d * 4);
  w.thr0 = (float*)b.take((size_t)Q * 4, 4);   // (right behind qn)
  w.total = b.off;
  if (!use_v4(N, Q, d, k)) return w;
  const size_t lists = (size_t)Q * v4_lists(Q) * 32;   // (v4_lists >= 8 for every Q >= 1)
  w.qb = (bf16*)b.take((size_t)Q * d * 2);
  w.qcnt = (int*)b.take((size_t)Q * 8 + 48);
  w.rows = (int*)b.take((size_t)Q * V4_CAP * 4);
  w.dists = (float*)b.take((size_t)Q * V4_CAP * 4);
  w.bmins = (float*)b.take((size_t)Q * B5_G * 4);
  w.split_d = (float*)b.take(lists * 4);
  w.split_i = (int64_t*)b.take(lists * 8);
  w.total = b.off + 256;
  return w;
}

// Final merge of the per-block k-lists, one block per query.  Measured at
// 1M rows (512 lists, 5632 candidates per query): this filter-and-compact
// block 32 us; a two-stage (16 groups, then the group lists) 32 + 16 us; a
// one-shot 8192-entry bitonic sort by 1024 threads 107 us; a per-wave register
// merge 50 us -- the block barriers of a one-block kernel dominate all of them.
dcnr_status merge_lists(const Cand* cands, int64_t Q, int ns, int k, int64_t* idx, float* dist,
                        hipStream_t s) {
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)Q), dim3(NT), 0, s, cands, ns, k, idx, dist);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

// The kernels' compile-time shapes, each chosen in one place: f is called
// with the shape as std::integral_constant arguments.
template <int V> using ic = std::integral_constant<int, V>;
// d / 4 in [1, 16] (scan v2's widths)
template <int DV = 1, class F>
void with_dv(int dv, F f) {
  if (dv == DV) f(ic<DV>{});
  else if constexpr (DV < 16) with_dv<DV + 1>(dv, f);
}
// scan v4: KS = d / 32 (1 or 2), and whether the fit-time bf16 copy is read
template <class F>
void with_v4_rows(int d, bool packed, F f) {
  if (d == 32) packed ? f(ic<1>{}, std::true_type{}) : f(ic<1>{}, std::false_type{});
  else packed ? f(ic<2>{}, std::true_type{}) : f(ic<2>{}, std::false_type{});
}
// ... and the 16-query blocks per scan4 block (2, 4, 8 or 16)
template <class F>
void with_v4_nqb(int nqb, F f) {
  nqb == 2 ? f(ic<2>{}) : nqb == 4 ? f(ic<4>{}) : nqb == 8 ? f(ic<8>{}) : f(ic<16>{});
}

// enough for every d (the v2 path keeps Q x d <= Q x 64 normalised queries;
// wider rows take scan v1)
static size_t topk_ws(int64_t N, int64_t Q, int k) {
  return std::max(carve_topk(nullptr, N, Q, k, 64).total, carve_topk(nullptr, N, Q, k, 256).total);
}

static dcnr_status cosine_topk(const float* t, const float* inv, const bf16* tb, int64_t N, int d,
                               const float* q, int64_t Q, int k, int64_t* idx, float* dist, void* ws,
                               size_t ws_bytes, hipStream_t s, bool allow_v3 = true) {
  if (k < 1 || k > KMAX || d < 4 || d % 4 || d > 256 || N < 1) {
    set_error("cosine_topk: unsupported k=%d d=%d N=%lld (1<=k<=64, d%%4==0, d<=256)", k, d,
              (long long)N);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (Q <= 0) return DCNR_OK;
  const TopkWs w = carve_topk(ws, N, Q, k, d);
  if (ws_bytes < w.total) {
    set_error("cosine_topk: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  if (!use_v2(d, k)) {   // scan v1
    const dim3 grid(w.ns, (unsigned)cdiv(Q, QT));
    if (d <= 64)
      hipLaunchKernelGGL(scan_kernel<16>, grid, dim3(NT), 0, s, t, inv, N, d, q, Q, k, w.rps, w.cands);
    else
      hipLaunchKernelGGL(scan_kernel<64>, grid, dim3(NT), 0, s, t, inv, N, d, q, Q, k, w.rps, w.cands);
    DCNR_LAUNCH_CHECK();
    return merge_lists(w.cands, Q, w.ns, k, idx, dist, s);
  }
  if (use_v4(N, Q, d, k)) {
    // query blocks of 16: NQB per launch row (the table is read once per
    // NQB * 16 queries)
    const int nqb = (int)std::min<int64_t>(cdiv(Q, 16), V4_QC / 16);
    const int NQ = nqb <= 2 ? 2 : nqb <= 4 ? 4 : nqb <= 8 ? 8 : 16;
    const int rpb = v4_rpb(NQ, N);
    const dim3 g4((unsigned)cdiv(N, rpb), (unsigned)cdiv(Q, NQ * 16));
    // the admission bound from the first V4_S rows (bound5_kernel, which also
    // normalises the queries), its minima merged by scan4 itself up to V4_MQ
    // queries
    const int ng = (int)cdiv(std::min<int64_t>(N, V4_S), B5_C);
    const bool merge4 = Q <= V4_MQ;
    const dim3 gb((unsigned)ng, (unsigned)cdiv(Q, 16 * (merge4 ? 1 : B5_QG)));
    with_v4_rows(d, tb != nullptr, [&](auto ks, auto pk) {
      constexpr int KS = decltype(ks)::value;
      constexpr bool PK = decltype(pk)::value;
      if (merge4)
        hipLaunchKernelGGL((bound5_kernel<KS, PK, 1>), gb, dim3(256), 0, s, t, inv, tb, N, q, Q, w.qn, w.qb,
                           w.qcnt, w.bmins);
      else
        hipLaunchKernelGGL((bound5_kernel<KS, PK, B5_QG>), gb, dim3(256), 0, s, t, inv, tb, N, q, Q, w.qn, w.qb,
                           w.qcnt, w.bmins);
    });
    DCNR_LAUNCH_CHECK();
    if (!merge4) {
      hipLaunchKernelGGL(bound5_merge_kernel, dim3((unsigned)cdiv(Q, 4)), dim3(256), 0, s, w.bmins, ng, Q, k,
                         w.thr0);
      DCNR_LAUNCH_CHECK();
    }
    with_v4_rows(d, tb != nullptr, [&](auto ks, auto pk) {
      with_v4_nqb(NQ, [&](auto nq) {
        hipLaunchKernelGGL((scan4_kernel<decltype(ks)::value, decltype(nq)::value, decltype(pk)::value>), g4,
                           dim3(256), 0, s, t, inv, tb, N, rpb, w.qb, w.thr0, w.qn, Q, w.qcnt, w.rows, w.dists,
                           merge4 ? w.bmins : nullptr, ng, k);
      });
    });
    DCNR_LAUNCH_CHECK();
    // (a query whose list overflowed: the split fallback for Q <= V4_FQ,
    // else the batched fallback's pool, inside these blocks)
    const int F = v4_fallback_split(Q);
    const int FB = v4_batch_chunks(Q);
    const unsigned nb = (unsigned)(Q * F);
    if (d == 32)
      hipLaunchKernelGGL(rescore_kernel<8>, dim3(nb), dim3(B4_T), 0, s, w.dists, w.qcnt, w.rows, k, idx, dist, t,
                         inv, N, w.qn, Q, F, FB, w.split_d, w.split_i, w.qcnt + Q + 1);
    else
      hipLaunchKernelGGL(rescore_kernel<16>, dim3(nb), dim3(B4_T), 0, s, w.dists, w.qcnt, w.rows, k, idx, dist, t,
                         inv, N, w.qn, Q, F, FB, w.split_d, w.split_i, w.qcnt + Q + 1);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  // scans v2 / v3: normalised queries + admission bounds, one block per query
  with_dv(d / 4, [&](auto dv) {
    hipLaunchKernelGGL(kth_bound_kernel<decltype(dv)::value>, dim3((unsigned)Q), dim3(256), 0, s, t, inv, N, q,
                       w.qn, k, w.thr0);
  });
  DCNR_LAUNCH_CHECK();
  const bool v3 = allow_v3 && Q >= MFMA_MIN_Q && d % 16 == 0;
  const int qtiles = (int)cdiv(Q, v3 ? K3_QT : K2_QT);
  const dim3 blocks((unsigned)(rup(w.ns, 8) * qtiles));
  // scan v3 where it applies, else scan v2: the exact VALU scan (the same
  // distance arithmetic as v4's rescoring and its per-query fallback)
  with_dv(d / 4, [&](auto dv) {
    constexpr int DV = decltype(dv)::value;
    if constexpr (DV % 4 == 0) {
      if (v3) {
        hipLaunchKernelGGL(scan3_kernel<DV>, blocks, dim3(K2_NT), 0, s, t, inv, N, w.qn, Q, k, w.rps, w.ns, qtiles,
                           w.cands, w.thr0);
        return;
      }
    }
    hipLaunchKernelGGL(scan2_kernel<DV>, blocks, dim3(K2_NT), 0, s, t, inv, N, w.qn, Q, k, w.rps, w.ns, qtiles,
                       w.cands, w.thr0);
  });
  DCNR_LAUNCH_CHECK();
  return merge_lists(w.cands, Q, w.ns, k, idx, dist, s);
}

// ---- the set-scoped search: the k nearest rows within a row set
//
// A call carries G segments of queries; segment g searches the rows listed in
// set seg_set[g] of a CSR of row sets (a city's hotels) instead of the table.
// Three launches, no device word read by the host:
//   * within_prep_kernel: one wave per query normalises it, with the
//     expression of the scan cosine_topk takes at this (d, k) -- the two
//     round differently (see there); one wave per segment checks the segment's offsets, its set index and the
//     set's offsets against the lengths passed by value and writes a record
//     (set start, set length or W_SKIP / W_BAD, segment) for each of its
//     queries.  Later kernels use a record only after checking that its
//     segment does hold the query, so a workspace's stale bytes are never
//     followed: a segment that holds a query has overwritten its record.
//   * within_scan_kernel (d <= 64, k <= 32: scan v2's wave-register lists) /
//     within_scan_wide_kernel (the rest: scan v1's LDS buffers and bitonic
//     compaction): work item (window of W_BQ consecutive queries, chunk of
//     rpi set positions).  The window's queries are grouped by segment -- one
//     group when the segments are multiples of W_BQ long, as requests of 8
//     positives are -- and each group's chunk is read once: a lane loads one
//     listed row (its id, checked against N; its inverse norm; its d floats as
//     16-B loads) and scores it against the group's queries.  The k-lists
//     hold table rows, so the merge needs no second mapping.  A row outside
//     [0, N) is never dereferenced: it marks the group's records W_BAD.
//   * within_merge_kernel: merge_kernel's block over the query's chunk lists,
//     written at the caller's row stride; W_BAD and empty sets are padded,
//     W_SKIP and queries no segment holds are left as they were.
// rpi, and with it the chunk count, follows from max_set_rows on the host.
// Rows reach a wave in set order and are admitted strictly under the k-th
// best, so ties keep (distance, row) order when the set is ascending.
constexpr int W_BQ = QT;            // queries per work item
constexpr int64_t W_RPI = 1024;     // set positions per work item, at least
constexpr int W_CHUNKS = 256;       // ... and at most this many chunks
constexpr int W_SKIP = -1, W_BAD = -2;
struct WithinQ { int64_t lo; int len; int seg; };

namespace {

__global__ __launch_bounds__(256) void within_prep_kernel(
    const float* __restrict__ q, int64_t Q, int d, int lane_form, float* __restrict__ qn,
    const int64_t* __restrict__ seg_off,
    int64_t G, const int* __restrict__ seg_set, const int64_t* __restrict__ set_off, int S, int64_t n_set_rows,
    int64_t max_set_rows, int64_t qblocks, WithinQ* recs, int* seg_status) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if ((int64_t)blockIdx.x < qblocks) {
    const int64_t qq = (int64_t)blockIdx.x * 4 + w;
    if (qq >= Q) return;
    if (lane_form) {
      // kth_bound_kernel's / bound5_kernel's wave_sum(v * v), one element per
      // lane, as the compiler contracts it there: the first butterfly step is
      // fma(v, v, the partner's rounded square), so the sum, and with it the
      // scale, may differ between lanes by an ulp -- spelled out, because the
      // answers are compared with those kernels' bit for bit
      const float v = lane < d ? q[qq * d + lane] : 0.f;
      float s = fmaf(v, v, __shfl_xor(v * v, 32, 64));
#pragma unroll
      for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
      const float in = s > 0.f ? 1.f / sqrtf(s) : 1.f;
      if (lane < d) qn[qq * d + lane] = v * in;
      return;
    }
    // scan v1's (scan_kernel's) form
    float s = 0.f;
    for (int i = lane; i < d; i += 64) { float v = q[qq * d + i]; s += v * v; }
    s = wave_sum(s);
    float in = s > 0.f ? 1.f / sqrtf(s) : 1.f;
    for (int i = lane; i < d; i += 64) qn[qq * d + i] = q[qq * d + i] * in;
    return;
  }
  const int64_t g = ((int64_t)blockIdx.x - qblocks) * 4 + w;
  if (g >= G) return;
  const int64_t a = seg_off[g], b = seg_off[g + 1];
  const int s = seg_set[g];
  WithinQ r{0, 0, (int)g};
  if (s < 0) {
    r.len = W_SKIP;
  } else if (a < 0 || b < a || b > Q || s >= S) {
    r.len = W_BAD;
  } else {
    const int64_t lo = set_off[s], hi = set_off[s + 1];
    if (lo < 0 || hi < lo || hi > n_set_rows || hi - lo > max_set_rows) r.len = W_BAD;
    else { r.lo = lo; r.len = (int)(hi - lo); }
  }
  if (seg_status && lane == 0) seg_status[g] = r.len == W_BAD ? DCNR_REQ_BAD_DATA : 0;
  // (every query the segment holds, even when its other offset is out of range)
  const int64_t q0 = a < 0 ? 0 : a, q1 = b > Q ? Q : b;
  for (int64_t qq = q0 + lane; qq < q1; qq += 64) recs[qq] = r;
}

// the record of query qq when its segment does hold it, else a skipped one
__device__ __forceinline__ WithinQ within_record(const WithinQ* recs, const int64_t* __restrict__ seg_off,
                                                 int64_t G, int64_t qq) {
  WithinQ r = recs[qq];
  const bool held = r.seg >= 0 && r.seg < G && seg_off[r.seg] <= qq && qq < seg_off[r.seg + 1];
  if (!held) r = WithinQ{0, W_SKIP, -1};
  return r;
}

// The window's groups, one at a time: next_group() gives the slots (bit qq =
// query q0 + qq) of the first pending slot's segment and that set's start and
// length.  wlen[qq] > p0 marks a slot with rows in this chunk.  (uniform)
__device__ __forceinline__ unsigned within_next_group(unsigned& pend, const int* wseg) {
  const int f = __ffs(pend) - 1;
  unsigned grp = 0;
#pragma unroll
  for (int qq = 0; qq < W_BQ; ++qq)
    if (((pend >> qq) & 1u) && wseg[qq] == wseg[f]) grp |= 1u << qq;
  grp = __builtin_amdgcn_readfirstlane(grp);
  pend &= ~grp;
  return grp;
}

// a row outside [0, N) was listed: the group's queries are padded, its segment flagged
__device__ __forceinline__ void within_mark_bad(unsigned grp, int64_t q0, WithinQ* recs, int seg, int* seg_status) {
  for (int qq = 0; qq < W_BQ; ++qq)
    if ((grp >> qq) & 1u) recs[q0 + qq].len = W_BAD;
  if (seg_status) seg_status[seg] = DCNR_REQ_BAD_DATA;
}

template <int DV>
__global__ __launch_bounds__(K2_NT) void within_scan_kernel(
    const float* __restrict__ tab, const float* __restrict__ inv, int64_t N, const float* __restrict__ qn,
    int64_t Q, const int64_t* __restrict__ excl, const int64_t* __restrict__ seg_off, int64_t G,
    const int64_t* __restrict__ set_rows, WithinQ* recs, int64_t rpi, int nchunks, int k, Cand* lists,
    int* seg_status) {
  __shared__ float cd[K2_WPB][W_BQ][K2_CAP];
  __shared__ int ci[K2_WPB][W_BQ][K2_CAP];
  __shared__ int cntl[K2_WPB][W_BQ];
  __shared__ int64_t wlo[W_BQ];
  __shared__ int wlen[W_BQ], wseg[W_BQ], wex[W_BQ];
  const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
  const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)nchunks) * W_BQ;
  const int64_t p0 = (int64_t)chunk * rpi;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x < W_BQ) {
    const int64_t qq = q0 + threadIdx.x;
    WithinQ r{0, W_SKIP, -1};
    int64_t e = -1;
    if (qq < Q) {
      r = within_record(recs, seg_off, G, qq);
      if (excl) e = excl[qq];
    }
    wlo[threadIdx.x] = r.lo;
    wlen[threadIdx.x] = r.len;
    wseg[threadIdx.x] = r.seg;
    wex[threadIdx.x] = e >= 0 && e < N ? (int)e : -1;
  }
  __syncthreads();
  unsigned pend = 0;
#pragma unroll
  for (int qq = 0; qq < W_BQ; ++qq)
    if ((int64_t)wlen[qq] > p0) pend |= 1u << qq;
  pend = __builtin_amdgcn_readfirstlane(pend);
  const unsigned act = pend;
  if (!act) return;
  // slot qq's list count and k-th best of this wave live in lane qq
  int cntv = 0;
  float thrv = FLT_MAX;
  const float4* qv = reinterpret_cast<const float4*>(qn + q0 * DV * 4);
  while (pend) {
    const int f = __ffs(pend) - 1;
    const unsigned grp = within_next_group(pend, wseg);
    const int64_t lo = wlo[f];
    const int64_t p1 = min<int64_t>(wlen[f], p0 + rpi);
    bool bad = false;
    for (int64_t base = p0 + 64 * w; base < p1; base += 64 * K2_WPB) {
      const int64_t p = base + lane;
      bool ok = p < p1;
      int64_t r = ok ? set_rows[lo + p] : 0;
      if (r < 0 || r >= N) { bad = true; ok = false; r = 0; }
      float4 x[DV];
      load_row<DV>(tab, r, x);
      const float ir = inv[r];
#pragma unroll 1
      for (int qq = 0; qq < W_BQ; ++qq) {
        if (!((grp >> qq) & 1u)) continue;   // (uniform)
        const float dist = exact_dist<DV>(x, qv + qq * DV, ir);
        float th = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(thrv), qq));
        const bool cand = ok && (int)r != wex[qq];
        if (!__ballot(cand && dist < th)) continue;
        int c = __builtin_amdgcn_readlane(cntv, qq);
        wave_admit(cd[w][qq], ci[w][qq], c, th, k, lane, cand, dist, r);
        cntv = lane == qq ? c : cntv;
        thrv = lane == qq ? th : thrv;
      }
    }
    if (__ballot(bad) && lane == 0) within_mark_bad(grp, q0, recs, wseg[f], seg_status);
  }
  for (int qq = 0; qq < W_BQ; ++qq) {
    if (!((act >> qq) & 1u)) continue;
    float th;
    const int c = wave_compact(cd[w][qq], ci[w][qq], __builtin_amdgcn_readlane(cntv, qq), k, lane, &th);
    if (lane == 0) cntl[w][qq] = c;
  }
  __syncthreads();
  for (int qq = w; qq < W_BQ; qq += K2_WPB) {
    if (!((act >> qq) & 1u)) continue;
    float d;
    int i;
    wave_merge_lists<K2_WPB>(cd[0][qq], ci[0][qq], &cntl[0][qq], W_BQ * K2_CAP, W_BQ, k, lane, d, i);
    Cand* o = lists + ((q0 + qq) * nchunks + chunk) * (int64_t)k;
    if (lane < k) o[lane] = Cand{d, i};
  }
}

template <int MAXV>
__global__ __launch_bounds__(NT) void within_scan_wide_kernel(
    const float* __restrict__ tab, const float* __restrict__ inv, int64_t N, int d, const float* __restrict__ qn,
    int64_t Q, const int64_t* __restrict__ excl, const int64_t* __restrict__ seg_off, int64_t G,
    const int64_t* __restrict__ set_rows, WithinQ* recs, int64_t rpi, int nchunks, int k, Cand* lists,
    int* seg_status) {
  __shared__ __attribute__((aligned(16))) float qs[W_BQ][MAXV * 4];
  __shared__ float cd[W_BQ][CAP];
  __shared__ int ci[W_BQ][CAP];
  __shared__ int cnt[W_BQ];
  __shared__ float thr[W_BQ];
  __shared__ int64_t wlo[W_BQ];
  __shared__ int wlen[W_BQ], wseg[W_BQ], wex[W_BQ];
  __shared__ int badf;
  const int chunk = (int)(blockIdx.x % (unsigned)nchunks);
  const int64_t q0 = (int64_t)(blockIdx.x / (unsigned)nchunks) * W_BQ;
  const int64_t p0 = (int64_t)chunk * rpi;
  const int nq = (int)min<int64_t>(W_BQ, Q - q0);
  if (threadIdx.x < W_BQ) {
    const int64_t qq = q0 + threadIdx.x;
    WithinQ r{0, W_SKIP, -1};
    int64_t e = -1;
    if (qq < Q) {
      r = within_record(recs, seg_off, G, qq);
      if (excl) e = excl[qq];
    }
    wlo[threadIdx.x] = r.lo;
    wlen[threadIdx.x] = r.len;
    wseg[threadIdx.x] = r.seg;
    wex[threadIdx.x] = e >= 0 && e < N ? (int)e : -1;
    cnt[threadIdx.x] = 0;
    thr[threadIdx.x] = FLT_MAX;
  }
  if (threadIdx.x == 0) badf = 0;
  for (int i = threadIdx.x; i < nq * d; i += NT) qs[i / d][i % d] = qn[q0 * d + i];
  __syncthreads();
  unsigned pend = 0;
#pragma unroll
  for (int qq = 0; qq < W_BQ; ++qq)
    if ((int64_t)wlen[qq] > p0) pend |= 1u << qq;
  pend = __builtin_amdgcn_readfirstlane(pend);
  const unsigned act = pend;
  if (!act) return;
  const int dv = d >> 2;
  while (pend) {
    const int f = __ffs(pend) - 1;
    const unsigned grp = within_next_group(pend, wseg);
    const int64_t lo = wlo[f];
    const int64_t p1 = min<int64_t>(wlen[f], p0 + rpi);
    for (int64_t base = p0; base < p1; base += NT) {
      const int64_t p = base + threadIdx.x;
      if (p < p1) {
        const int64_t r = set_rows[lo + p];
        if (r < 0 || r >= N) {
          badf = 1;
        } else {
          float4 x[MAXV];
          const float4* rp = reinterpret_cast<const float4*>(tab + r * d);
#pragma unroll
          for (int v = 0; v < MAXV; ++v) if (v < dv) x[v] = rp[v];
          const float ir = inv[r];
          for (int qq = 0; qq < W_BQ; ++qq) {
            if (!((grp >> qq) & 1u)) continue;
            const float4* qp = reinterpret_cast<const float4*>(qs[qq]);
            float s = 0.f;
#pragma unroll
            for (int v = 0; v < MAXV; ++v)
              if (v < dv) {
                float4 wq = qp[v];
                s += dot4(x[v], wq);
              }
            float dist = cos_dist(s, ir);
            if (dist <= thr[qq] && (int)r != wex[qq]) {
              int pos = atomicAdd(&cnt[qq], 1);
              cd[qq][pos] = dist;
              ci[qq][pos] = (int)r;
            }
          }
        }
      }
      __syncthreads();
      for (int qq = 0; qq < W_BQ; ++qq) {
        if (cnt[qq] > CAP - NT) compact(cd[qq], ci[qq], &cnt[qq], &thr[qq], k);
      }
      __syncthreads();   // (no append of the next step before every thread has read the counts)
    }
    if (badf) {   // (uniform: read after the barrier, reset behind the next one)
      if (threadIdx.x == 0) within_mark_bad(grp, q0, recs, wseg[f], seg_status);
      __syncthreads();
      if (threadIdx.x == 0) badf = 0;
    }
  }
  for (int qq = 0; qq < W_BQ; ++qq) {
    if (!((act >> qq) & 1u)) continue;
    compact(cd[qq], ci[qq], &cnt[qq], &thr[qq], k);
    Cand* o = lists + ((q0 + qq) * nchunks + chunk) * (int64_t)k;
    for (int t = threadIdx.x; t < k; t += NT) {
      bool ok = t < cnt[qq];
      o[t] = Cand{ok ? cd[qq][t] : FLT_MAX, ok ? ci[qq][t] : INT_MAX};
    }
  }
}

__global__ __launch_bounds__(NT) void within_merge_kernel(const Cand* lists, int nchunks, int64_t rpi, int k,
                                                          int64_t ld, int64_t* idx, float* dist,
                                                          const int64_t* __restrict__ seg_off, int64_t G,
                                                          const WithinQ* recs) {
  const int64_t qq = blockIdx.x;
  const WithinQ r = within_record(recs, seg_off, G, qq);   // (uniform)
  if (r.len == W_SKIP) return;
  idx += qq * ld;
  dist += qq * ld;
  if (r.len <= 0) {   // W_BAD, or an empty set
    for (int t = threadIdx.x; t < k; t += NT) { idx[t] = -1; dist[t] = FLT_MAX; }
    return;
  }
  merge_block(lists + qq * (int64_t)nchunks * k, (int)((r.len + rpi - 1) / rpi), k, idx, dist);
}

}  // namespace

// The scratch of one set-scoped search (null base: `total` is the size):
// normalised queries [Q][d] | records [Q] | chunk k-lists [Q][chunks][k]
struct WithinWs { int nchunks; int64_t rpi; float* qn; WithinQ* recs; Cand* lists; size_t total; };
WithinWs carve_within(void* ws, int64_t Q, int k, int d, int64_t max_set_rows) {
  WithinWs w{};
  Bump b(ws);
  w.rpi = std::max<int64_t>(W_RPI, rup(cdiv(max_set_rows, W_CHUNKS), 256));
  w.nchunks = (int)std::max<int64_t>(1, cdiv(max_set_rows, w.rpi));
  w.qn = (float*)b.take((size_t)Q * d * 4);
  w.recs = (WithinQ*)b.take((size_t)Q * sizeof(WithinQ));
  // (room for the most chunks any smaller bound plans, so that the size grows with the bound)
  const int64_t room = std::max<int64_t>(1, std::min<int64_t>(W_CHUNKS, cdiv(max_set_rows, W_RPI)));
  w.lists = (Cand*)b.take((size_t)Q * room * k * sizeof(Cand));
  w.total = b.off;
  return w;
}

bool within_shape_ok(int64_t Q, int k, int d, int64_t max_set_rows) {
  return Q >= 0 && k >= 1 && k <= KMAX && d >= 4 && d % 4 == 0 && d <= 256 && max_set_rows >= 0 &&
         max_set_rows <= INT32_MAX && Q <= INT32_MAX;
}

static size_t cosine_topk_within_ws(int64_t Q, int k, int d, int64_t max_set_rows) {
  if (!within_shape_ok(Q, k, d, max_set_rows)) return 0;
  return carve_within(nullptr, Q, k, d, max_set_rows).total + 256;   // (never 0 for a shape it takes)
}

// ---- the item neighbour table: the top-k of every table row, built once
//
// Row r of the table is the answer of cosine_topk for the single query t[r].
// The build walks the rows in chunks of NBR_CHUNK queries through cosine_topk
// with the query pointer inside the table, and keeps scan v3 out: v1, v2, v4
// and their fallbacks all end in dot4 / cos_dist, so a row's distances, and
// with them its order among ties, do not depend on the chunk it was built in
// or on the width of the batch; v3's MFMA sums in another order.
constexpr int64_t NBR_CHUNK = 1024;

__global__ void narrow_idx_kernel(const int64_t* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x)
    out[e] = (int32_t)in[e];
}

// One chunk's scratch, carved once: idx [NBR_CHUNK][k] int64 | dist (when the
// caller wants none) | the search's own workspace, the largest any chunk
// width up to NBR_CHUNK asks for (the last chunk of a range is narrower, and
// the search's plan is not monotone in Q)
struct NbrWs { int64_t* idx; float* dist; void* topk; size_t topk_bytes, total; };
NbrWs carve_nbr(void* ws, int64_t N, int k) {
  NbrWs w{};
  Bump b(ws);
  w.idx = (int64_t*)b.take((size_t)NBR_CHUNK * k * sizeof(int64_t));
  w.dist = (float*)b.take((size_t)NBR_CHUNK * k * sizeof(float));
  for (int64_t Q = 1; Q <= NBR_CHUNK; ++Q) w.topk_bytes = std::max(w.topk_bytes, topk_ws(N, Q, k));
  w.topk = b.take(w.topk_bytes);
  w.total = b.off;
  return w;
}

static size_t neighbor_table_ws(int64_t N, int k) { return carve_nbr(nullptr, N, k).total; }

// ---- the item neighbour table, updated in place after m rows changed
//
// C: the changed rows (their vectors, inv and packed rows already new); kt:
// the table's width; L(r): row r's list as it stands, exact for the table
// before the change.  Keys are (distance, row) under cless, every distance
// from the new table.  A row outside C keeps its vector, so its distance to
// another such row is what it was; the old distance to a changed row is never
// needed.
//   * r in C: searched again.
//   * r not in C, no member of C in L(r), every c in C with a key above the
//     list's last: untouched (the filter, phase A).
//   * else (the merge, phase B): K' = the largest key of L(r) \ C.  Every row
//     outside L(r) and C has its old key, above the old k-th key >= K'.  So
//     when L(r) \ C and the c in C with key <= K' number at least kt, the kt
//     smallest of them are the new list; with fewer, a changed row left a
//     hole that only a scan can fill: searched again.  So is a row with no
//     entry outside C, and one whose candidates exceed UPD_CAP.
// The re-search (phase C) is the build over a list of rows.
//
// Phase A marks a superset: the exact k-th distance dk of r (its last entry
// is outside C, or the row is affected anyway), and then, d = 32 / 64, scan
// v4's coarse bf16 cosine of r against every c -- |coarse - exact| <= 2^-7 +
// 2^-16 + fp32 slack < V4_EPS, 2^-8 per bf16 factor (scan v4's comment; DESIGN
// section 4), so coarse <= dk + V4_EPS + TH_MARGIN holds for every c
// with exact distance <= dk: one margin, because dk itself is exact (a coarse
// dk would double it and gather as many rows) -- or, other widths, the exact
// distance against dk + TH_MARGIN.  A row is appended once, by the block that
// owns it; the order of the lists decides nothing (each row's result depends
// on that row alone).
constexpr int UPD_MAX_M = 16384;   // changed rows per call
constexpr int UPD_CT = V4_QC;      // changed rows per LDS tile of the MFMA filter
constexpr int UPD_RPB = 1024;      // table rows per block of the MFMA filter
constexpr int UPD_XT = 16;         // changed rows per LDS tile of the exact filter
constexpr int UPD_CAP = CAP;       // merge candidates per row
constexpr int UPD_DMAX = 256;      // cosine_topk's widest row
constexpr float UPD_NEVER = -1.f;  // k-th distance of a row the filter skips

namespace {

__device__ __forceinline__ bool upd_bit(const unsigned* __restrict__ bits, int r) {
  return (bits[r >> 5] >> (r & 31)) & 1u;
}

// exact distance of table row e to the normalised query qv (dv float4 chunks):
// dot4 per chunk in order, then cos_dist -- exact_dist's sum at a run-time width
__device__ __forceinline__ float upd_row_dist(const float* __restrict__ tab, const float* __restrict__ inv,
                                              int64_t e, int dv, const float4* qv) {
  const float4* rp = reinterpret_cast<const float4*>(tab) + e * dv;
  float s = 0.f;
  for (int v = 0; v < dv; ++v) s += dot4(rp[v], qv[v]);
  return cos_dist(s, inv[e]);
}

// the changed rows into the bitmap and the head of the re-search list; counts
__global__ void upd_mark_kernel(const int* __restrict__ chg, int m, unsigned* bits, int* research, int* counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) {
    const int c = chg[i];
    atomicOr(&bits[c >> 5], 1u << (c & 31));
    research[i] = c;
  }
  if (i == 0) { counts[0] = m; counts[1] = 0; counts[2] = 0; counts[3] = m; }
}

// Phase A, first pass, one row per thread: a row whose list holds a member
// of C (or an entry outside the table) is affected; every other row outside C
// gets its exact k-th distance, query r against its last entry.
__global__ __launch_bounds__(256) void upd_kth_kernel(const float* __restrict__ tab, const float* __restrict__ inv,
                                                      int N, int dv, int kt, const int* __restrict__ nbr,
                                                      const unsigned* __restrict__ bits, float* kth, int* aff,
                                                      int* counts) {
  const int64_t r64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r64 >= N) return;
  const int r = (int)r64;
  if (upd_bit(bits, r)) { kth[r] = UPD_NEVER; return; }
  const int* L = nbr + (int64_t)r * kt;
  bool hit = false;
  int last = 0;
  for (int j = 0; j < kt; ++j) {
    last = L[j];
    hit = hit || (unsigned)last >= (unsigned)N || upd_bit(bits, last);
  }
  if (hit) {
    aff[atomicAdd(&counts[1], 1)] = r;
    kth[r] = UPD_NEVER;
    return;
  }
  const float4* xr = reinterpret_cast<const float4*>(tab) + (int64_t)r * dv;
  const float4* xe = reinterpret_cast<const float4*>(tab) + (int64_t)last * dv;
  const float ir = inv[r];
  float s = 0.f;
  for (int v = 0; v < dv; ++v) {
    const float4 x = xr[v];
    s += dot4(xe[v], float4{x.x * ir, x.y * ir, x.z * ir, x.w * ir});
  }
  kth[r] = cos_dist(s, inv[last]);
}

// Phase A, d = 32 / 64: scan4's MFMA with the changed rows in the queries'
// place.  A block owns UPD_RPB table rows; per tile of UPD_CT changed rows it
// stages their bf16 B fragments in LDS in fragment order (entry (b, ks, lane)
// is lane's 16 B: conflict-free ds_read_b128, as scan4's bqs), rounded from
// the fp32 rows as pack_rows_kernel rounds them, then walks its rows in
// 16-row A tiles (the packed copy, or fp32 rows scaled and rounded here).
// Lane (c, g) of an accumulator holds rows 4 g + i against changed row
// 16 b + c; a row passes when any c reaches its bound.  Hits are kept as a
// bitmap of the block's rows in LDS and appended once at the end.
template <int KS, bool PK>
__global__ __launch_bounds__(256) void upd_filter4_kernel(const float* __restrict__ tab,
                                                          const float* __restrict__ inv,
                                                          const bf16* __restrict__ tb, int N,
                                                          const int* __restrict__ chg, int m,
                                                          const float* __restrict__ kth, int* aff, int* counts) {
  constexpr int D = KS * 32;
  __shared__ bf16x8 bqs[(UPD_CT / 16) * KS * 64];
  __shared__ unsigned hit[UPD_RPB / 32];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * UPD_RPB;
  const int64_t r1 = min<int64_t>(N, r0 + UPD_RPB);
  for (int i = threadIdx.x; i < UPD_RPB / 32; i += 256) hit[i] = 0;
  for (int c0 = 0; c0 < m; c0 += UPD_CT) {
    const int nc = min(UPD_CT, m - c0);
    const int nb = (nc + 15) / 16;
    __syncthreads();   // (the tile before is read out; hit[] is zeroed)
    for (int e = threadIdx.x; e < nb * KS * 64; e += 256) {
      const int l = e & 63, ks = (e >> 6) % KS, b = (e >> 6) / KS;
      const int ci = 16 * b + (l & 15);
      bf16x8 v = bf16x8{};
      if (ci < nc) {
        const int64_t c = chg[c0 + ci];
        const float4* p = reinterpret_cast<const float4*>(tab + c * D + ks * 32 + 8 * (l >> 4));
        const float4 lo = p[0], hi = p[1];
        const float sc = inv[c];
        v = bf16x8{(bf16)(lo.x * sc), (bf16)(lo.y * sc), (bf16)(lo.z * sc), (bf16)(lo.w * sc),
                   (bf16)(hi.x * sc), (bf16)(hi.y * sc), (bf16)(hi.z * sc), (bf16)(hi.w * sc)};
      }
      bqs[e] = v;
    }
    __syncthreads();
    for (int64_t base = r0 + 16 * w; base < r1; base += 64) {
      const int64_t ra = base + r16 < r1 ? base + r16 : r0;
      bf16x8 a[KS];
      if constexpr (PK) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ks] = *reinterpret_cast<const bf16x8*>(tb + ra * D + ks * 32 + 8 * g);
      } else {
        float4 x[KS][2];
        v4_load_rows<KS>(tab, ra, x, g);
        const float sc = inv[ra];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const float4 p = x[ks][0], v = x[ks][1];
          a[ks] = bf16x8{(bf16)(p.x * sc), (bf16)(p.y * sc), (bf16)(p.z * sc), (bf16)(p.w * sc),
                         (bf16)(v.x * sc), (bf16)(v.y * sc), (bf16)(v.z * sc), (bf16)(v.w * sc)};
        }
      }
      // a row passes iff a coarse cosine is >= 1 - its bound (the 1e-6 covers
      // the rounding of 1 - bound); skipped rows and rows past r1: 3, never
      float th[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t rr = base + 4 * g + i;
        const float t = rr < r1 ? kth[rr] : UPD_NEVER;
        th[i] = t < 0.f ? 3.f : (1.f - (t + V4_EPS + TH_MARGIN)) - 1e-6f;
      }
      bool pass[4] = {false, false, false, false};
      for (int b = 0; b < nb; ++b) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], bqs[(b * KS + ks) * 64 + lane], acc, 0, 0, 0);
        const bool valid = 16 * b + r16 < nc;   // (a padded column's cosine is 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) pass[i] = pass[i] || (valid && acc[i] >= th[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint64_t mk = __ballot(pass[i]);
        if (!mk) continue;
        const int j = (int)(base + 4 * g + i - r0);   // (< UPD_RPB: a passing row lies under r1)
        if (r16 == 0 && ((mk >> (16 * g)) & 0xffffull)) atomicOr(&hit[j >> 5], 1u << (j & 31));
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < UPD_RPB; j += 256)
    if ((hit[j >> 5] >> (j & 31)) & 1u) aff[atomicAdd(&counts[1], 1)] = (int)(r0 + j);
}

// Phase A, every other width: one row per thread against tiles of UPD_XT
// changed rows broadcast from LDS (uniform addresses), exact distances in
// the merge's direction (query r, row c)
__global__ __launch_bounds__(256) void upd_filter_exact_kernel(const float* __restrict__ tab,
                                                               const float* __restrict__ inv, int N, int dv,
                                                               const int* __restrict__ chg, int m,
                                                               const float* __restrict__ kth, int* aff,
                                                               int* counts) {
  __shared__ float4 xc[UPD_XT * (UPD_DMAX / 4)];
  __shared__ float ic[UPD_XT];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool ok = r < N;
  const float t = ok ? kth[r] : UPD_NEVER;
  const bool active = t >= 0.f;
  const float ir = ok ? inv[r] : 1.f;
  const float4* xr = reinterpret_cast<const float4*>(tab) + (ok ? r : 0) * dv;
  const float4* tab4 = reinterpret_cast<const float4*>(tab);
  bool pass = false;
  for (int c0 = 0; c0 < m; c0 += UPD_XT) {
    const int nc = min(UPD_XT, m - c0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * dv; e += 256) xc[e] = tab4[(int64_t)chg[c0 + e / dv] * dv + e % dv];
    if ((int)threadIdx.x < nc) ic[threadIdx.x] = inv[chg[c0 + threadIdx.x]];
    __syncthreads();
    if (!active || pass) continue;
    float s[UPD_XT];
#pragma unroll
    for (int j = 0; j < UPD_XT; ++j) s[j] = 0.f;
    for (int v = 0; v < dv; ++v) {
      const float4 x = xr[v];
      const float4 q = float4{x.x * ir, x.y * ir, x.z * ir, x.w * ir};
#pragma unroll
      for (int j = 0; j < UPD_XT; ++j)
        if (j < nc) s[j] += dot4(xc[j * dv + v], q);
    }
#pragma unroll
    for (int j = 0; j < UPD_XT; ++j)
      if (j < nc) pass = pass || cos_dist(s[j], ic[j]) <= t + TH_MARGIN;
  }
  if (pass) aff[atomicAdd(&counts[1], 1)] = (int)r;
}

// Phase B: a workgroup per UPD_G affected rows (grid-stride over the list,
// whose length only the device knows).  Per row r: the exact distances of
// L(r) \ C and their largest key K' (a wave per row), then of every c in C,
// those with key <= K' kept; with at least kt candidates the kt smallest by
// (distance, row) are written into row r of the table, else r joins the
// re-search list.  The changed rows are the expensive part -- m gathered rows
// per affected row -- so a thread loads each chunk of a changed row once and
// scores it against the UPD_G queries held in LDS (uniform addresses), each
// query's sum in upd_row_dist's order.
constexpr int UPD_G = 8;
__global__ __launch_bounds__(NT) void upd_merge_kernel(const float* __restrict__ tab, const float* __restrict__ inv,
                                                       int N, int d, int kt, const int* __restrict__ chg, int m,
                                                       const unsigned* __restrict__ bits,
                                                       const int* __restrict__ aff, int* nbr, int* research,
                                                       int* counts) {
  __shared__ __attribute__((aligned(16))) float qs[UPD_G][UPD_DMAX];
  __shared__ float cd[UPD_G][UPD_CAP];
  __shared__ int ci[UPD_G][UPD_CAP];
  __shared__ int cnt[UPD_G], bad[UPD_G], ki[UPD_G], rowg[UPD_G];
  __shared__ float kd[UPD_G];
  const int na = counts[1];
  const int dv = d >> 2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float4* tab4 = reinterpret_cast<const float4*>(tab);
  for (int a0 = blockIdx.x * UPD_G; a0 < na; a0 += gridDim.x * UPD_G) {
    const int ng = min(UPD_G, na - a0);
    __syncthreads();   // (the rows before are done with the LDS words)
    if (threadIdx.x < UPD_G) {
      cnt[threadIdx.x] = 0;
      bad[threadIdx.x] = 0;
      rowg[threadIdx.x] = (int)threadIdx.x < ng ? aff[a0 + threadIdx.x] : 0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < ng * d; e += NT) {
      const int g = e / d, i = e % d, r = rowg[g];
      qs[g][i] = tab[(int64_t)r * d + i] * inv[r];
    }
    __syncthreads();
    for (int g = w; g < ng; g += NT / 64) {
      if (lane < kt) {
        const int e = nbr[(int64_t)rowg[g] * kt + lane];
        if ((unsigned)e >= (unsigned)N) {
          bad[g] = 1;
        } else if (!upd_bit(bits, e)) {
          const float dd = upd_row_dist(tab, inv, e, dv, reinterpret_cast<const float4*>(qs[g]));
          const int pos = atomicAdd(&cnt[g], 1);
          cd[g][pos] = dd;
          ci[g][pos] = e;
        }
      }
      // K': the largest key among them (the wave's own LDS writes, fenced as wave_compact's)
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const int nl = cnt[g];   // <= kt <= 64
      float dd = lane < nl ? cd[g][lane] : -1.f;
      int ii = lane < nl ? ci[g][lane] : 0;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float od = __shfl_xor(dd, o, 64);
        const int oi = __shfl_xor(ii, o, 64);
        if (cless(dd, ii, od, oi)) { dd = od; ii = oi; }
      }
      if (lane == 0) {
        kd[g] = dd;
        ki[g] = ii;
        if (nl == 0) bad[g] = 1;   // no entry outside C: searched again
      }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += NT) {
      const int c = chg[j];
      const float4* rp = tab4 + (int64_t)c * dv;
      float s[UPD_G];
#pragma unroll
      for (int g = 0; g < UPD_G; ++g) s[g] = 0.f;
      for (int v = 0; v < dv; ++v) {
        const float4 x = rp[v];
#pragma unroll
        for (int g = 0; g < UPD_G; ++g) s[g] += dot4(x, reinterpret_cast<const float4*>(qs[g])[v]);
      }
      const float ic = inv[c];
#pragma unroll
      for (int g = 0; g < UPD_G; ++g) {
        if (g >= ng || bad[g]) continue;   // (slots past ng hold another group's queries)
        const float dd = cos_dist(s[g], ic);
        if (!cless(kd[g], ki[g], dd, c)) {
          const int pos = atomicAdd(&cnt[g], 1);
          if (pos < UPD_CAP) { cd[g][pos] = dd; ci[g][pos] = c; }
        }
      }
    }
    __syncthreads();
    // up to 64 candidates (the usual case): a wave per row sorts them in registers
    for (int g = w; g < ng; g += NT / 64) {
      const int T = cnt[g];
      if (bad[g] || T < kt || T > 64) continue;
      float dd = lane < T ? cd[g][lane] : FLT_MAX;
      int ii = lane < T ? ci[g][lane] : INT_MAX;
      wave_sort64(dd, ii, lane);
      if (lane < kt) nbr[(int64_t)rowg[g] * kt + lane] = ii;
      if (lane == 0) atomicAdd(&counts[2], 1);
    }
    // more: the block's bitonic sort, row by row; the rest joins the re-search list
    for (int g = 0; g < ng; ++g) {
      const int T = cnt[g];   // (block-uniform)
      const bool redo = bad[g] || T < kt || T > UPD_CAP;
      if (redo) {
        if (threadIdx.x == 0) research[atomicAdd(&counts[3], 1)] = rowg[g];
        continue;
      }
      if (T <= 64) continue;
      int n2 = 128;
      while (n2 < T) n2 <<= 1;
      for (int t = T + threadIdx.x; t < n2; t += NT) { cd[g][t] = FLT_MAX; ci[g][t] = INT_MAX; }
      __syncthreads();
      bitonic<NT>(cd[g], ci[g], n2);
      if ((int)threadIdx.x < kt) nbr[(int64_t)rowg[g] * kt + threadIdx.x] = ci[g][threadIdx.x];
      if (threadIdx.x == 0) atomicAdd(&counts[2], 1);
    }
  }
}

// dcnr_cosine_neighbor_table_affected: the affected rows behind the changed
// ones in the re-search list, in place of the merge
__global__ void upd_list_kernel(const int* __restrict__ aff, int m, int* research, int* counts) {
  const int na = counts[1];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < na; i += gridDim.x * blockDim.x) research[m + i] = aff[i];
}
__global__ void upd_list_counts_kernel(int* counts) {
  if (threadIdx.x == 0) counts[3] = counts[0] + counts[1];
}

// Phase C: the listed rows as a chunk of queries, and the chunk's answers
// into the listed table rows (a row id outside the table is read as row 0
// and written nowhere)
__global__ void upd_gather_kernel(const float* __restrict__ tab, int N, int d, const int* __restrict__ rows,
                                  int64_t n, float* __restrict__ q) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * d; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = rows[e / d];
    q[e] = tab[(int64_t)((unsigned)r < (unsigned)N ? r : 0) * d + e % d];
  }
}
__global__ void upd_scatter_kernel(const int64_t* __restrict__ idx, int64_t n, int k, int N,
                                   const int* __restrict__ rows, int32_t* nbr) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * k; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = rows[e / k];
    if ((unsigned)r < (unsigned)N) nbr[(int64_t)r * k + e % k] = (int32_t)idx[e];
  }
}

// One workspace for both calls: phases A + B carve chg [m] | the bitmap of C
// | the rows' k-th distances [N] | the affected rows [N]; phase C a chunk of
// gathered queries and the build's chunk scratch.
struct UpdWs { int* chg; unsigned* bits; float* kth; int* aff; size_t ab_total;
               float* q; NbrWs nbr; size_t c_total; };
UpdWs carve_upd(void* ws, int64_t N, int d, int k, int64_t m) {
  UpdWs w{};
  Bump b(ws);
  w.chg = (int*)b.take((size_t)std::max<int64_t>(m, 1) * 4);
  w.bits = (unsigned*)b.take((size_t)cdiv(N, 32) * 4);
  w.kth = (float*)b.take((size_t)N * 4);
  w.aff = (int*)b.take((size_t)N * 4);
  w.ab_total = b.off;
  Bump c(ws);
  w.q = (float*)c.take((size_t)NBR_CHUNK * d * 4);
  const size_t q_end = rup((int64_t)c.off, 256);
  w.nbr = carve_nbr(ws ? (char*)ws + q_end : nullptr, N, k);
  w.c_total = q_end + w.nbr.total;
  return w;
}

}  // namespace

static size_t neighbor_table_update_ws(int64_t N, int d, int k, int64_t m) {
  const UpdWs w = carve_upd(nullptr, N, d, k, m);
  return std::max(w.ab_total, w.c_total);
}
}  // namespace dcnr

using namespace dcnr;

extern "C" {

dcnr_status dcnr_row_inv_norms(const float* table, int64_t N, int32_t d, float* inv_norms,
                               dcnr_stream_t stream) {
  if (!table || !inv_norms || d < 1 || N < 0) {
    set_error("dcnr_row_inv_norms: bad argument");
    return DCNR_BAD_ARG;
  }
  if (N <= 0) return DCNR_OK;
  int64_t blocks = std::min<int64_t>(cdiv(N, 4), 8192);
  hipLaunchKernelGGL(inv_norm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, N, d,
                     inv_norms);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

size_t dcnr_cosine_topk_workspace_size(int64_t N, int64_t Q, int32_t k) {
  if (N < 1 || Q < 1 || k < 1) return 256;   // nothing to plan (cosine_topk returns or rejects)
  return topk_ws(N, Q, k) + 256;
}

dcnr_status dcnr_cosine_pack_rows(const float* table, const float* inv_norms, int64_t N, int32_t d,
                                  uint16_t* packed, dcnr_stream_t stream) {
  if (!table || !inv_norms || !packed || d < 1 || N < 0) {
    set_error("dcnr_cosine_pack_rows: bad argument");
    return DCNR_BAD_ARG;
  }
  if (d % 8) {
    set_error("cosine_pack_rows: d=%d is not a multiple of 8", d);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (N <= 0) return DCNR_OK;
  const int64_t blocks = std::min<int64_t>(cdiv(N * d / 8, 256), 8192);
  hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table,
                     inv_norms, N, d, (bf16*)packed);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_cosine_topk_packed(const float* table, const float* inv_norms, const uint16_t* packed,
                                    int64_t N, int32_t d, const float* queries, int64_t Q, int32_t k,
                                    int64_t* idx, float* dist, void* ws, size_t ws_bytes,
                                    dcnr_stream_t stream) {
  // (no queries: the query and output pointers may be null)
  if (!table || !inv_norms || (Q > 0 && (!queries || !idx || !dist || !ws))) {
    set_error("dcnr_cosine_topk: null argument");
    return DCNR_BAD_ARG;
  }
  if (k > N) {
    set_error("Expected n_neighbors <= n_samples_fit, but n_neighbors = %d, n_samples_fit = %lld",
              k, (long long)N);
    return DCNR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  TRYB(DCNR_K_KNN, s, (double)N * (4.0 * d + 4.0),
       cosine_topk(table, inv_norms, (const bf16*)packed, N, d, queries, Q, k, idx, dist, ws, ws_bytes, s));
  return DCNR_OK;
}

dcnr_status dcnr_cosine_topk(const float* table, const float* inv_norms, int64_t N, int32_t d,
                             const float* queries, int64_t Q, int32_t k, int64_t* idx, float* dist,
                             void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  return dcnr_cosine_topk_packed(table, inv_norms, nullptr, N, d, queries, Q, k, idx, dist, ws, ws_bytes,
                                 stream);
}

size_t dcnr_cosine_topk_within_workspace_size(int64_t Q, int32_t k, int32_t d, int64_t max_set_rows) {
  return cosine_topk_within_ws(Q, k, d, max_set_rows);   // (0 for what the call rejects)
}

dcnr_status dcnr_cosine_topk_within(const float* table, const float* inv_norms, int64_t N, int32_t d,
                                    const float* queries, int64_t Q, const int64_t* exclude,
                                    const int64_t* seg_offsets, int64_t G, const int32_t* seg_set,
                                    const int64_t* set_rows, int64_t n_set_rows, const int64_t* set_offsets,
                                    int32_t S, int64_t max_set_rows, int32_t k, int64_t ld, int64_t* idx,
                                    float* dist, int32_t* seg_status, void* ws, size_t ws_bytes,
                                    dcnr_stream_t stream) {
  if (Q < 0 || G < 0 || S < 0 || N < 1 || n_set_rows < 0 || max_set_rows < 0 || k < 1 || ld < k) {
    set_error("dcnr_cosine_topk_within: bad argument (N=%lld, Q=%lld, G=%lld, S=%d, k=%d, ld=%lld, "
              "n_set_rows=%lld, max_set_rows=%lld)", (long long)N, (long long)Q, (long long)G, S, k,
              (long long)ld, (long long)n_set_rows, (long long)max_set_rows);
    return DCNR_BAD_ARG;
  }
  // (set_rows may be null when the CSR holds no row)
  if (Q > 0 && (!table || !inv_norms || !queries || !idx || !dist || !ws ||
                (G > 0 && (!seg_offsets || !seg_set || !set_offsets || (n_set_rows > 0 && !set_rows))))) {
    set_error("dcnr_cosine_topk_within: null argument");
    return DCNR_BAD_ARG;
  }
  if (k > KMAX || d % 4 || d < 4 || d > 256 || N > INT32_MAX || n_set_rows > INT32_MAX ||
      max_set_rows > INT32_MAX || Q > INT32_MAX || G > INT32_MAX) {
    set_error("dcnr_cosine_topk_within: unsupported k=%d d=%d N=%lld n_set_rows=%lld Q=%lld G=%lld "
              "(k<=64, d%%4==0, 4<=d<=256, the rest below 2^31)", k, d, (long long)N, (long long)n_set_rows,
              (long long)Q, (long long)G);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (Q == 0 || G == 0) return DCNR_OK;   // (no query, or none in a segment: nothing is written)
  if (ws_bytes < cosine_topk_within_ws(Q, k, d, max_set_rows)) {
    set_error("dcnr_cosine_topk_within: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  hipStream_t s = (hipStream_t)stream;
  // (bytes: the longest set once per window of 8 queries)
  ProfScope ps(DCNR_K_KNN, s, (double)((Q + 7) / 8) * (double)max_set_rows * (4.0 * d + 12.0));
  const WithinWs w = carve_within(ws, Q, k, d, max_set_rows);
  if (ws_bytes < w.total) {
    set_error("cosine_topk_within: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  const int64_t qblocks = cdiv(Q, 4), windows = cdiv(Q, W_BQ);
  if (qblocks + cdiv(G, 4) > INT32_MAX || windows * w.nchunks > INT32_MAX) {
    set_error("cosine_topk_within: Q=%lld, G=%lld need more blocks than a launch holds", (long long)Q,
              (long long)G);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  hipLaunchKernelGGL(within_prep_kernel, dim3((unsigned)(qblocks + cdiv(G, 4))), dim3(256), 0, s, queries, Q, d,
                     use_v2(d, k) ? 1 : 0, w.qn, seg_offsets, G, seg_set, set_offsets, S, n_set_rows,
                     max_set_rows, qblocks, w.recs, seg_status);
  DCNR_LAUNCH_CHECK();
  if (max_set_rows > 0) {   // (else every set is empty or too long: nothing to scan)
    const dim3 grid((unsigned)(windows * w.nchunks));
    if (use_v2(d, k)) {
      with_dv(d / 4, [&](auto dv) {
        hipLaunchKernelGGL(within_scan_kernel<decltype(dv)::value>, grid, dim3(K2_NT), 0, s, table, inv_norms, N,
                           w.qn, Q, exclude, seg_offsets, G, set_rows, w.recs, w.rpi, w.nchunks, k, w.lists,
                           seg_status);
      });
    } else if (d <= 64) {
      hipLaunchKernelGGL(within_scan_wide_kernel<16>, grid, dim3(NT), 0, s, table, inv_norms, N, d, w.qn, Q,
                         exclude, seg_offsets, G, set_rows, w.recs, w.rpi, w.nchunks, k, w.lists, seg_status);
    } else {
      hipLaunchKernelGGL(within_scan_wide_kernel<64>, grid, dim3(NT), 0, s, table, inv_norms, N, d, w.qn, Q,
                         exclude, seg_offsets, G, set_rows, w.recs, w.rpi, w.nchunks, k, w.lists, seg_status);
    }
    DCNR_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(within_merge_kernel, dim3((unsigned)Q), dim3(NT), 0, s, w.lists, w.nchunks, w.rpi, k, ld, idx,
                     dist, seg_offsets, G, w.recs);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

size_t dcnr_cosine_neighbor_table_workspace_size(int64_t N, int32_t k) {
  if (N < 1 || N > INT32_MAX || k < 1 || k > KMAX || k > N) return 256;   // (the build rejects these)
  return neighbor_table_ws(N, k);   // (exact: one byte less is DCNR_WORKSPACE_TOO_SMALL)
}

dcnr_status dcnr_cosine_neighbor_table(const float* table, const float* inv_norms, const uint16_t* packed,
                                       int64_t N, int32_t d, int32_t k, int64_t row_lo, int64_t row_hi,
                                       int32_t* out_idx, float* out_dist, void* ws, size_t ws_bytes,
                                       dcnr_stream_t stream) {
  if (!table || !inv_norms || N < 1 || row_lo < 0 || row_lo > row_hi || row_hi > N || k < 1 || k > N) {
    set_error("dcnr_cosine_neighbor_table: bad argument (N=%lld, k=%d, rows [%lld, %lld))", (long long)N, k,
              (long long)row_lo, (long long)row_hi);
    return DCNR_BAD_ARG;
  }
  if (N > INT32_MAX || k > KMAX) {
    set_error("dcnr_cosine_neighbor_table: N=%lld (below 2^31), k=%d (max 64)", (long long)N, k);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (row_lo == row_hi) return DCNR_OK;
  if (!out_idx || !ws) {
    set_error("dcnr_cosine_neighbor_table: null argument");
    return DCNR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  // (bytes: one pass over the table and the result; every chunk of queries streams the table again)
  ProfScope ps(DCNR_K_KNN, s, (double)N * (4.0 * d + 4.0) + (double)(row_hi - row_lo) * k * 8.0);
  const bf16* tb = (const bf16*)packed;
  const NbrWs w = carve_nbr(ws, N, k);
  if (ws_bytes < w.total) {
    set_error("neighbor_table: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  for (int64_t lo = row_lo; lo < row_hi; lo += NBR_CHUNK) {
    const int64_t Q = std::min(NBR_CHUNK, row_hi - lo);
    const int64_t o = (lo - row_lo) * k;
    TRY(cosine_topk(table, inv_norms, tb, N, d, table + lo * d, Q, k, w.idx, out_dist ? out_dist + o : w.dist,
                    w.topk, w.topk_bytes, s, /*allow_v3=*/false));
    hipLaunchKernelGGL(narrow_idx_kernel, dim3((unsigned)cdiv(Q * k, 256)), dim3(256), 0, s, w.idx, Q * k,
                       out_idx + o);
    DCNR_LAUNCH_CHECK();
  }
  return DCNR_OK;
}

// the shapes both update calls take: dcnr_cosine_neighbor_table's, and a width
// the search takes (cosine_topk rejects the others only once it runs)
static dcnr_status nbr_update_shape(const char* what, int64_t N, int32_t d, int32_t k) {
  if (N < 1 || k < 1 || k > N) {
    set_error("%s: bad argument (N=%lld, k=%d)", what, (long long)N, k);
    return DCNR_BAD_ARG;
  }
  if (N > INT32_MAX || k > KMAX || d < 4 || d % 4 || d > UPD_DMAX) {
    set_error("%s: N=%lld (below 2^31), k=%d (max 64), d=%d (d %% 4 == 0, 4 <= d <= 256)", what, (long long)N, k,
              d);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  return DCNR_OK;
}

size_t dcnr_cosine_neighbor_table_update_workspace_size(int64_t N, int32_t d, int32_t k, int64_t m) {
  if (nbr_update_shape("dcnr_cosine_neighbor_table_update", N, d, k) != DCNR_OK || m < 0 ||
      m > UPD_MAX_M)
    return 256;   // (the calls reject these)
  return neighbor_table_update_ws(N, d, k, m);   // (exact: one byte less is DCNR_WORKSPACE_TOO_SMALL)
}

// dcnr_cosine_neighbor_table_update and _affected: the checks (the messages
// name the entry, `what`), phase A -- C's bitmap, the rows' exact k-th
// distances, the filter's superset of the rows a changed row may enter --, then
// the merge into `merge_nbr` or, without one, the affected rows to the
// re-search list; the count words to the caller's mirror.
static dcnr_status nbr_update_call(const char* what, const float* table, const float* inv_norms,
                                   const uint16_t* packed, int64_t N, int32_t d, int32_t k, const int32_t* changed,
                                   int64_t m, const int32_t* nbr, int32_t* merge_nbr, int32_t* counts,
                                   int32_t* host_counts, int32_t* research_rows, void* ws, size_t ws_bytes,
                                   hipStream_t s) {
  if (!table || !inv_norms || m < 0) {
    set_error("%s: bad argument (m=%lld)", what, (long long)m);
    return DCNR_BAD_ARG;
  }
  TRY(nbr_update_shape(what, N, d, k));
  if (m > UPD_MAX_M) {
    set_error("%s: m=%lld changed rows (max %d per call)", what, (long long)m, UPD_MAX_M);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (m == 0) return DCNR_OK;
  if (!changed || !nbr || !counts || !research_rows || !ws) {
    set_error("%s: null argument", what);
    return DCNR_BAD_ARG;
  }
  for (int64_t i = 0; i < m; ++i)
    if (changed[i] < 0 || changed[i] >= N || (i > 0 && changed[i] <= changed[i - 1])) {
      set_error("%s: changed[%lld] = %d (ascending, distinct, inside [0, %lld))", what, (long long)i, changed[i],
                (long long)N);
      return DCNR_BAD_ARG;
    }
  // (bytes: the lists, each row's k-th neighbour gathered, one pass over the rows, the changed rows)
  ProfScope ps(DCNR_K_KNN, s,
               (double)N * (4.0 * k + 8.0 + 4.0 * d) +
                   (double)N * d * ((d == 32 || d == 64) && packed ? 2.0 : 4.0) + (double)m * (4.0 * d + 8.0));
  const bf16* tb = (const bf16*)packed;
  const UpdWs w = carve_upd(ws, N, d, k, m);
  if (ws_bytes < std::max(w.ab_total, w.c_total)) {
    set_error("%s: workspace too small", what + sizeof("dcnr_cosine_") - 1);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  DCNR_HIP(hipMemcpyAsync(w.chg, changed, (size_t)m * 4, hipMemcpyHostToDevice, s));
  DCNR_HIP(hipMemsetAsync(w.bits, 0, (size_t)cdiv(N, 32) * 4, s));
  hipLaunchKernelGGL(upd_mark_kernel, dim3((unsigned)cdiv(m, 256)), dim3(256), 0, s, w.chg, (int)m, w.bits,
                     research_rows, counts);
  DCNR_LAUNCH_CHECK();
  const unsigned rb = (unsigned)cdiv(N, 256);
  hipLaunchKernelGGL(upd_kth_kernel, dim3(rb), dim3(256), 0, s, table, inv_norms, (int)N, d / 4, k, nbr, w.bits,
                     w.kth, w.aff, counts);
  DCNR_LAUNCH_CHECK();
  if (d == 32 || d == 64) {
    with_v4_rows(d, tb != nullptr, [&](auto ks, auto pk) {
      hipLaunchKernelGGL((upd_filter4_kernel<decltype(ks)::value, decltype(pk)::value>),
                         dim3((unsigned)cdiv(N, UPD_RPB)), dim3(256), 0, s, table, inv_norms, tb, (int)N, w.chg,
                         (int)m, w.kth, w.aff, counts);
    });
  } else {
    hipLaunchKernelGGL(upd_filter_exact_kernel, dim3(rb), dim3(256), 0, s, table, inv_norms, (int)N, d / 4, w.chg,
                       (int)m, w.kth, w.aff, counts);
  }
  DCNR_LAUNCH_CHECK();
  if (merge_nbr) {
    const unsigned mb = (unsigned)std::min<int64_t>(cdiv(N, UPD_G), 4096);
    hipLaunchKernelGGL(upd_merge_kernel, dim3(mb), dim3(NT), 0, s, table, inv_norms, (int)N, d, k, w.chg, (int)m,
                       w.bits, w.aff, merge_nbr, research_rows, counts);
    DCNR_LAUNCH_CHECK();
  } else {   // (at most N - m affected rows behind the m changed rows)
    hipLaunchKernelGGL(upd_list_kernel, dim3((unsigned)std::min<int64_t>(cdiv(N, 256), 4096)), dim3(256), 0, s,
                       (const int*)w.aff, (int)m, research_rows, counts);
    DCNR_LAUNCH_CHECK();
    hipLaunchKernelGGL(upd_list_counts_kernel, dim3(1), dim3(64), 0, s, counts);
    DCNR_LAUNCH_CHECK();
  }
  if (host_counts) TRY(mirror_words(counts, 4, host_counts, s));
  return DCNR_OK;
}

dcnr_status dcnr_cosine_neighbor_table_update(const float* table, const float* inv_norms, const uint16_t* packed,
                                              int64_t N, int32_t d, int32_t k, const int32_t* changed, int64_t m,
                                              int32_t* nbr, int32_t* counts, int32_t* host_counts,
                                              int32_t* research_rows, void* ws, size_t ws_bytes,
                                              dcnr_stream_t stream) {
  return nbr_update_call("dcnr_cosine_neighbor_table_update", table, inv_norms, packed, N, d, k, changed, m, nbr,
                         nbr, counts, host_counts, research_rows, ws, ws_bytes, (hipStream_t)stream);
}

dcnr_status dcnr_cosine_neighbor_table_affected(const float* table, const float* inv_norms, const uint16_t* packed,
                                                int64_t N, int32_t d, int32_t k, const int32_t* changed, int64_t m,
                                                const int32_t* nbr, int32_t* counts, int32_t* host_counts,
                                                int32_t* research_rows, void* ws, size_t ws_bytes,
                                                dcnr_stream_t stream) {
  // no merge: every affected row is searched again
  return nbr_update_call("dcnr_cosine_neighbor_table_affected", table, inv_norms, packed, N, d, k, changed, m, nbr,
                         nullptr, counts, host_counts, research_rows, ws, ws_bytes, (hipStream_t)stream);
}

dcnr_status dcnr_cosine_neighbor_table_rows(const float* table, const float* inv_norms, const uint16_t* packed,
                                            int64_t N, int32_t d, int32_t k, const int32_t* rows, int64_t n,
                                            int32_t* nbr, void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  if (!table || !inv_norms || n < 0) {
    set_error("dcnr_cosine_neighbor_table_rows: bad argument (n=%lld)", (long long)n);
    return DCNR_BAD_ARG;
  }
  TRY(nbr_update_shape("dcnr_cosine_neighbor_table_rows", N, d, k));
  if (n == 0) return DCNR_OK;
  if (!rows || !nbr || !ws) {
    set_error("dcnr_cosine_neighbor_table_rows: null argument");
    return DCNR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  // (bytes: as the build's -- every chunk of queries streams the table again)
  ProfScope ps(DCNR_K_KNN, s, (double)N * (4.0 * d + 4.0) + (double)n * (4.0 * d + 12.0 * k + 4.0));
  const bf16* tb = (const bf16*)packed;
  const UpdWs w = carve_upd(ws, N, d, k, 0);
  if (ws_bytes < w.c_total) {
    set_error("neighbor_table_rows: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  for (int64_t lo = 0; lo < n; lo += NBR_CHUNK) {
    const int64_t Q = std::min(NBR_CHUNK, n - lo);
    hipLaunchKernelGGL(upd_gather_kernel, dim3((unsigned)cdiv(Q * d, 256)), dim3(256), 0, s, table, (int)N, d,
                       rows + lo, Q, w.q);
    DCNR_LAUNCH_CHECK();
    TRY(cosine_topk(table, inv_norms, tb, N, d, w.q, Q, k, w.nbr.idx, w.nbr.dist, w.nbr.topk, w.nbr.topk_bytes, s,
                    /*allow_v3=*/false));
    hipLaunchKernelGGL(upd_scatter_kernel, dim3((unsigned)cdiv(Q * k, 256)), dim3(256), 0, s, w.nbr.idx, Q, k, (int)N,
                       rows + lo, nbr);
    DCNR_LAUNCH_CHECK();
  }
  return DCNR_OK;
}

dcnr_status dcnr_topk_merge(const float* dist, const int64_t* idx, int32_t lists, int64_t Q,
                            int32_t k, int64_t* out_idx, float* out_dist, dcnr_stream_t stream) {
  if (!dist || !idx || !out_idx || !out_dist || Q < 0) {
    set_error("dcnr_topk_merge: bad argument");
    return DCNR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(DCNR_K_KNN, s, (double)lists * Q * k * 12.0 + Q * k * 12.0);
  if (k < 1 || lists < 1 || (int64_t)lists * k > TM_CAP) {
    set_error("topk_merge: %d lists of k=%d unsupported (lists * k <= %d)", lists, k, TM_CAP);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (Q <= 0) return DCNR_OK;
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)Q), dim3(NT), 0, s, dist, idx, lists, Q, k,
                     out_idx, out_dist);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // extern "C"
