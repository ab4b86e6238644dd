// The large lane of a batch of /recommendations requests: the requests whose
// bound `need` = positives * k + fallback rows exceeds SV_MAX, which the
// one-workgroup-per-request kernels of serving.hip report as overflow.  Here
// all L of them are processed together, every step with a grid over their
// entries, so there is no capacity but the workspace:
//
//   candidates   one 64-bit key (lane, row, from-fallback bit) per staged entry
//                -> stable radix sort over the key bits in use -> the head of
//                every (lane, row) run is a distinct row -> fallback rule and
//                allowed / excluded filters as flags -> tiled scan -> the
//                surviving rows ascending per request, compact
//   ranking batch  over the compact rows, the user of lane l's request
//   rank         radix sort of (lane, order-preserving bits of -logit) records
//                (stable: ties keep their position, as rank_sort's do)
//   MMR          one workgroup per request.  Up to SV_MAX candidates exactly
//                req_rank_mmr_kernel's choice of form (mmr_lds where the rows
//                fit LDS, else mmr_table with its scratch in LDS), so that a
//                segment both lanes take gets the same bits; above, mmr_table
//                with maxsim / taken in the workspace: the same arithmetic in
//                the same order, hence the same picks
//
// Lane l serves request large_req[l] of the call's R requests: its positives,
// its set indices and its user are read at that index of the batch's arrays.
#include "device_prims.h"
#include "serving_blocks.h"

namespace dcnr {
namespace {

using namespace rsort;
using tscan::scan_inplace;
using tscan::scan_tiles;

constexpr int LG_NT = 256;
constexpr int64_t LG_MAX_ENTRIES = int64_t(1) << 30;   // sort positions are 32-bit
constexpr int64_t LG_MAX_LANES = int64_t(1) << 22;
constexpr int64_t LG_MAX_ITEMS = int64_t(1) << 38;     // lane + row + 2 bits in 64

inline int ceil_log2(int64_t n) {
  int b = 0;
  while ((int64_t(1) << b) < n) ++b;
  return b;
}

// key = lane << (rb + 1) | row << 1 | from_fallback; a skipped entry (a row
// < 0, an entry of a rejected lane) is the one bit above them: it sorts last
struct KeyBits {
  int rb, lb;
  __host__ __device__ uint64_t skip() const { return uint64_t(1) << (rb + 1 + lb); }
  __host__ __device__ int total() const { return rb + lb + 2; }
};
inline KeyBits key_bits(int64_t n_items, int64_t L) {
  return KeyBits{std::max(1, ceil_log2(n_items)), ceil_log2(L)};
}

struct SortPlan { int units; int64_t chunk; };
inline SortPlan sort_plan(int64_t n) {
  SortPlan p;
  p.units = (int)std::min<int64_t>(MAX_UNITS, std::max<int64_t>(1, cdiv(n, UNIT_KEYS)));
  p.chunk = rup(cdiv(n, p.units), WAVE);
  return p;
}

// what lane_kernel found of a lane: ok, the positives' first index, the staged
// entries that come from positives (their number * k) and the three sets
struct LaneInfo {
  int32_t ok;
  int64_t q0, n_pos;
  const int64_t *arows, *erows, *frows;
  int64_t alen, elen, flen;   // -1: none
};

// the last lane l < L with off[l] <= e (off ascending, off[0] <= e)
__device__ __forceinline__ int64_t lane_of(const int64_t* off, int64_t L, int64_t e) {
  int64_t lo = 0, hi = L - 1;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (off[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Lane l's request, offsets and sets checked against the lengths passed by
// value -> info[l], status[l] = 0 or REQ_BAD_DATA.  stage_off must split
// [0, n_staged) into the lanes' bounds exactly; a lane's bound must be its
// positives * k + its fallback set's rows.  Offsets that are not such a
// partition set *off_bad: no entry can then be told to a lane, and every lane
// is rejected.
__global__ __launch_bounds__(LG_NT) void lane_kernel(const int32_t* large_req,
                                                     const int64_t* stage_off, int64_t L,
                                                     int64_t n_staged, const int64_t* pos_off,
                                                     int64_t R, int64_t Q_total, int k, ReqSets st,
                                                     int64_t n_items, LaneInfo* info,
                                                     int32_t* status, int32_t* off_bad) {
  const int64_t l = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (l >= L) return;
  LaneInfo li = {};
  const int64_t s0 = stage_off[l], s1 = stage_off[l + 1];
  if (s0 < 0 || s1 < s0 || s1 > n_staged || (l == 0 && s0 != 0) || (l == L - 1 && s1 != n_staged))
    atomicOr(off_bad, 1);
  const int64_t r = large_req[l];
  bool ok = r >= 0 && r < R;
  if (ok) {
    const int64_t q0 = pos_off[r], q1 = pos_off[r + 1];
    const bool a_ok = req_set(st, st.allowed, r, li.arows, li.alen);
    const bool e_ok = req_set(st, st.excluded, r, li.erows, li.elen);
    const bool f_ok = req_set(st, st.fallback, r, li.frows, li.flen);
    ok = q0 >= 0 && q1 >= q0 && q1 <= Q_total && a_ok && e_ok && f_ok;
    // ascending sets: the ends bound every row of a filter set
    if (ok && ((li.alen > 0 && (li.arows[0] < 0 || li.arows[li.alen - 1] >= n_items)) ||
               (li.elen > 0 && (li.erows[0] < 0 || li.erows[li.elen - 1] >= n_items))))
      ok = false;
    if (ok) {
      li.q0 = q0;
      li.n_pos = (q1 - q0) * k;
      ok = li.n_pos + (li.flen > 0 ? li.flen : 0) == s1 - s0;
    }
  }
  li.ok = ok;
  info[l] = li;
  status[l] = ok ? 0 : REQ_BAD_DATA;
}

// keys[e] of staged entry e: entry t = e - stage_off[l] of its lane is staged
// entry t of the request (union_entry) below n_pos, row t - n_pos of the
// fallback set from there on.  A row >= n_items (a fallback row < 0) rejects
// the lane (an OR into its status: a flag, no position depends on it).
template <class Src>
__global__ __launch_bounds__(LG_NT) void stage_kernel(const int64_t* pos, Src src, int k,
                                                      const int64_t* stage_off, int64_t L,
                                                      int64_t n_staged, const LaneInfo* info,
                                                      int64_t n_items, KeyBits kb,
                                                      const int32_t* off_bad, int32_t* status,
                                                      uint64_t* keys) {
  const int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (e >= n_staged) return;
  uint64_t key = kb.skip();
  if (!*off_bad) {
    const int64_t l = lane_of(stage_off, L, e);
    const int64_t t = e - stage_off[l];
    const LaneInfo li = info[l];
    const int64_t fl = li.flen > 0 ? li.flen : 0;
    if (li.ok && t >= 0 && t < li.n_pos + fl) {
      bool b = false;
      int64_t v;
      if (t < li.n_pos) {
        v = union_entry(pos + li.q0, src.from(li.q0), k, (int)t, b);
      } else {
        v = li.frows[t - li.n_pos];
        if (v < 0) b = true;
      }
      if (b || (v != INT64_MAX && v >= n_items)) atomicOr(&status[l], REQ_BAD_DATA);
      else if (v != INT64_MAX)
        key = ((uint64_t)l << (kb.rb + 1)) | ((uint64_t)v << 1) | (uint64_t)(t >= li.n_pos);
    }
  }
  keys[e] = key;
}

// lane_lo[l], l <= L: the first sorted position whose key is not below lane l's
// first key (lane_lo[L]: where the skipped entries begin)
__global__ __launch_bounds__(LG_NT) void lane_bounds_kernel(const uint64_t* keys, int64_t n,
                                                            int64_t L, KeyBits kb,
                                                            int64_t* lane_lo) {
  const int64_t l = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (l > L) return;
  const uint64_t v = l == L ? kb.skip() : (uint64_t)l << (kb.rb + 1);
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  lane_lo[l] = lo;
}

// is sorted position e the head of its (lane, row) run?
__device__ __forceinline__ bool run_head(const uint64_t* keys, int64_t e, uint64_t key, KeyBits kb) {
  return key < kb.skip() && (e == 0 || (keys[e - 1] >> 1) != (key >> 1));
}

// f[e] = 1 where e heads a run that a positive or a neighbour takes part in
// (within a run the entries that are not from the fallback sort first)
__global__ __launch_bounds__(LG_NT) void union_flag_kernel(const uint64_t* keys, int64_t n, KeyBits kb,
                                                           uint32_t* f) {
  const int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (e >= n) return;
  const uint64_t key = keys[e];
  f[e] = run_head(keys, e, key, kb) && !(key & 1);
}

// the flags' sum over sorted positions [a, b) from their inclusive scan
__device__ __forceinline__ uint32_t scan_range(const uint32_t* inc, int64_t a, int64_t b) {
  return b > a ? inc[b - 1] - (a ? inc[a - 1] : 0u) : 0u;
}

// f[e] = 1 where the row at the head e survives: its lane was not rejected; a
// head the fallback alone brought is kept iff the lane's union (u_inc: the
// inclusive scan of union_flag_kernel's flags) has fewer than min_cand rows
// (main.py:204-207); then the allowed / excluded filters
__global__ __launch_bounds__(LG_NT) void keep_flag_kernel(const uint64_t* keys, int64_t n, KeyBits kb,
                                                          const LaneInfo* info, const int32_t* status,
                                                          const int64_t* lane_lo, const uint32_t* u_inc,
                                                          int min_cand, uint32_t* f) {
  const int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (e >= n) return;
  const uint64_t key = keys[e];
  bool keep = run_head(keys, e, key, kb);
  if (keep) {
    const int64_t l = (int64_t)(key >> (kb.rb + 1));
    const int64_t v = (int64_t)((key >> 1) & ((uint64_t(1) << kb.rb) - 1));
    const LaneInfo li = info[l];
    keep = status[l] == 0;
    if (keep && (key & 1))
      keep = (int64_t)scan_range(u_inc, lane_lo[l], lane_lo[l + 1]) < (int64_t)min_cand;
    keep = keep && (li.alen < 0 || set_contains(li.arows, li.alen, v)) &&
           !(li.elen > 0 && set_contains(li.erows, li.elen, v));
  }
  f[e] = keep;
}

// the surviving rows to their places: the number of survivors before them
// (k_inc: the inclusive scan of keep_flag_kernel's flags).  Sorted by (lane,
// row), so every request's rows stand together, ascending.
__global__ __launch_bounds__(LG_NT) void compact_kernel(const uint64_t* keys, int64_t n, KeyBits kb,
                                                        const uint32_t* k_inc, int64_t* out) {
  const int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (e >= n) return;
  const uint32_t here = k_inc[e], before = e ? k_inc[e - 1] : 0u;
  if (here != before) out[before] = (int64_t)((keys[e] >> 1) & ((uint64_t(1) << kb.rb) - 1));
}

// offsets [L + 1], out_count [L] and the final status [L] (every lane rejected
// when the staged offsets were no partition), mirrored to pinned host memory
// with system-scope stores as req_offsets_kernel mirrors the small lane's
__global__ __launch_bounds__(LG_NT) void lane_out_kernel(const uint32_t* k_inc, int64_t n,
                                                         const int64_t* lane_lo, int64_t L,
                                                         const int32_t* off_bad, int32_t* status,
                                                         int64_t* offsets, int32_t* out_count,
                                                         int64_t* host_off, int32_t* host_status) {
  const int64_t l = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (l > L) return;
  const int64_t a = lane_lo[l];
  const int64_t before = n == 0 || a == 0 ? 0 : (int64_t)k_inc[a - 1];
  offsets[l] = before;
  if (host_off) __hip_atomic_store(host_off + l, before, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (l == L) return;
  const int32_t stt = *off_bad ? (int32_t)REQ_BAD_DATA : status[l];
  status[l] = stt;
  out_count[l] = (int32_t)scan_range(k_inc, a, lane_lo[l + 1]);
  if (host_status) __hip_atomic_store(host_status + l, stt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// a call whose lanes stage nothing: every offset and count 0, the lanes' status
__global__ __launch_bounds__(LG_NT) void lane_empty_kernel(int64_t L, const int32_t* off_bad,
                                                           int32_t* status, int64_t* offsets,
                                                           int32_t* out_count, int64_t* host_off,
                                                           int32_t* host_status) {
  const int64_t l = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (l > L) return;
  offsets[l] = 0;
  if (host_off) __hip_atomic_store(host_off + l, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (l == L) return;
  const int32_t stt = *off_bad ? (int32_t)REQ_BAD_DATA : status[l];
  status[l] = stt;
  out_count[l] = 0;
  if (host_status) __hip_atomic_store(host_status + l, stt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct CandWs {
  uint64_t *ka, *kb;       // [n] key ping-pong
  uint32_t *counts, *tot;  // the sort's [units][NB], [NB]
  uint32_t *fu, *fk;       // [n] union flags, keep flags -> their scans
  uint32_t* tile_tot;
  LaneInfo* info;          // [L]
  int64_t* lane_lo;        // [L + 1]
  int32_t* off_bad;        // [1]
  size_t total;
};
CandWs cand_carve(int64_t L, int64_t n, void* base) {
  Bump b(base);
  CandWs w;
  const SortPlan p = sort_plan(n);
  w.ka = (uint64_t*)b.take((size_t)n * 8);
  w.kb = (uint64_t*)b.take((size_t)n * 8);
  w.counts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.tot = (uint32_t*)b.take((size_t)NB * 4);
  w.fu = (uint32_t*)b.take((size_t)n * 4);
  w.fk = (uint32_t*)b.take((size_t)n * 4);
  w.tile_tot = (uint32_t*)b.take((size_t)scan_tiles(n) * 4);
  w.info = (LaneInfo*)b.take((size_t)L * sizeof(LaneInfo));
  w.lane_lo = (int64_t*)b.take((size_t)(L + 1) * 8);
  w.off_bad = (int32_t*)b.take(4);
  w.total = b.off;
  return w;
}

inline unsigned blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, cdiv(n, LG_NT)); }

// ---- ranking batch over the compact rows
__global__ void large_batch_kernel(const int64_t* rows, const int64_t* offsets, int64_t L, int64_t n,
                                   const int32_t* large_req, int64_t R, const int64_t* user_rows,
                                   const int64_t* item_cat, int K, const float* item_num, int F,
                                   int64_t n_items, int64_t* user_out, int64_t* item_out,
                                   int64_t* cat_out, float* num_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  if (i >= n) return;
  const int64_t l = lane_of(offsets, L, i);
  int64_t r = large_req[l];
  r = r < 0 ? 0 : (r >= R ? R - 1 : r);   // (clamped, as batch_row clamps the item)
  batch_row(i, rows[i], user_rows[r], item_cat, K, item_num, F, n_items, user_out, item_out, cat_out,
            num_out);
}

// ---- rank + MMR
// a record of the rank sort: key = lane << 32 | order-preserving bits of
// -logit, pos = the candidate's place in the batch
struct RankRec { uint64_t key; uint32_t pos; uint32_t pad; };
__device__ __forceinline__ uint32_t radix_digit(const RankRec& r, int shift) {
  return (uint32_t)((r.key >> shift) & (NB - 1));
}

// ascending on -z as rank_sort's float compare orders it: the sign flipped in
// the bits, -0.0 as +0.0, then the usual order-preserving map
__device__ __forceinline__ uint32_t rank_bits(float z) {
  uint32_t u = __float_as_uint(z) ^ 0x80000000u;
  if (u == 0x80000000u) u = 0u;
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// the lanes' segments checked: offsets must rise from 0 within [0, n] (else
// *off_bad: every lane is rejected), lambda < 1 needs top_k >= 1
__global__ __launch_bounds__(LG_NT) void rank_lane_kernel(const int64_t* offsets, int64_t L, int64_t n,
                                                          const float* lambda, const int32_t* top_k,
                                                          int32_t* status, int32_t* off_bad) {
  const int64_t l = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (l >= L) return;
  const int64_t o0 = offsets[l], o1 = offsets[l + 1];
  if (o0 < 0 || o1 < o0 || o1 > n || (l == 0 && o0 != 0)) atomicOr(off_bad, 1);
  if (lambda[l] < 1.f && top_k[l] < 1) atomicOr(&status[l], REQ_BAD_DATA);
}

// rec[i] of candidate i (lane L for one behind the last segment: it sorts
// last); a logit without a rank (-inf, NaN) rejects its lane
__global__ __launch_bounds__(LG_NT) void rank_stage_kernel(const float* logits, int64_t n,
                                                           const int64_t* offsets, int64_t L,
                                                           const int32_t* off_bad, int32_t* status,
                                                           RankRec* rec) {
  const int64_t i = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (i >= n) return;
  RankRec r = {(uint64_t)L << 32, (uint32_t)i, 0u};
  if (!*off_bad) {
    const int64_t l = lane_of(offsets, L, i);
    if (i >= offsets[l] && i < offsets[l + 1]) {
      const float z = logits[i];
      if (!(z >= -FLT_MAX)) atomicOr(&status[l], REQ_BAD_DATA);
      r.key = ((uint64_t)l << 32) | rank_bits(z);
    }
  }
  rec[i] = r;
}

// the sorted records to the ranked lists: place e of the sorted batch is place
// e of the segments (the lanes rise with the positions, and the sort keeps a
// lane's records in its segment).  lambda >= 1: the answer itself (out_rows /
// out_logits); else the list the MMR reads (rrows / rscores), where a row >=
// n_items rejects the lane
__global__ __launch_bounds__(LG_NT) void rank_emit_kernel(const RankRec* rec, int64_t n, int64_t L,
                                                          const int32_t* off_bad, const float* logits,
                                                          const int64_t* rows, int64_t n_items,
                                                          const float* lambda, int32_t* status,
                                                          int64_t* rrows, float* rscores,
                                                          int64_t* out_rows, float* out_logits) {
  const int64_t e = (int64_t)blockIdx.x * LG_NT + threadIdx.x;
  if (e >= n || *off_bad) return;
  const RankRec r = rec[e];
  const int64_t l = (int64_t)(r.key >> 32);
  if (l >= L || r.pos >= n) return;
  const int64_t row = rows[r.pos];
  const float z = logits[r.pos];
  if (lambda[l] < 1.f) {
    if (row >= n_items) atomicOr(&status[l], REQ_BAD_DATA);
    rrows[e] = row;
    rscores[e] = z;
  } else {
    out_rows[e] = row;
    out_logits[e] = z;
  }
}

// Lane l = blockIdx.x after the rank: a rejected lane's whole segment marked
// (rows -1, logits NaN) and count 0, as req_rank_mmr_kernel does; lambda >= 1:
// the count; else the greedy MMR over the ranked list: up to SV_MAX candidates
// in the form req_rank_mmr_kernel takes for that length (dynamic LDS of
// MMR_LDS_MAX bytes, carved as there), above with maxsim / taken in the
// workspace (g_maxsim / g_taken [n], the segment's part)
__global__ __launch_bounds__(SV_NT) void large_mmr_kernel(
    const int64_t* offsets, int64_t L, int64_t n_total, const int32_t* off_bad, const float* table,
    const float* inv, int d, const float* lambda, const int32_t* top_k, const int64_t* rrows,
    const float* rscores, float* g_maxsim, unsigned char* g_taken, int64_t* out_rows,
    float* out_logits, int32_t* out_count, int32_t* status) {
  __shared__ unsigned char flags[SV_MAX];   // vld (LDS form) / taken (table form)
  extern __shared__ float dyn[];
  const int64_t l = blockIdx.x;
  if (l >= L) return;
  // (everything that decides an exit below is uniform over the workgroup)
  if (*off_bad) {
    if (threadIdx.x == 0) { out_count[l] = 0; status[l] |= REQ_BAD_DATA; }
    return;
  }
  const int64_t o0 = offsets[l], o1 = offsets[l + 1];   // inside [0, n_total]: rank_lane_kernel
  const int n = (int)(o1 - o0);
  if (status[l] & REQ_BAD_DATA) {
    for (int t = threadIdx.x; t < n; t += SV_NT) {
      out_rows[o0 + t] = -1;
      out_logits[o0 + t] = __int_as_float(0x7fc00000);
    }
    if (threadIdx.x == 0) out_count[l] = 0;
    return;
  }
  const float lam = lambda[l];
  if (n == 0 || !(lam < 1.f)) {
    if (threadIdx.x == 0) out_count[l] = n;
    return;
  }
  const int64_t* rr = rrows + o0;
  const float* rs = rscores + o0;
  const int tk = top_k[l];
  auto emit = [&](int i, int p) { out_rows[o0 + i] = rr[p]; out_logits[o0 + i] = rs[p]; };
  int cnt;
  if (n > SV_MAX)
    cnt = mmr_table(table, inv, d, rr, rs, n, lam, tk, g_maxsim + o0, g_taken + o0, dyn, emit);
  else if (mmr_lds_bytes(n, d) <= MMR_LDS_MAX)
    cnt = mmr_lds(table, inv, d, rr, rs, n, lam, tk, dyn, flags, emit);
  else
    cnt = mmr_table(table, inv, d, rr, rs, n, lam, tk, dyn, flags, dyn + SV_MAX, emit);
  if (threadIdx.x == 0) out_count[l] = cnt;
}

struct RankWs {
  RankRec *ra, *rb;        // [n] record ping-pong
  uint32_t *counts, *tot;
  int64_t* rrows;          // [n] the ranked lists the MMR reads
  float* rscores;
  float* maxsim;           // [n]
  unsigned char* taken;    // [n]
  int32_t* off_bad;
  size_t total;
};
RankWs rank_carve(int64_t n, void* base) {
  Bump b(base);
  RankWs w;
  const SortPlan p = sort_plan(n);
  w.ra = (RankRec*)b.take((size_t)n * sizeof(RankRec));
  w.rb = (RankRec*)b.take((size_t)n * sizeof(RankRec));
  w.counts = (uint32_t*)b.take((size_t)p.units * NB * 4);
  w.tot = (uint32_t*)b.take((size_t)NB * 4);
  w.rrows = (int64_t*)b.take((size_t)n * 8);
  w.rscores = (float*)b.take((size_t)n * 4);
  w.maxsim = (float*)b.take((size_t)n * 4);
  w.taken = (unsigned char*)b.take((size_t)n);
  w.off_bad = (int32_t*)b.take(4);
  w.total = b.off;
  return w;
}

// ---- one request's MMR for any n: mmr_kernel with its scratch in the workspace
__global__ __launch_bounds__(SV_NT) void mmr_large_kernel(const float* table, const float* inv, int d,
                                                          const int64_t* rows, const float* scores,
                                                          int n, float lambda, int top_k,
                                                          float* maxsim, unsigned char* taken,
                                                          int64_t* out_pos, int32_t* out_count) {
  __shared__ float selv[256];
  const int cnt = mmr_table(table, inv, d, rows, scores, n, lambda, top_k, maxsim, taken, selv,
                            [&](int i, int p) { out_pos[i] = p; });
  for (int t = threadIdx.x + cnt; t < top_k; t += SV_NT) out_pos[t] = -1;
  if (threadIdx.x == 0) *out_count = cnt;
}

size_t mmr_large_bytes(int64_t n) {
  Bump b(nullptr);
  b.take((size_t)n * 4);
  b.take((size_t)n);
  return b.off + 256;
}

bool large_shape(const char* who, int64_t L, int64_t n, dcnr_status& st) {
  st = DCNR_OK;
  if (L < 0 || n < 0) {
    set_error("%s: L=%lld, n=%lld (>= 0)", who, (long long)L, (long long)n);
    st = DCNR_BAD_ARG;
  } else if (L > LG_MAX_LANES || n > LG_MAX_ENTRIES) {
    set_error("%s: L=%lld exceeds %lld lanes, or n=%lld exceeds %lld entries", who, (long long)L,
              (long long)LG_MAX_LANES, (long long)n, (long long)LG_MAX_ENTRIES);
    st = DCNR_UNSUPPORTED_SHAPE;
  }
  return st == DCNR_OK;
}

}  // namespace
}  // namespace dcnr

using namespace dcnr;

extern "C" {

size_t dcnr_requests_large_workspace_size(int64_t L, int64_t n_staged) {
  if (L <= 0 || L > LG_MAX_LANES || n_staged < 0 || n_staged > LG_MAX_ENTRIES) return 0;
  return std::max(cand_carve(L, n_staged, nullptr).total, rank_carve(n_staged, nullptr).total) + 256;
}

dcnr_status dcnr_requests_large_candidates(
    const int64_t* positives, const int64_t* pos_offsets, int64_t R, int64_t Q_total,
    const int64_t* knn_idx, const int32_t* nbr, int32_t kt, int32_t k, const int64_t* set_rows,
    int64_t n_set_rows, const int64_t* set_offsets, int32_t S, const int32_t* allowed,
    const int32_t* excluded, const int32_t* fallback, int32_t min_candidates, int64_t n_items,
    const int32_t* large_req, const int64_t* stage_offsets, int64_t L, int64_t n_staged,
    int64_t* out_rows, int32_t* out_count, int32_t* status, int64_t* offsets, int64_t* host_offsets,
    int32_t* host_status, void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  const char* who = "dcnr_requests_large_candidates";
  hipStream_t s = (hipStream_t)stream;
  dcnr_status shape;
  if (!large_shape(who, L, n_staged, shape)) return shape;
  if (R < 0 || Q_total < 0 || k < 1 || S < 0 || n_set_rows < 0 || n_items < 1 || (nbr && kt < k)) {
    set_error("%s: R=%lld, Q_total=%lld, k=%d, kt=%d, S=%d, n_set_rows=%lld, n_items=%lld", who,
              (long long)R, (long long)Q_total, k, kt, S, (long long)n_set_rows, (long long)n_items);
    return DCNR_BAD_ARG;
  }
  if (L > 0 && (!pos_offsets || !large_req || !stage_offsets || !out_count || !status || !offsets ||
                !ws || (n_staged > 0 && !out_rows) ||
                (Q_total > 0 && (!positives || (!knn_idx && !nbr))) || (S > 0 && !set_offsets) ||
                (n_set_rows > 0 && !set_rows) || (S == 0 && (allowed || excluded || fallback)))) {
    set_error("%s: null argument (or set indices without sets)", who);
    return DCNR_BAD_ARG;
  }
  if (k > 64 || n_set_rows > INT32_MAX || n_items > LG_MAX_ITEMS) {
    set_error("%s: k=%d (max 64), n_set_rows=%lld (max 2^31 - 1), n_items=%lld (max 2^38)", who, k,
              (long long)n_set_rows, (long long)n_items);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (L == 0) return DCNR_OK;
  const size_t need = cand_carve(L, n_staged, nullptr).total + 256;
  if (ws_bytes < need) {
    set_error("%s: workspace too small: %zu < %zu", who, ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  const CandWs w = cand_carve(L, n_staged, ws_align(ws));
  const KeyBits kb = key_bits(n_items, L);
  const int64_t n = n_staged;
  ProfScope ps(DCNR_K_SERVE, s);
  DCNR_HIP(hipMemsetAsync(w.off_bad, 0, 4, s));
  ReqSets st{set_rows, n_set_rows, set_offsets, S, allowed, excluded, fallback};
  hipLaunchKernelGGL(lane_kernel, dim3(blocks(L)), dim3(LG_NT), 0, s, large_req, stage_offsets, L, n,
                     pos_offsets, R, Q_total, (int)k, st, n_items, w.info, status, w.off_bad);
  DCNR_LAUNCH_CHECK();
  if (n == 0) {
    hipLaunchKernelGGL(lane_empty_kernel, dim3(blocks(L + 1)), dim3(LG_NT), 0, s, L,
                       (const int32_t*)w.off_bad, status, offsets, out_count, host_offsets, host_status);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }
  auto stage = [&](auto src) {
    hipLaunchKernelGGL(stage_kernel<decltype(src)>, dim3(blocks(n)), dim3(LG_NT), 0, s, positives, src,
                       (int)k, stage_offsets, L, n, (const LaneInfo*)w.info, n_items, kb,
                       (const int32_t*)w.off_bad, status, w.ka);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  };
  TRY(nbr ? stage(NbrTable{nbr, kt, n_items}) : stage(KnnLists{knn_idx, k}));
  const SortPlan p = sort_plan(n);
  uint64_t *src = w.ka, *dst = w.kb;
  TRY(sort_passes(src, dst, n, p.units, p.chunk, 0, (int)cdiv(kb.total(), RBITS), w.counts, w.tot,
                  (const uint32_t*)nullptr, s));
  hipLaunchKernelGGL(lane_bounds_kernel, dim3(blocks(L + 1)), dim3(LG_NT), 0, s, (const uint64_t*)src, n,
                     L, kb, w.lane_lo);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(union_flag_kernel, dim3(blocks(n)), dim3(LG_NT), 0, s, (const uint64_t*)src, n, kb,
                     w.fu);
  DCNR_LAUNCH_CHECK();
  TRY(scan_inplace<false>(w.fu, nullptr, n, w.tile_tot, s));
  hipLaunchKernelGGL(keep_flag_kernel, dim3(blocks(n)), dim3(LG_NT), 0, s, (const uint64_t*)src, n, kb,
                     (const LaneInfo*)w.info, (const int32_t*)status, (const int64_t*)w.lane_lo,
                     (const uint32_t*)w.fu, (int)min_candidates, w.fk);
  DCNR_LAUNCH_CHECK();
  TRY(scan_inplace<false>(w.fk, nullptr, n, w.tile_tot, s));
  hipLaunchKernelGGL(compact_kernel, dim3(blocks(n)), dim3(LG_NT), 0, s, (const uint64_t*)src, n, kb,
                     (const uint32_t*)w.fk, out_rows);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(lane_out_kernel, dim3(blocks(L + 1)), dim3(LG_NT), 0, s, (const uint32_t*)w.fk, n,
                     (const int64_t*)w.lane_lo, L, (const int32_t*)w.off_bad, status, offsets, out_count,
                     host_offsets, host_status);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_requests_large_ranking_batch(const int64_t* cand_rows, const int64_t* offsets,
                                              int64_t L, int64_t n, const int32_t* large_req,
                                              int64_t R, const int64_t* user_rows,
                                              const int64_t* item_cat, int32_t n_cat,
                                              const float* item_num, int32_t n_num, int64_t n_items,
                                              int64_t* user_ids, int64_t* item_ids,
                                              int64_t* cat_features, float* num_features,
                                              dcnr_stream_t stream) {
  const char* who = "dcnr_requests_large_ranking_batch";
  hipStream_t s = (hipStream_t)stream;
  dcnr_status shape;
  if (!large_shape(who, L, n, shape)) return shape;
  if (R < 0 || n_items < 1 || n_cat < 0 || n_num < 0 || (n > 0 && (L < 1 || R < 1)) ||
      (n > 0 && (!cand_rows || !offsets || !large_req || !user_rows || !user_ids || !item_ids ||
                 (n_cat && (!item_cat || !cat_features)) || (n_num && (!item_num || !num_features))))) {
    set_error("%s: bad argument (n=%lld rows of L=%lld lanes, R=%lld)", who, (long long)n, (long long)L,
              (long long)R);
    return DCNR_BAD_ARG;
  }
  if (L == 0 || n == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  dim3 blk(16, 16);
  hipLaunchKernelGGL(large_batch_kernel, dim3((unsigned)cdiv(n, 16)), blk, 0, s, cand_rows, offsets, L,
                     n, large_req, R, user_rows, item_cat, n_cat, item_num, n_num, n_items, user_ids,
                     item_ids, cat_features, num_features);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_requests_large_rank_mmr(const float* logits, int64_t n, const int64_t* cand_rows,
                                         const int64_t* offsets, int64_t L, const float* table,
                                         const float* inv_norms, int32_t d, int64_t n_items,
                                         const float* lambda_param, const int32_t* top_k,
                                         int64_t* out_rows, float* out_logits, int32_t* out_count,
                                         int32_t* status, void* ws, size_t ws_bytes,
                                         dcnr_stream_t stream) {
  const char* who = "dcnr_requests_large_rank_mmr";
  hipStream_t s = (hipStream_t)stream;
  dcnr_status shape;
  if (!large_shape(who, L, n, shape)) return shape;
  if (d < 1 || d > 256 || n_items < 1 ||
      (L > 0 && (!offsets || !table || !inv_norms || !lambda_param || !top_k || !out_count || !status ||
                 !ws || (n > 0 && (!logits || !cand_rows || !out_rows || !out_logits))))) {
    set_error("%s: bad argument (d=%d of 1..256, n_items=%lld, or a null pointer)", who, d,
              (long long)n_items);
    return DCNR_BAD_ARG;
  }
  if (L == 0) return DCNR_OK;
  const size_t need = rank_carve(n, nullptr).total + 256;
  if (ws_bytes < need) {
    set_error("%s: workspace too small: %zu < %zu", who, ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  const RankWs w = rank_carve(n, ws_align(ws));
  ProfScope ps(DCNR_K_SERVE, s);
  DCNR_HIP(hipMemsetAsync(w.off_bad, 0, 4, s));
  hipLaunchKernelGGL(rank_lane_kernel, dim3(blocks(L)), dim3(LG_NT), 0, s, offsets, L, n, lambda_param,
                     top_k, status, w.off_bad);
  DCNR_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(rank_stage_kernel, dim3(blocks(n)), dim3(LG_NT), 0, s, logits, n, offsets, L,
                       (const int32_t*)w.off_bad, status, w.ra);
    DCNR_LAUNCH_CHECK();
    const SortPlan p = sort_plan(n);
    RankRec *src = w.ra, *dst = w.rb;
    TRY(sort_passes(src, dst, n, p.units, p.chunk, 0, (int)cdiv(32 + ceil_log2(L + 1), RBITS), w.counts,
                    w.tot, (const uint32_t*)nullptr, s));
    hipLaunchKernelGGL(rank_emit_kernel, dim3(blocks(n)), dim3(LG_NT), 0, s, (const RankRec*)src, n, L,
                       (const int32_t*)w.off_bad, logits, cand_rows, n_items, lambda_param, status,
                       w.rrows, w.rscores, out_rows, out_logits);
    DCNR_LAUNCH_CHECK();
  }
  TRY(set_max_dyn_lds((const void*)large_mmr_kernel, MMR_LDS_MAX));
  hipLaunchKernelGGL(large_mmr_kernel, dim3((unsigned)L), dim3(SV_NT), MMR_LDS_MAX, s, offsets, L, n,
                     (const int32_t*)w.off_bad, table, inv_norms, (int)d, lambda_param, top_k,
                     (const int64_t*)w.rrows, (const float*)w.rscores, w.maxsim, w.taken, out_rows,
                     out_logits, out_count, status);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

size_t dcnr_mmr_rerank_large_workspace_size(int64_t n) {
  if (n <= 0 || n > LG_MAX_ENTRIES) return 0;
  return mmr_large_bytes(n);
}

dcnr_status dcnr_mmr_rerank_large(const float* table, const float* inv_norms, int32_t d,
                                  const int64_t* rows, const float* scores, int64_t n,
                                  float lambda_param, int32_t top_k, int64_t* out_pos,
                                  int32_t* out_count, void* ws, size_t ws_bytes,
                                  dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || top_k < 1 || (n > 0 && (!table || !inv_norms || !rows || !scores || !out_pos ||
                                       !out_count || !ws))) {
    set_error("dcnr_mmr_rerank_large: bad argument");
    return DCNR_BAD_ARG;
  }
  if (n > LG_MAX_ENTRIES || d > 256 || d < 1) {
    set_error("mmr_rerank_large: n=%lld (max %lld), d=%d (max 256)", (long long)n,
              (long long)LG_MAX_ENTRIES, d);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (n == 0) return DCNR_OK;
  const size_t need = mmr_large_bytes(n);
  if (ws_bytes < need) {
    set_error("dcnr_mmr_rerank_large: workspace too small: %zu < %zu", ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  Bump b(ws_align(ws));
  float* maxsim = (float*)b.take((size_t)n * 4);
  unsigned char* taken = (unsigned char*)b.take((size_t)n);
  ProfScope ps(DCNR_K_SERVE, s);
  hipLaunchKernelGGL(mmr_large_kernel, dim3(1), dim3(SV_NT), 0, s, table, inv_norms, (int)d, rows,
                     scores, (int)n, lambda_param, top_k, maxsim, taken, out_pos, out_count);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // extern "C"
