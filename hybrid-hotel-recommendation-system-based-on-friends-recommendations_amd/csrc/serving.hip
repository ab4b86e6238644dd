// The steps either side of scoring in /recommendations (main.py:294-357), on
// the device, for candidate sets of up to SV_MAX items:
//
//   candidate union   _generate_candidates, main.py:196-203: the positive
//                     hotels plus the neighbours the cosine index returns for
//                     each (position 0 dropped), as a set (here: ascending ids)
//   ranking batch     preprocess_for_ranking, main.py:215-230: the user id
//                     repeated, and each candidate's item id, categorical codes
//                     and scaled numeric features gathered from per-item tables
//   rank by score     sorted(zip(scores, ids), key=score, reverse=True),
//                     main.py:325: descending, equal scores keep input order
//   MMR re-rank       rerank_with_mmr, main.py:133-169: greedy
//                     argmax of lambda * score - (1 - lambda) * max cosine
//                     similarity to the already selected items
//
// Each is one workgroup (the sets are tens to thousands of items): the sort is
// an LDS bitonic sort of (key, position) pairs, so ties resolve by position
// exactly as Python's stable sort does.
//
// A batch of R requests (req_* kernels) is the same work over CSR segments,
// request r in workgroup r, side by side on the CUs: candidates (their
// neighbours from the call's top-k lists or from the item neighbour table,
// one staging loop: KnnLists / NbrTable) with the
// fallback and the allowed / excluded filters (main.py:204-212) as binary
// searches in resident row sets, the offsets of the compacted batch, its
// ranking batch, and rank + MMR per segment.  Both forms call one copy of
// each building block (lds_bitonic, block_compact, union_entry, batch_row,
// rank_sort, block_argmax, mmr_sim / mmr_value / mmr_better, mmr_table /
// mmr_lds), so a request's answer is the same bits either way.  The blocks the
// large lane (serving_large.hip: requests above SV_MAX) calls as well stand in
// serving_blocks.h: SV_NT / SV_MAX, KnnLists / NbrTable / union_entry,
// set_contains / ReqSets / req_set, batch_row, block_argmax and the MMR's
// arithmetic with its two forms.
#include "serving_blocks.h"

namespace dcnr {
namespace {

// ascending bitonic sort of n2 (power of two) (key, val) pairs in LDS;
// less(a, b) on (key, val)
template <typename K>
__device__ void lds_bitonic(K* key, int* val, int n2) {
  for (int k2 = 2; k2 <= n2; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < n2 / 2; t += SV_NT) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo + j;
        const bool asc = (lo & k2) == 0;
        const K ka = key[lo], kb = key[hi];
        const int va = val[lo], vb = val[hi];
        const bool b_less = kb < ka || (kb == ka && vb < va);
        if (asc ? b_less : !b_less && (ka != kb || va != vb)) {
          key[lo] = kb; key[hi] = ka; val[lo] = vb; val[hi] = va;
        }
      }
      __syncthreads();
    }
  }
}

// Stable compaction by the whole workgroup: for t < n in order, where
// flag(t, v) holds (it also hands over the element's value v), write(p, v)
// with p = the number of flagged elements before t (ballot prefix per wave,
// wave totals through LDS).  Every value is taken before the chunk's barrier
// and written after it, to p <= t, so write may store into the array flag
// reads.  Returns the number of flagged elements, in every thread.
template <typename V, typename F, typename W>
__device__ int block_compact(int n, int* wsum, F flag, W write) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int running = 0;
  for (int base = 0; base < n; base += SV_NT) {
    const int t = base + threadIdx.x;
    V v = V();
    const bool f = t < n && flag(t, v);
    const uint64_t m = __ballot(f);
    const int pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = running, tot = 0;
    for (int i = 0; i < SV_NT / 64; ++i) {
      off += i < w ? wsum[i] : 0;
      tot += wsum[i];
    }
    if (f) write(off + pre, v);
    running += tot;
    __syncthreads();
  }
  return running;
}

// key[0 .. n2) sorted ascending (INT64_MAX last): the first occurrence of
// every row, compacted through write; returns their number
template <typename W>
__device__ int distinct_rows(const int64_t* key, int n2, int* wsum, W write) {
  return block_compact<int64_t>(
      n2, wsum,
      [&](int t, int64_t& v) {
        v = key[t];
        return v != INT64_MAX && (t == 0 || v != key[t - 1]);
      },
      write);
}

// union of positives[Q] and their neighbours [1:] (rows < 0 skipped) ->
// ascending unique rows; out_count[0] = number of rows, or -1 where the
// neighbour source reported bad data (NbrTable)
template <class Src>
__global__ __launch_bounds__(SV_NT) void union_kernel(const int64_t* pos, int64_t Q, Src src, int k,
                                                      int64_t* out, int32_t* out_count) {
  __shared__ int64_t key[SV_MAX];
  __shared__ int val[SV_MAX];
  __shared__ int wsum[SV_NT / 64];
  __shared__ int bad;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  const int n = (int)(Q * k);   // positives + k-1 neighbours per query
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += SV_NT) {
    bool b = false;
    key[t] = t < n ? union_entry(pos, src, k, t, b) : INT64_MAX;
    val[t] = t;
    if (b) bad = 1;
  }
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) *out_count = -1;
    return;
  }
  lds_bitonic(key, val, n2);
  const int cnt = distinct_rows(key, n2, wsum, [&](int p, int64_t v) { out[p] = v; });
  if (threadIdx.x == 0) *out_count = cnt;
}

// The candidates of request r = blockIdx.x (main.py:196-212 on hotel rows):
// union of its positives and their neighbours; the fallback set joined when
// fewer than min_cand rows resulted; the allowed / excluded filters; the
// surviving rows ascending in out[r][0 .. cap), their number in out_count[r].
// status[r]: REQ_OVERFLOW when the staged list, the union or the result does
// not fit (count 0), REQ_BAD_DATA when the request's offsets, set indices or
// rows lie outside the lengths passed by value (count 0).  Every index formed
// here is checked against one of those lengths first.
template <class Src>
__global__ __launch_bounds__(SV_NT) void req_candidates_kernel(
    const int64_t* pos, const int64_t* pos_off, int64_t R, int64_t Q_total, Src src,
    int k, ReqSets st, int min_cand, int64_t n_items, int cap, int64_t* out, int32_t* out_count,
    int32_t* status) {
  __shared__ int64_t key[SV_MAX];
  __shared__ int val[SV_MAX];
  __shared__ int wsum[SV_NT / 64];
  __shared__ int bad;
  const int64_t r = blockIdx.x;
  if (r >= R) return;
  // (everything that decides an exit below is uniform over the workgroup)
  auto finish = [&](int cnt, int32_t stt) {
    if (threadIdx.x == 0) { out_count[r] = cnt; status[r] = stt; }
  };
  const int64_t q0 = pos_off[r], q1 = pos_off[r + 1];
  const int64_t *arows, *erows, *frows;
  int64_t alen, elen, flen;
  const bool a_ok = req_set(st, st.allowed, r, arows, alen);
  const bool e_ok = req_set(st, st.excluded, r, erows, elen);
  const bool f_ok = req_set(st, st.fallback, r, frows, flen);
  const bool sets_ok = a_ok && e_ok && f_ok;
  if (q0 < 0 || q1 < q0 || q1 > Q_total || !sets_ok) return finish(0, REQ_BAD_DATA);
  // ascending sets: the ends bound every row of a filter set (its rows are
  // compared, never used as an index; fallback rows are checked one by one)
  if ((alen > 0 && (arows[0] < 0 || arows[alen - 1] >= n_items)) ||
      (elen > 0 && (erows[0] < 0 || erows[elen - 1] >= n_items)))
    return finish(0, REQ_BAD_DATA);
  if ((q1 - q0) * k > SV_MAX) return finish(0, REQ_OVERFLOW);
  const int n = (int)((q1 - q0) * k);
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += SV_NT) {
    int64_t v = INT64_MAX;
    if (t < n) {
      bool b = false;
      v = union_entry(pos + q0, src.from(q0), k, t, b);
      if (b || (v != INT64_MAX && v >= n_items)) { bad = 1; v = INT64_MAX; }
    }
    key[t] = v;
    val[t] = t;
  }
  __syncthreads();
  if (bad) return finish(0, REQ_BAD_DATA);
  lds_bitonic(key, val, n2);
  // distinct rows, compacted in place: key[0 .. m)
  int m = distinct_rows(key, n2, wsum, [&](int p, int64_t v) { key[p] = v; });
  if (flen >= 0 && m < min_cand) {
    // the fallback rows not among them, appended (while room), then one more sort
    const int n1 = m;
    const int extra = block_compact<int64_t>(
        (int)flen, wsum,
        [&](int t, int64_t& v) {
          v = frows[t];
          if (v < 0 || v >= n_items) { bad = 1; return false; }
          return !set_contains(key, n1, v);
        },
        [&](int p, int64_t v) { if (n1 + p < SV_MAX) key[n1 + p] = v; });
    if (bad) return finish(0, REQ_BAD_DATA);
    if ((int64_t)n1 + extra > SV_MAX) return finish(0, REQ_OVERFLOW);
    m = n1 + extra;
    n2 = 1;
    while (n2 < m) n2 <<= 1;
    for (int t = threadIdx.x; t < n2; t += SV_NT) {
      if (t >= m) key[t] = INT64_MAX;
      val[t] = t;
    }
    __syncthreads();
    lds_bitonic(key, val, n2);
  }
  int64_t* slot = out + r * cap;
  const int cnt = block_compact<int64_t>(
      m, wsum,
      [&](int t, int64_t& v) {
        v = key[t];
        return (alen < 0 || set_contains(arows, alen, v)) &&
               !(elen > 0 && set_contains(erows, elen, v));
      },
      [&](int p, int64_t v) { if (p < cap) slot[p] = v; });
  if (cnt > cap) return finish(0, REQ_OVERFLOW);
  finish(cnt, 0);
}

// offsets[r] = sum of count[0 .. r) (counts clamped to 0 .. cap), r <= R, by
// one workgroup; mirrored to host_off, and status [R] to host_status (pinned
// host memory, or null), with system-scope stores, visible to the host once
// the stream has reached here
__global__ __launch_bounds__(SV_NT) void req_offsets_kernel(const int32_t* count,
                                                            const int32_t* status, int64_t R,
                                                            int cap, int64_t* offsets,
                                                            int64_t* host_off,
                                                            int32_t* host_status) {
  __shared__ int wsum[SV_NT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t running = 0;
  auto put = [&](int64_t i, int64_t v) {
    offsets[i] = v;
    if (host_off) __hip_atomic_store(host_off + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  };
  for (int64_t base = 0; base < R; base += SV_NT) {
    const int64_t t = base + threadIdx.x;
    const int c = t < R ? min(max(count[t], 0), cap) : 0;
    int inc = c;   // inclusive scan over the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
    for (int i = 0; i < SV_NT / 64; ++i) {
      off += i < w ? wsum[i] : 0;
      tot += wsum[i];
    }
    if (t < R) {
      put(t, running + off + inc - c);
      if (host_status)
        __hip_atomic_store(host_status + t, status[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    running += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) put(R, running);
}

// ranking batch for one user over rows[n]
__global__ void batch_kernel(const int64_t* rows, int64_t n, int64_t user_row,
                             const int64_t* item_cat, int K, const float* item_num, int F,
                             int64_t n_items, int64_t* user_out, int64_t* item_out,
                             int64_t* cat_out, float* num_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  if (i >= n) return;
  batch_row(i, rows[i], user_row, item_cat, K, item_num, F, n_items, user_out, item_out, cat_out,
            num_out);
}

// ranking batch of a whole batch of requests: row i < n of the compacted
// batch belongs to the request whose segment [offsets[r], offsets[r + 1])
// holds it and is candidate i - offsets[r] of slots[r][cap] (a position the
// offsets put outside the slot reads as row 0)
__global__ void req_batch_kernel(const int64_t* slots, int cap, const int64_t* offsets, int64_t R,
                                 int64_t n, const int64_t* user_rows, const int64_t* item_cat,
                                 int K, const float* item_num, int F, int64_t n_items,
                                 int64_t* user_out, int64_t* item_out, int64_t* cat_out,
                                 float* num_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  if (i >= n) return;
  int64_t lo = 0, hi = R - 1;   // the last request with offsets[r] <= i
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int64_t j = i - offsets[lo];
  const int64_t row = j >= 0 && j < cap ? slots[lo * cap + j] : 0;
  batch_row(i, row, user_rows[lo], item_cat, K, item_num, F, n_items, user_out, item_out, cat_out,
            num_out);
}

// val[0 .. n) = positions of scores[0 .. n) in descending score order (ties:
// lower position first), through key / val [n rounded up to a power of two]
__device__ void rank_sort(const float* scores, int n, float* key, int* val) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += SV_NT) {
    key[t] = t < n ? -scores[t] : FLT_MAX;   // ascending on -score
    val[t] = t < n ? t : INT_MAX;
  }
  __syncthreads();
  lds_bitonic(key, val, n2);
}

// order[i] = position of the i-th highest score (ties: lower position first)
__global__ __launch_bounds__(SV_NT) void rank_kernel(const float* scores, int n, int64_t* order) {
  __shared__ float key[SV_MAX];
  __shared__ int val[SV_MAX];
  rank_sort(scores, n, key, val);
  for (int t = threadIdx.x; t < n; t += SV_NT) order[t] = val[t];
}

__global__ __launch_bounds__(SV_NT) void mmr_kernel(const float* table, const float* inv, int d,
                                                    const int64_t* rows, const float* scores,
                                                    int n, float lambda, int top_k,
                                                    int64_t* out_pos, int32_t* out_count) {
  __shared__ float maxsim[SV_MAX];
  __shared__ unsigned char taken[SV_MAX];
  __shared__ float selv[256];
  const int cnt = mmr_table(table, inv, d, rows, scores, n, lambda, top_k, maxsim, taken, selv,
                            [&](int i, int p) { out_pos[i] = p; });
  for (int t = threadIdx.x + cnt; t < top_k; t += SV_NT) out_pos[t] = -1;
  if (threadIdx.x == 0) *out_count = cnt;
}

__global__ __launch_bounds__(SV_NT) void mmr_lds_kernel(const float* table, const float* inv, int d,
                                                    const int64_t* rows, const float* scores,
                                                    int n, float lambda, int top_k,
                                                    int64_t* out_pos, int32_t* out_count) {
  __shared__ unsigned char vld[SV_MAX];
  extern __shared__ float lds_rows[];
  const int cnt = mmr_lds(table, inv, d, rows, scores, n, lambda, top_k, lds_rows, vld,
                          [&](int i, int p) { out_pos[i] = p; });
  for (int t = threadIdx.x + cnt; t < top_k; t += SV_NT) out_pos[t] = -1;
  if (threadIdx.x == 0) *out_count = cnt;
}

// Rank + MMR of request r = blockIdx.x over its segment [offsets[r],
// offsets[r + 1]) of the compacted batch: the segment's logits sorted
// descending (ties by position); lambda[r] >= 1: the whole ranked list; else
// the greedy MMR over it with top_k[r], in the LDS-resident form when the
// segment fits it, the table-reading form otherwise.  Ranked rows and their
// logits go to the segment's start of out_rows / out_logits, their number to
// out_count[r].  rrows / rscores [R][cap] (workspace) hold the ranked list the
// MMR reads.  Everything in LDS but 4 KiB is dynamic (MMR_LDS_MAX), carved per
// stage: the sort's keys, then either form's scratch.  A segment the offsets
// put outside the batch or the slot, a top_k < 1, a row >= n_items or a logit
// without a rank (-inf, NaN): count 0 and REQ_BAD_DATA in status[r].
__global__ __launch_bounds__(SV_NT) void req_rank_mmr_kernel(
    const float* logits, int64_t n_total, const int64_t* slots, int cap, const int64_t* offsets,
    int64_t R, const float* table, const float* inv, int d, int64_t n_items, const float* lambda,
    const int32_t* top_k, int64_t* rrows, float* rscores, int64_t* out_rows, float* out_logits,
    int32_t* out_count, int32_t* status) {
  __shared__ unsigned char flags[SV_MAX];   // vld (LDS form) / taken (table form)
  __shared__ int bad;
  extern __shared__ float dyn[];
  const int64_t r = blockIdx.x;
  if (r >= R) return;
  const int64_t o0 = offsets[r], o1 = offsets[r + 1];
  const float lam = lambda[r];
  const int tk = top_k[r];
  if (o0 < 0 || o1 < o0 || o1 > n_total || o1 - o0 > cap || (lam < 1.f && tk < 1)) {
    if (threadIdx.x == 0) { out_count[r] = 0; status[r] |= REQ_BAD_DATA; }
    return;
  }
  const int n = (int)(o1 - o0);
  if (n == 0) {
    if (threadIdx.x == 0) out_count[r] = 0;
    return;
  }
  const int64_t* slot = slots + r * cap;
  const float* z = logits + o0;
  float* key = dyn;
  int* val = (int*)(dyn + SV_MAX);
  if (threadIdx.x == 0) bad = 0;
  rank_sort(z, n, key, val);
  // a logit that does not order below the padding (-inf, NaN) leaves a
  // padding position among the first n: no position is used unchecked
  const bool mmr = lam < 1.f;
  int64_t* rr = rrows + r * cap;
  float* rs = rscores + r * cap;
  for (int t = threadIdx.x; t < n; t += SV_NT) {
    const int p = val[t];
    if (p < 0 || p >= n) { bad = 1; continue; }
    const int64_t row = slot[p];
    const float zp = z[p];
    if (!(zp >= -FLT_MAX)) bad = 1;   // -inf, NaN (a NaN may leave the padding in place)
    if (!mmr) {   // main.py:325-326: the sorted list is the answer
      out_rows[o0 + t] = row;
      out_logits[o0 + t] = zp;
    } else {
      if (row >= n_items) bad = 1;
      rr[t] = row;
      rs[t] = zp;
    }
  }
  __syncthreads();   // the ranked list is in memory; the sort's LDS is free
  if (bad) {
    // the whole segment marked (rows -1, logits NaN), so that a caller who does
    // not read the status back never takes stale memory for an answer
    for (int t = threadIdx.x; t < n; t += SV_NT) {
      out_rows[o0 + t] = -1;
      out_logits[o0 + t] = __int_as_float(0x7fc00000);
    }
    if (threadIdx.x == 0) { out_count[r] = 0; status[r] |= REQ_BAD_DATA; }
    return;
  }
  if (!mmr) {
    if (threadIdx.x == 0) out_count[r] = n;
    return;
  }
  auto emit = [&](int i, int p) { out_rows[o0 + i] = rr[p]; out_logits[o0 + i] = rs[p]; };
  const int cnt = mmr_lds_bytes(n, d) <= MMR_LDS_MAX
                      ? mmr_lds(table, inv, d, rr, rs, n, lam, tk, dyn, flags, emit)
                      : mmr_table(table, inv, d, rr, rs, n, lam, tk, dyn, flags, dyn + SV_MAX, emit);
  if (threadIdx.x == 0) out_count[r] = cnt;
}

// ---- requests by user: the interaction store (dcnr.InteractionStore) on the
// device, the steps of /recommendations that read it (get_friends_for_user,
// main.py:172-178; the positives and negatives of _generate_candidates,
// main.py:187-194; the recommended_by lists, main.py:336-351)
//
// Two CSRs over the U reviewers: friends (symmetric, distinct) and reviews
// (within a reviewer in main_df order): rv_item = hotel row * 4 + class bits
// (1: rating >= 8, 2: rating <= 4), rv_row = the review's main_df row.
struct ReqStore {
  int64_t U;
  const int64_t* fr_off; const int32_t* fr_idx; int64_t n_fr;
  const int64_t* rv_off; const int32_t* rv_item; const int32_t* rv_row; int64_t M;
};

constexpr int REQ_FRIENDS = 0, REQ_PERSONAL = 1;   // dcnr.h: DCNR_MODE_*
constexpr int64_t SRC_NEG = int64_t(1) << 40;      // staged key of a negative row: row + SRC_NEG

// the friend list of reviewer u (0 <= u < U) as (first, length); false:
// offsets outside the CSR
__device__ bool store_friends(const ReqStore& st, int64_t u, const int32_t*& fr, int64_t& nf) {
  const int64_t lo = st.fr_off[u], hi = st.fr_off[u + 1];
  fr = nullptr;
  nf = 0;
  if (lo < 0 || hi < lo || hi > st.n_fr) return false;
  fr = st.fr_idx + lo;
  nf = hi - lo;
  return true;
}

// the review segment [lo, hi) of reviewer f; false: f outside [0, U) or
// offsets outside the CSR
__device__ bool store_reviews(const ReqStore& st, int64_t f, int64_t& lo, int64_t& hi) {
  lo = hi = 0;
  if (f < 0 || f >= st.U) return false;
  lo = st.rv_off[f];
  hi = st.rv_off[f + 1];
  return lo >= 0 && hi >= lo && hi <= st.M;
}

// Sum of the review rows of the nf sources of a request (src(i): source i),
// one wave per source, into *total (LDS, zeroed by the caller before a
// barrier); *bad set when a source or its offsets lie outside the store
template <typename Src>
__device__ void store_count_rows(const ReqStore& st, int64_t nf, Src src,
                                 unsigned long long* total, int* bad) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t i = w; i < nf; i += SV_NT / 64) {
    int64_t lo, hi;
    if (!store_reviews(st, src(i), lo, hi)) { *bad = 1; continue; }
    if (lane == 0) atomicAdd(total, (unsigned long long)(hi - lo));
  }
}

// first position of key[0 .. n) (ascending) not below v
template <typename K>
__device__ __forceinline__ int lower_bound(const K* key, int n, K v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (key[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The positives and negatives of request r = blockIdx.x (main.py:187-194 on
// hotel rows): the reviews of its sources -- the friends of reviewers[r]
// (REQ_FRIENDS) or the reviewer alone (REQ_PERSONAL); -1 = unknown user, no
// sources -- staged in LDS as row (rating >= 8) or row + SRC_NEG (rating <= 4),
// sorted, made distinct.  The request owns pos[pos_off[r] .. pos_off[r + 1])
// and neg[neg_off[r] .. neg_off[r + 1]) (lengths the host knows as bounds of
// the counts): its distinct positives ascending, then the last repeated to
// the segment's end; likewise its negatives, which makes the segment a set
// req_candidates_kernel's binary search takes as `excluded`.  counts[2r],
// counts[2r + 1] = the distinct numbers.  status[r]: REQ_OVERFLOW when the
// friends or the staged review rows exceed SV_MAX, REQ_BAD_DATA when a
// reviewer, mode, offset, friend or hotel row lies outside the lengths passed
// by value, or a segment is shorter than its count or non-empty with count 0;
// both leave counts 0 and the segments filled with -1 (no positive; a set
// req_candidates_kernel rejects).  counts and status are mirrored to pinned
// host memory (or null) with system-scope stores, as req_offsets_kernel does.
__global__ __launch_bounds__(SV_NT) void req_sources_kernel(
    ReqStore st, const int32_t* reviewers, const int32_t* modes, int64_t R, int64_t n_items,
    const int64_t* pos_off, int64_t Q_total, int64_t* pos, const int64_t* neg_off, int64_t neg_lo,
    int64_t neg_hi, int64_t* neg, int32_t* counts, int32_t* status, int32_t* host_counts,
    int32_t* host_status) {
  __shared__ int64_t key[SV_MAX];
  __shared__ int val[SV_MAX];
  __shared__ int wsum[SV_NT / 64];
  __shared__ int bad, n_st;
  __shared__ unsigned long long total;
  const int64_t r = blockIdx.x;
  if (r >= R) return;
  // (everything that decides an exit below is uniform over the workgroup)
  const int64_t p0 = pos_off[r], p1 = pos_off[r + 1], g0 = neg_off[r], g1 = neg_off[r + 1];
  const bool seg_ok = p0 >= 0 && p1 >= p0 && p1 <= Q_total && p1 - p0 <= SV_MAX && g0 >= neg_lo &&
                      g1 >= g0 && g1 <= neg_hi && g1 - g0 <= SV_MAX;
  const int np = seg_ok ? (int)(p1 - p0) : 0, ng = seg_ok ? (int)(g1 - g0) : 0;
  auto finish = [&](int npos, int nneg, int32_t stt) {
    if (stt) {   // nothing of the segments stays unwritten
      for (int t = threadIdx.x; t < np; t += SV_NT) pos[p0 + t] = -1;
      for (int t = threadIdx.x; t < ng; t += SV_NT) neg[g0 + t] = -1;
    }
    if (threadIdx.x == 0) {
      counts[2 * r] = npos; counts[2 * r + 1] = nneg; status[r] = stt;
      if (host_counts) {
        __hip_atomic_store(host_counts + 2 * r, npos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_counts + 2 * r + 1, nneg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      if (host_status)
        __hip_atomic_store(host_status + r, stt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  };
  const int64_t u = reviewers[r];
  const int mode = modes[r];
  if (!seg_ok || u < -1 || u >= st.U || (mode != REQ_FRIENDS && mode != REQ_PERSONAL))
    return finish(0, 0, REQ_BAD_DATA);
  const int32_t* fr = nullptr;
  int64_t nf = 0;
  if (u >= 0 && mode == REQ_PERSONAL) nf = 1;
  else if (u >= 0 && !store_friends(st, u, fr, nf)) return finish(0, 0, REQ_BAD_DATA);
  if (nf > SV_MAX) return finish(0, 0, REQ_OVERFLOW);
  auto src = [&](int64_t i) -> int64_t { return fr ? fr[i] : u; };
  if (threadIdx.x == 0) { bad = 0; n_st = 0; total = 0; }
  __syncthreads();
  store_count_rows(st, nf, src, &total, &bad);
  __syncthreads();
  if (bad) return finish(0, 0, REQ_BAD_DATA);
  if (total > (unsigned long long)SV_MAX) return finish(0, 0, REQ_OVERFLOW);
  // stage the classed reviews, one wave per source; the order in the list is
  // of no account (it is sorted next), so a slot is claimed with an LDS atomic
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t i = w; i < nf; i += SV_NT / 64) {
    int64_t lo, hi;
    if (!store_reviews(st, src(i), lo, hi)) { bad = 1; continue; }
    for (int64_t j = lo + lane; j < hi; j += 64) {
      const int32_t wd = st.rv_item[j];
      const int cls = wd & 3;
      if (wd < 0 || (wd >> 2) >= n_items || cls == 3) { bad = 1; continue; }
      if (cls == 0) continue;
      const int p = atomicAdd(&n_st, 1);
      if (p >= SV_MAX) { bad = 1; continue; }   // (total <= SV_MAX: not reached)
      key[p] = (int64_t)(wd >> 2) + (cls == 2 ? SRC_NEG : 0);
      val[p] = 0;
    }
  }
  __syncthreads();
  if (bad) return finish(0, 0, REQ_BAD_DATA);
  const int n = n_st;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int t = n + threadIdx.x; t < n2 || t < 1; t += SV_NT) { key[t] = INT64_MAX; val[t] = 0; }
  __syncthreads();
  lds_bitonic(key, val, n2);
  // distinct keys, compacted in place: positives key[0 .. npos), negatives behind
  const int m = distinct_rows(key, n2, wsum, [&](int p, int64_t v) { key[p] = v; });
  const int npos = lower_bound<int64_t>(key, m, SRC_NEG), nneg = m - npos;
  if (npos > np || nneg > ng || (npos == 0) != (np == 0) || (nneg == 0) != (ng == 0))
    return finish(0, 0, REQ_BAD_DATA);
  for (int t = threadIdx.x; t < np; t += SV_NT) pos[p0 + t] = key[min(t, npos - 1)];
  for (int t = threadIdx.x; t < ng; t += SV_NT) neg[g0 + t] = key[npos + min(t, nneg - 1)] - SRC_NEG;
  finish(npos, nneg, 0);
}

struct ByPair { int64_t k; int v; };

// The recommended_by lists of request r = blockIdx.x (main.py:336-351), after
// req_rank_mmr_kernel: for each returned position i < out_count[r] of its
// segment [offsets[r], offsets[r + 1]) of out_rows, the distinct friends of
// reviewers[r] (whatever the request's mode) with a rating >= 8 review of that
// hotel, in the order of their first such review's main_df row.  The returned
// rows sorted in LDS are the map hotel -> position; the matching reviews are
// staged as (position, reviewer, review row) and sorted, the first of every
// (position, reviewer) kept, and those sorted by (position, review row).  The
// reviewers go, position by position, to lists[list_off[r] .. list_off[r + 1])
// (a length the host knows as a bound; the rest -1), their number per
// position to by_count[offsets[r] + i] (0 from out_count[r] on).  status[r]:
// REQ_OVERFLOW (friends or their review rows above SV_MAX) and REQ_BAD_DATA
// (an offset, count, reviewer, friend, hotel or review row outside the
// lengths passed by value; more reviewers than the list segment holds) leave
// every count of the request 0.
__global__ __launch_bounds__(SV_NT) void req_recommended_by_kernel(
    ReqStore st, const int32_t* reviewers, int64_t R, int64_t n_items, const int64_t* out_rows,
    int64_t n_total, const int64_t* offsets, const int32_t* out_count, const int64_t* list_off,
    int64_t L_total, int32_t* lists, int32_t* by_count, int32_t* status) {
  __shared__ int mkey[SV_MAX];
  __shared__ int mval[SV_MAX];
  __shared__ int64_t key[SV_MAX];
  __shared__ int val[SV_MAX];
  __shared__ int wsum[SV_NT / 64];
  __shared__ int bad, n_st;
  __shared__ unsigned long long total;
  const int64_t r = blockIdx.x;
  if (r >= R) return;
  const int64_t o0 = offsets[r], o1 = offsets[r + 1], l0 = list_off[r], l1 = list_off[r + 1];
  const bool seg_ok = o0 >= 0 && o1 >= o0 && o1 <= n_total && o1 - o0 <= SV_MAX;
  const bool list_ok = l0 >= 0 && l1 >= l0 && l1 <= L_total;
  const int n = seg_ok ? (int)(o1 - o0) : 0;
  const int64_t nl = list_ok ? l1 - l0 : 0;
  // a request without lists: every count 0, its list segment -1
  auto finish = [&](int32_t stt) {
    for (int t = threadIdx.x; t < n; t += SV_NT) by_count[o0 + t] = 0;
    for (int64_t t = threadIdx.x; t < nl; t += SV_NT) lists[l0 + t] = -1;
    if (threadIdx.x == 0) status[r] = stt;
  };
  const int c = out_count[r];
  const int64_t u = reviewers[r];
  if (!seg_ok || !list_ok || c < 0 || c > n || u < -1 || u >= st.U) return finish(REQ_BAD_DATA);
  if (c == 0 || u < 0) return finish(0);
  const int32_t* fr;
  int64_t nf;
  if (!store_friends(st, u, fr, nf)) return finish(REQ_BAD_DATA);
  if (nf > SV_MAX) return finish(REQ_OVERFLOW);
  auto src = [&](int64_t i) -> int64_t { return fr[i]; };
  if (threadIdx.x == 0) { bad = 0; n_st = 0; total = 0; }
  __syncthreads();
  store_count_rows(st, nf, src, &total, &bad);
  __syncthreads();
  if (bad) return finish(REQ_BAD_DATA);
  if (total > (unsigned long long)SV_MAX) return finish(REQ_OVERFLOW);
  // hotel row -> position among the c returned rows (a row outside the table,
  // the -1 of a marked answer: never found)
  int c2 = 1;
  while (c2 < c) c2 <<= 1;
  for (int t = threadIdx.x; t < c2; t += SV_NT) {
    const int64_t row = t < c ? out_rows[o0 + t] : -1;
    mkey[t] = row >= 0 && row < n_items ? (int)row : INT_MAX;
    mval[t] = t;
  }
  __syncthreads();
  lds_bitonic(mkey, mval, c2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t i = w; i < nf; i += SV_NT / 64) {
    const int64_t f = fr[i];
    int64_t lo, hi;
    if (!store_reviews(st, f, lo, hi)) { bad = 1; continue; }
    for (int64_t j = lo + lane; j < hi; j += 64) {
      const int32_t wd = st.rv_item[j];
      const int32_t row = st.rv_row[j];
      // (row is a sort key only, and not below M: rows that were removed leave gaps)
      if (wd < 0 || (wd >> 2) >= n_items || row < 0) { bad = 1; continue; }
      if (!(wd & 1)) continue;
      const int q = lower_bound<int>(mkey, c2, wd >> 2);
      if (q >= c2 || mkey[q] != (wd >> 2)) continue;
      const int p = atomicAdd(&n_st, 1);
      if (p >= SV_MAX) { bad = 1; continue; }   // (total <= SV_MAX: not reached)
      key[p] = ((int64_t)mval[q] << 32) | (uint32_t)f;
      val[p] = row;
    }
  }
  __syncthreads();
  if (bad) return finish(REQ_BAD_DATA);
  const int ns = n_st;
  int n2 = 1;
  while (n2 < ns) n2 <<= 1;
  for (int t = ns + threadIdx.x; t < n2 || t < 1; t += SV_NT) { key[t] = INT64_MAX; val[t] = 0; }
  __syncthreads();
  lds_bitonic(key, val, n2);   // by (position, reviewer), then review row
  // a reviewer's repeats dropped: the first of every (position, reviewer), in place
  const int m = block_compact<ByPair>(
      n2, wsum,
      [&](int t, ByPair& v) {
        v.k = key[t];
        v.v = val[t];
        return v.k != INT64_MAX && (t == 0 || v.k != key[t - 1]);
      },
      [&](int p, ByPair v) { key[p] = v.k; val[p] = v.v; });
  if (m > nl) return finish(REQ_BAD_DATA);
  // (position, reviewer | row) -> (position, row | reviewer), each thread its own entries
  int m2 = 1;
  while (m2 < m) m2 <<= 1;
  for (int t = threadIdx.x; t < m2; t += SV_NT) {
    const int64_t k = key[t];
    const int row = val[t];
    key[t] = t < m ? (k & ~(int64_t)0xffffffff) | (uint32_t)row : INT64_MAX;
    val[t] = t < m ? (int)(uint32_t)k : 0;
  }
  __syncthreads();
  lds_bitonic(key, val, m2);   // by (position, first review row)
  for (int64_t t = threadIdx.x; t < nl; t += SV_NT) lists[l0 + t] = t < m ? val[t] : -1;
  for (int t = threadIdx.x; t < n; t += SV_NT)
    by_count[o0 + t] = t < c ? lower_bound<int64_t>(key, m, (int64_t)(t + 1) << 32) -
                                   lower_bound<int64_t>(key, m, (int64_t)t << 32)
                             : 0;
  if (threadIdx.x == 0) status[r] = 0;
}

// by_reviewers as one CSR over the n positions of the result (by_off [n + 1]
// = the exclusive sum of by_count): position i of request r (the segment of
// offsets holding it) copies its by_count[i] reviewers from the request's
// list segment, where they follow those of the request's earlier positions;
// the words behind by_off[n] are set to -1.  A copy that would leave either
// buffer (L_total words) is not made.
__global__ void req_by_gather_kernel(const int32_t* lists, const int64_t* list_off, int64_t L_total,
                                     const int64_t* offsets, int64_t R, int64_t n,
                                     const int32_t* by_count, const int64_t* by_off,
                                     int32_t* by_reviewers) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t end = n > 0 ? by_off[n] : 0;
  if (i >= end && i < L_total) by_reviewers[i] = -1;   // (one thread per word of the tail, too)
  if (i >= n) return;
  int64_t lo = 0, hi = R - 1;   // the last request with offsets[r] <= i
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo + 1) >> 1);
    if (offsets[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int64_t o0 = offsets[lo];
  if (o0 < 0 || o0 > i) return;
  const int64_t dst = by_off[i], src = list_off[lo] + (dst - by_off[o0]);
  const int64_t cnt = by_count[i];
  if (cnt <= 0 || dst < 0 || src < 0 || dst + cnt > L_total || src + cnt > L_total) return;
  for (int64_t j = 0; j < cnt; ++j) by_reviewers[dst + j] = lists[src + j];
}

// Batch assembly of a device-resident dataset (the DataLoader of
// train.py:195-196): dst_a[i] = src_a[idx[i]] for each array a, whole rows of
// row_bytes (a multiple of 4) copied as dwords, one wave per (row, array).
struct RowGather {
  const char* src[8];
  char* dst[8];
  int64_t row_bytes[8];
  int n;
};

__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t* idx, int64_t n,
                                                          int64_t n_src, RowGather g) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= n * g.n) return;
  const int a = (int)(w % g.n);
  const int64_t i = w / g.n;
  int64_t r = idx[i];
  r = r < 0 ? 0 : (r >= n_src ? n_src - 1 : r);
  const int64_t words = g.row_bytes[a] >> 2;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(g.src[a] + r * g.row_bytes[a]);
  uint32_t* d = reinterpret_cast<uint32_t*>(g.dst[a] + i * g.row_bytes[a]);
  for (int64_t k = lane; k < words; k += 64) d[k] = s[k];
}

// ---- a new generation of a CSR with m entries inserted (dcnr_csr_insert;
// InteractionStore.append).  Output-centric: the output positions are cut into
// chunks of CI_CHUNK, the new offsets into chunks behind them, and a workgroup
// takes a contiguous range of chunks; every output element is written once, by
// one lane, from the old generation (read only) or the uploaded batch.  An
// output position p holds old[p - (the inserts in front of p)]; the inserts in
// front are constant between two touched segments, so a chunk no touched
// segment reaches into is a copy shifted by a constant: destination-aligned
// 16-byte stores, the source read as the two aligned 16-byte words around it
// (it is misaligned by the shift).  Only chunks a touched segment reaches into
// search per element.  The touched owners' new segment bounds that a workgroup
// can meet are staged in LDS when there are at most CI_LDS_RUNS of them and
// derived from the global arrays otherwise.  All positions are 64-bit.
constexpr int CI_NT = 256;
constexpr int CI_CHUNK = DCNR_CSR_INSERT_CHUNK;
constexpr int CI_LDS_RUNS = 1024;
constexpr int CI_MAX_BLOCKS = 2048;
static_assert(CI_CHUNK % (4 * CI_NT) == 0, "a chunk is whole 16-byte stores of the workgroup");

struct CsrInsert {
  const int64_t* old_off;   // [U_old + 1]
  const int64_t* touched;   // [t] ascending, distinct
  const int64_t* prefix;    // [t + 1] inserts in front of touched owner j
  const int64_t* ins_pos;   // [m] position inside the owner's new segment
  const int32_t* old_val[2];
  const int32_t* ins_val[2];
  int32_t* new_val[2];
  int64_t* new_off;         // [U_new + 1]
  int64_t U_old, U_new, M_old, m, t;
  int64_t n_pay_units, n_units, units_per_block;
  int n_payloads, vec;
};

// first j in [lo, hi) where pred holds (pred: false ... false true ... true), else hi
template <class F>
__device__ __forceinline__ int64_t ci_first(int64_t lo, int64_t hi, F pred) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (pred(mid)) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// old start of owner o in [0, U_new]: owners at or beyond U_old start from M_old
__device__ __forceinline__ int64_t ci_old_at(const CsrInsert& a, int64_t o) {
  return o <= a.U_old ? a.old_off[o] : a.M_old;
}
__device__ __forceinline__ int64_t ci_owner(const CsrInsert& a, int64_t j) {
  const int64_t o = a.touched[j];
  return o < 0 ? 0 : (o >= a.U_new ? a.U_new - 1 : o);
}
// touched owner j's new segment [ns, ne)
__device__ __forceinline__ int64_t ci_ns(const CsrInsert& a, int64_t j) {
  return ci_old_at(a, ci_owner(a, j)) + a.prefix[j];
}
__device__ __forceinline__ int64_t ci_ne(const CsrInsert& a, int64_t j) {
  return ci_old_at(a, ci_owner(a, j) + 1) + a.prefix[j + 1];
}

__device__ __forceinline__ int32_t ci_old(const int32_t* src, int64_t e, int64_t M_old) {
  if (M_old <= 0) return 0;
  return src[e < 0 ? 0 : (e >= M_old ? M_old - 1 : e)];
}

// dst[w][c0, c1) = src[w][c0 - shift, c1 - shift) for each payload: c0 is a
// multiple of CI_CHUNK, the shift of either sign (inserts in front push the
// source back, removals pull it forward); vec: every array is 16-byte aligned
__device__ void ci_copy_shift(const int32_t* const* old_val, int32_t* const* new_val,
                              int n_payloads, int vec, int64_t M_old, int64_t c0, int64_t c1,
                              int64_t shift) {
  for (int w = 0; w < n_payloads; ++w) {
    const int32_t* src = old_val[w];
    int32_t* dst = new_val[w];
    for (int64_t p = c0 + (int64_t)threadIdx.x * 4; p < c1; p += 4 * CI_NT) {
      const int64_t e = p - shift;
      const int r = (int)(e & 3);
      const int64_t lo = e - r;
      if (vec && p + 4 <= c1 && e >= 0 && lo + 4 <= M_old) {
        const int4 v0 = *reinterpret_cast<const int4*>(src + lo);
        int4 v1 = make_int4(0, 0, 0, 0);
        if (r) {
          if (lo + 8 <= M_old) {
            v1 = *reinterpret_cast<const int4*>(src + lo + 4);
          } else {   // the array ends inside the second word
            v1.x = ci_old(src, lo + 4, M_old);
            v1.y = ci_old(src, lo + 5, M_old);
            v1.z = ci_old(src, lo + 6, M_old);
          }
        }
        int4 o;
        switch (r) {
          case 0: o = v0; break;
          case 1: o = make_int4(v0.y, v0.z, v0.w, v1.x); break;
          case 2: o = make_int4(v0.z, v0.w, v1.x, v1.y); break;
          default: o = make_int4(v0.w, v1.x, v1.y, v1.z); break;
        }
        *reinterpret_cast<int4*>(dst + p) = o;
      } else {
        for (int i = 0; i < 4 && p + i < c1; ++i) dst[p + i] = ci_old(src, e + i, M_old);
      }
    }
  }
}

__global__ __launch_bounds__(CI_NT) void csr_insert_kernel(CsrInsert a) {
  __shared__ int64_t runs[2 * CI_LDS_RUNS];
  const int64_t u0 = (int64_t)blockIdx.x * a.units_per_block;
  const int64_t u1 = u0 + a.units_per_block < a.n_units ? u0 + a.units_per_block : a.n_units;
  if (u0 >= u1) return;
  const int64_t M_new = a.M_old + a.m;
  const int64_t pu1 = u1 < a.n_pay_units ? u1 : a.n_pay_units;
  if (u0 < pu1) {
    // the touched segments [j_lo, j_hi) that reach into this workgroup's positions
    const int64_t p0 = u0 * CI_CHUNK;
    const int64_t p1 = pu1 * CI_CHUNK < M_new ? pu1 * CI_CHUNK : M_new;
    const int64_t j_lo = ci_first(0, a.t, [&](int64_t j) { return ci_ne(a, j) > p0; });
    const int64_t j_hi = ci_first(j_lo, a.t, [&](int64_t j) { return ci_ns(a, j) >= p1; });
    const bool staged = j_hi - j_lo <= CI_LDS_RUNS;   // (the same in every thread)
    if (staged) {
      for (int64_t i = threadIdx.x; i < j_hi - j_lo; i += CI_NT) {
        runs[2 * i] = ci_ns(a, j_lo + i);
        runs[2 * i + 1] = ci_ne(a, j_lo + i);
      }
      __syncthreads();
    }
    auto ns = [&](int64_t j) { return staged ? runs[2 * (j - j_lo)] : ci_ns(a, j); };
    auto ne = [&](int64_t j) { return staged ? runs[2 * (j - j_lo) + 1] : ci_ne(a, j); };
    for (int64_t u = u0; u < pu1; ++u) {
      const int64_t c0 = u * CI_CHUNK;
      const int64_t c1 = c0 + CI_CHUNK < M_new ? c0 + CI_CHUNK : M_new;
      const int64_t cj_lo = ci_first(j_lo, j_hi, [&](int64_t j) { return ne(j) > c0; });
      const int64_t cj_hi = ci_first(cj_lo, j_hi, [&](int64_t j) { return ns(j) >= c1; });
      if (cj_lo == cj_hi) {
        ci_copy_shift(a.old_val, a.new_val, a.n_payloads, a.vec, a.M_old, c0, c1,
                      a.prefix[cj_lo]);
        continue;
      }
      for (int64_t p = c0 + threadIdx.x; p < c1; p += CI_NT) {
        // k: the inserts in front of p; ins: p is insert k itself
        const int64_t jj = ci_first(cj_lo, cj_hi, [&](int64_t j) { return ns(j) > p; });
        int64_t k;
        bool ins = false;
        if (jj == cj_lo) {
          k = a.prefix[cj_lo];
        } else if (p >= ne(jj - 1)) {
          k = a.prefix[jj];
        } else {
          const int64_t q = p - ns(jj - 1);
          const int64_t b1 = a.prefix[jj];
          k = ci_first(a.prefix[jj - 1], b1, [&](int64_t i) { return a.ins_pos[i] >= q; });
          ins = k < b1 && a.ins_pos[k] == q;
        }
        if (ins) k = k < 0 ? 0 : (k >= a.m ? a.m - 1 : k);
        for (int w = 0; w < a.n_payloads; ++w)
          a.new_val[w][p] = ins ? a.ins_val[w][k] : ci_old(a.old_val[w], p - k, a.M_old);
      }
    }
  }
  // new_off[o] = the old start of o + the inserts into owners in front of o
  for (int64_t u = u0 > a.n_pay_units ? u0 : a.n_pay_units; u < u1; ++u) {
    const int64_t o0 = (u - a.n_pay_units) * CI_CHUNK;
    const int64_t o1 = o0 + CI_CHUNK < a.U_new + 1 ? o0 + CI_CHUNK : a.U_new + 1;
    const int64_t lo = ci_first(0, a.t, [&](int64_t j) { return a.touched[j] >= o0; });
    const int64_t hi = ci_first(lo, a.t, [&](int64_t j) { return a.touched[j] >= o1; });
    for (int64_t o = o0 + threadIdx.x; o < o1; o += CI_NT) {
      const int64_t k = ci_first(lo, hi, [&](int64_t j) { return a.touched[j] >= o; });
      a.new_off[o] = ci_old_at(a, o) + (a.t ? a.prefix[k] : 0);
    }
  }
}

// ---- the mirror: a new generation with m entries taken out (dcnr_csr_remove;
// InteractionStore.remove).  The same cut into chunks of output positions with
// the offsets behind them.  An output position p holds old[p + c], c the
// removed positions in front of its source: the first c in [0, m] with c == m
// or removed[c] - c > p (removed[c] - c, the output position the survivors
// behind removed[c] start from, does not descend).  c is constant over a chunk
// no removed position falls into, which is then a shifted copy; the other
// chunks search per element, between the chunk's first and last c.  The
// searches index removed[] below m only and p + c <= M_old - 1 whatever its
// values are (the reads are clamped all the same).
struct CsrRemove {
  const int64_t* old_off;   // [U + 1]
  const int64_t* removed;   // [m] strictly ascending positions of the old payloads
  const int32_t* old_val[2];
  int32_t* new_val[2];
  int64_t* new_off;         // [U + 1]
  int64_t U, M_old, m;
  int64_t n_pay_units, n_units, units_per_block;
  int n_payloads, vec;
};

// the removed positions in front of the source of output position p, in [lo, hi]
__device__ __forceinline__ int64_t cr_front(const CsrRemove& a, int64_t lo, int64_t hi, int64_t p) {
  return ci_first(lo, hi, [&](int64_t c) { return a.removed[c] - c > p; });
}

__global__ __launch_bounds__(CI_NT) void csr_remove_kernel(CsrRemove a) {
  const int64_t u0 = (int64_t)blockIdx.x * a.units_per_block;
  const int64_t u1 = u0 + a.units_per_block < a.n_units ? u0 + a.units_per_block : a.n_units;
  if (u0 >= u1) return;
  const int64_t M_new = a.M_old - a.m;
  const int64_t pu1 = u1 < a.n_pay_units ? u1 : a.n_pay_units;
  if (u0 < pu1) {
    // c of this workgroup's first and last position: every chunk's lie between
    const int64_t p1 = pu1 * CI_CHUNK < M_new ? pu1 * CI_CHUNK : M_new;
    const int64_t g_lo = cr_front(a, 0, a.m, u0 * CI_CHUNK);
    const int64_t g_hi = cr_front(a, g_lo, a.m, p1 - 1);
    for (int64_t u = u0; u < pu1; ++u) {
      const int64_t c0 = u * CI_CHUNK;
      const int64_t c1 = c0 + CI_CHUNK < M_new ? c0 + CI_CHUNK : M_new;
      const int64_t k_lo = cr_front(a, g_lo, g_hi, c0);
      const int64_t k_hi = cr_front(a, k_lo, g_hi, c1 - 1);
      if (k_lo == k_hi) {
        ci_copy_shift(a.old_val, a.new_val, a.n_payloads, a.vec, a.M_old, c0, c1, -k_lo);
        continue;
      }
      for (int64_t p = c0 + threadIdx.x; p < c1; p += CI_NT) {
        const int64_t c = cr_front(a, k_lo, k_hi, p);
        for (int w = 0; w < a.n_payloads; ++w)
          a.new_val[w][p] = ci_old(a.old_val[w], p + c, a.M_old);
      }
    }
  }
  // new_off[o] = the old start of o - the removed positions in front of it
  for (int64_t u = u0 > a.n_pay_units ? u0 : a.n_pay_units; u < u1; ++u) {
    const int64_t o0 = (u - a.n_pay_units) * CI_CHUNK;
    const int64_t o1 = o0 + CI_CHUNK < a.U + 1 ? o0 + CI_CHUNK : a.U + 1;
    for (int64_t o = o0 + threadIdx.x; o < o1; o += CI_NT) {
      const int64_t at = a.old_off[o];
      a.new_off[o] = at - ci_first(0, a.m, [&](int64_t i) { return a.removed[i] >= at; });
    }
  }
}

}  // namespace

// the neighbour source of a call: the table where one is given (nbr), else
// the positives' own top-k lists
template <class F>
static dcnr_status with_neighbours(const int64_t* idx, int k, const int32_t* nbr, int kt, int64_t n_items, F f) {
  return nbr ? f(NbrTable{nbr, kt, n_items}) : f(KnnLists{idx, k});
}

static dcnr_status candidate_union(const int64_t* pos, int64_t Q, const int64_t* idx, int k,
                                   const int32_t* nbr, int kt, int64_t n_items, int64_t* out,
                                   int32_t* out_count, hipStream_t s) {
  if (Q < 0 || k < 1 || Q * k > SV_MAX) {
    set_error("candidate_union: Q*k=%lld exceeds %d", (long long)(Q * k), SV_MAX);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  return with_neighbours(idx, k, nbr, kt, n_items, [&](auto src) {
    hipLaunchKernelGGL(union_kernel<decltype(src)>, dim3(1), dim3(SV_NT), 0, s, pos, Q, src, k, out, out_count);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  });
}

// ---- a batch of R requests: one workgroup per request
// (the MMR's workspace: the ranked lists [R][cap])
struct RequestsWs { int64_t* rrows; float* rscores; };
static RequestsWs requests_ws(Bump& b, int64_t R, int cap) {
  RequestsWs w;
  w.rrows = (int64_t*)b.take((size_t)R * cap * sizeof(int64_t));
  w.rscores = (float*)b.take((size_t)R * cap * sizeof(float));
  return w;
}
static size_t requests_ws_bytes(int64_t R, int cap) {
  Bump b(nullptr);
  requests_ws(b, R, cap);
  return b.off;
}

// ---- requests by user (the interaction store on the device)
static ReqStore req_store(const dcnr_interactions& s) {
  return ReqStore{s.n_reviewers, s.friend_offsets, s.friend_rows, s.n_friend_rows,
                  s.review_offsets, s.review_items, s.review_rows, s.n_reviews};
}

}  // namespace dcnr

using namespace dcnr;

extern "C" {

dcnr_status dcnr_gather_rows(const int64_t* idx, int64_t n, int64_t n_src, int32_t n_arrays,
                             const void* const* src, void* const* dst, const int64_t* row_bytes,
                             dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!src || !dst || !row_bytes || (n > 0 && !idx)) {
    set_error("dcnr_gather_rows: null argument");
    return DCNR_BAD_ARG;
  }
  ProfScope ps(DCNR_K_SERVE, s);
  if (n_arrays < 1 || n_arrays > 8 || n < 0 || n_src < 1) {
    set_error("gather_rows: 1..8 arrays, n_src >= 1");
    return DCNR_BAD_ARG;
  }
  RowGather g;
  g.n = n_arrays;
  for (int a = 0; a < n_arrays; ++a) {
    if (!src[a] || !dst[a] || row_bytes[a] <= 0 || row_bytes[a] % 4) {
      set_error("gather_rows: array %d: null pointer or row bytes %lld not a multiple of 4", a,
                (long long)row_bytes[a]);
      return DCNR_BAD_ARG;
    }
    g.src[a] = (const char*)src[a];
    g.dst[a] = (char*)dst[a];
    g.row_bytes[a] = row_bytes[a];
  }
  if (n == 0) return DCNR_OK;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(n * n_arrays, 4)), dim3(256), 0, s,
                     idx, n, n_src, g);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_candidate_union(const int64_t* positives, int64_t Q, const int64_t* knn_idx,
                                 int32_t k, int64_t* out_rows, int32_t* out_count,
                                 dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (Q < 0 || (Q > 0 && (!positives || !knn_idx || !out_rows || !out_count))) {
    set_error("dcnr_candidate_union: bad argument");
    return DCNR_BAD_ARG;
  }
  if (Q == 0) return DCNR_OK;
  TRYP(DCNR_K_SERVE, s, candidate_union(positives, Q, knn_idx, k, nullptr, 0, 0, out_rows, out_count, s));
  return DCNR_OK;
}

dcnr_status dcnr_candidate_union_table(const int64_t* positives, int64_t Q, const int32_t* nbr,
                                       int32_t kt, int64_t n_items, int32_t k, int64_t* out_rows,
                                       int32_t* out_count, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (Q < 0 || k < 1 || kt < k || n_items < 1 ||
      (Q > 0 && (!positives || !nbr || !out_rows || !out_count))) {
    set_error("dcnr_candidate_union_table: bad argument (Q=%lld, k=%d, kt=%d, n_items=%lld)",
              (long long)Q, k, kt, (long long)n_items);
    return DCNR_BAD_ARG;
  }
  if (Q == 0) return DCNR_OK;
  TRYP(DCNR_K_SERVE, s, candidate_union(positives, Q, nullptr, k, nbr, kt, n_items, out_rows, out_count, s));
  return DCNR_OK;
}

dcnr_status dcnr_ranking_batch(const int64_t* item_rows, int64_t n, int64_t user_row,
                               const int64_t* item_cat, int32_t n_cat, const float* item_num,
                               int32_t n_num, int64_t n_items, int64_t* user_ids,
                               int64_t* item_ids, int64_t* cat_features, float* num_features,
                               dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || n_items < 1 || n_cat < 0 || n_num < 0 ||
      (n > 0 && (!item_rows || !user_ids || !item_ids || (n_cat && (!item_cat || !cat_features)) ||
                 (n_num && (!item_num || !num_features))))) {
    set_error("dcnr_ranking_batch: bad argument");
    return DCNR_BAD_ARG;
  }
  ProfScope ps(DCNR_K_SERVE, s);
  if (n <= 0) return DCNR_OK;
  dim3 blk(16, 16);
  hipLaunchKernelGGL(batch_kernel, dim3((unsigned)cdiv(n, 16)), blk, 0, s, item_rows, n, user_row,
                     item_cat, n_cat, item_num, n_num, n_items, user_ids, item_ids, cat_features,
                     num_features);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_rank_by_score(const float* scores, int64_t n, int64_t* order,
                               dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || (n > 0 && (!scores || !order))) {
    set_error("dcnr_rank_by_score: bad argument");
    return DCNR_BAD_ARG;
  }
  ProfScope ps(DCNR_K_SERVE, s);
  if (n > SV_MAX) {
    set_error("rank_by_score: n=%lld exceeds %d", (long long)n, SV_MAX);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (n <= 0) return DCNR_OK;
  hipLaunchKernelGGL(rank_kernel, dim3(1), dim3(SV_NT), 0, s, scores, (int)n, order);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_mmr_rerank(const float* table, const float* inv_norms, int32_t d,
                            const int64_t* rows, const float* scores, int64_t n,
                            float lambda_param, int32_t top_k, int64_t* out_pos,
                            int32_t* out_count, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || top_k < 1 || (n > 0 && (!table || !inv_norms || !rows || !scores || !out_pos ||
                                       !out_count))) {
    set_error("dcnr_mmr_rerank: bad argument");
    return DCNR_BAD_ARG;
  }
  ProfScope ps(DCNR_K_SERVE, s);
  if (n > SV_MAX || d > 256 || d < 1) {   // (top_k >= 1: checked above)
    set_error("mmr_rerank: n=%lld (max %d), d=%d (max 256), top_k=%d", (long long)n, SV_MAX, d,
              top_k);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (n <= 0) return DCNR_OK;
  // candidate rows staged in LDS when they fit (the same arithmetic, in the
  // same order, as the kernel that re-reads them from the table)
  const size_t lds = mmr_lds_bytes(n, d);
  if (lds <= MMR_LDS_MAX) {
    TRY(set_max_dyn_lds((const void*)mmr_lds_kernel, MMR_LDS_MAX));
    hipLaunchKernelGGL(mmr_lds_kernel, dim3(1), dim3(SV_NT), lds, s, table, inv_norms, d, rows, scores,
                       (int)n, lambda_param, top_k, out_pos, out_count);
  } else {
    hipLaunchKernelGGL(mmr_kernel, dim3(1), dim3(SV_NT), 0, s, table, inv_norms, d, rows, scores, (int)n,
                       lambda_param, top_k, out_pos, out_count);
  }
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

// ---- a batch of requests (the req_* kernels).  Shapes the kernels
// do not take: more requests than DCNR_REQ_MAX_R (one workgroup each), k above
// the top-k's 64, a set CSR of 2^31 rows or more.
namespace {
constexpr int64_t DCNR_REQ_MAX_R = int64_t(1) << 22;

// the checks the three entry points share; DCNR_OK: launch
dcnr_status requests_shape(const char* who, int64_t R, int32_t cap) {
  if (R < 0 || cap < 1 || cap > SV_MAX) {
    set_error("%s: R=%lld (>= 0), cap=%d (1..%d)", who, (long long)R, cap, SV_MAX);
    return DCNR_BAD_ARG;
  }
  if (R > DCNR_REQ_MAX_R) {
    set_error("%s: R=%lld exceeds %lld requests per call", who, (long long)R,
              (long long)DCNR_REQ_MAX_R);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  return DCNR_OK;
}
}  // namespace

size_t dcnr_requests_workspace_size(int64_t R, int64_t Q_total, int32_t k, int32_t cap) {
  if (R <= 0 || R > DCNR_REQ_MAX_R || Q_total < 0 || k < 1 || cap < 1 || cap > SV_MAX)
    return 0;
  return requests_ws_bytes(R, cap) + 256;
}

namespace {
// dcnr_requests_candidates and its table form: neighbours from knn_idx
// [Q_total][k], or (nbr != null) from the item neighbour table [n_items][kt]
dcnr_status requests_candidates_api(const char* who, const int64_t* positives,
                                    const int64_t* pos_offsets, int64_t R, int64_t Q_total,
                                    const int64_t* knn_idx, const int32_t* nbr, int32_t kt, int32_t k,
                                    const int64_t* set_rows, int64_t n_set_rows,
                                    const int64_t* set_offsets, int32_t S, const int32_t* allowed,
                                    const int32_t* excluded, const int32_t* fallback,
                                    int32_t min_candidates, int64_t n_items, int32_t cap,
                                    int64_t* out_rows, int32_t* out_count, int32_t* status,
                                    int64_t* offsets, int64_t* host_offsets, int32_t* host_status,
                                    hipStream_t s) {
  TRY(requests_shape(who, R, cap));
  if (Q_total < 0 || k < 1 || S < 0 || n_set_rows < 0 || n_items < 1) {
    set_error("%s: Q_total=%lld, k=%d, S=%d, n_set_rows=%lld, n_items=%lld", who,
              (long long)Q_total, k, S, (long long)n_set_rows, (long long)n_items);
    return DCNR_BAD_ARG;
  }
  if (R > 0 && (!pos_offsets || !out_rows || !out_count || !status || !offsets ||
                (Q_total > 0 && (!positives || (!knn_idx && !nbr))) || (S > 0 && !set_offsets) ||
                (n_set_rows > 0 && !set_rows) ||
                (S == 0 && (allowed || excluded || fallback)))) {
    set_error("%s: null argument (or set indices without sets)", who);
    return DCNR_BAD_ARG;
  }
  if (k > 64 || n_set_rows > INT32_MAX) {
    set_error("%s: k=%d (max 64), n_set_rows=%lld (max 2^31 - 1)", who, k, (long long)n_set_rows);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (R == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  ReqSets st{set_rows, n_set_rows, set_offsets, S, allowed, excluded, fallback};
  TRY(with_neighbours(knn_idx, k, nbr, kt, n_items, [&](auto src) {
    hipLaunchKernelGGL(req_candidates_kernel<decltype(src)>, dim3((unsigned)R), dim3(SV_NT), 0, s, positives,
                       pos_offsets, R, Q_total, src, k, st, min_candidates, n_items, cap, out_rows,
                       out_count, status);
    DCNR_LAUNCH_CHECK();
    return DCNR_OK;
  }));
  hipLaunchKernelGGL(req_offsets_kernel, dim3(1), dim3(SV_NT), 0, s, out_count, status, R, cap, offsets,
                     host_offsets, host_status);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}
}  // namespace

dcnr_status dcnr_requests_candidates(const int64_t* positives, const int64_t* pos_offsets,
                                     int64_t R, int64_t Q_total, const int64_t* knn_idx, int32_t k,
                                     const int64_t* set_rows, int64_t n_set_rows,
                                     const int64_t* set_offsets, int32_t S, const int32_t* allowed,
                                     const int32_t* excluded, const int32_t* fallback,
                                     int32_t min_candidates, int64_t n_items, int32_t cap,
                                     int64_t* out_rows, int32_t* out_count, int32_t* status,
                                     int64_t* offsets, int64_t* host_offsets,
                                     int32_t* host_status, dcnr_stream_t stream) {
  return requests_candidates_api("dcnr_requests_candidates", positives, pos_offsets, R, Q_total,
                                 knn_idx, nullptr, 0, k, set_rows, n_set_rows, set_offsets, S, allowed,
                                 excluded, fallback, min_candidates, n_items, cap, out_rows, out_count,
                                 status, offsets, host_offsets, host_status, (hipStream_t)stream);
}

dcnr_status dcnr_requests_candidates_table(const int64_t* positives, const int64_t* pos_offsets,
                                           int64_t R, int64_t Q_total, const int32_t* nbr, int32_t kt,
                                           int32_t k, const int64_t* set_rows, int64_t n_set_rows,
                                           const int64_t* set_offsets, int32_t S,
                                           const int32_t* allowed, const int32_t* excluded,
                                           const int32_t* fallback, int32_t min_candidates,
                                           int64_t n_items, int32_t cap, int64_t* out_rows,
                                           int32_t* out_count, int32_t* status, int64_t* offsets,
                                           int64_t* host_offsets, int32_t* host_status,
                                           dcnr_stream_t stream) {
  if (kt < k || (R > 0 && Q_total > 0 && !nbr)) {
    set_error("dcnr_requests_candidates_table: kt=%d below k=%d, or a null table", kt, k);
    return DCNR_BAD_ARG;
  }
  return requests_candidates_api("dcnr_requests_candidates_table", positives, pos_offsets, R, Q_total,
                                 nullptr, nbr, kt, k, set_rows, n_set_rows, set_offsets, S, allowed,
                                 excluded, fallback, min_candidates, n_items, cap, out_rows, out_count,
                                 status, offsets, host_offsets, host_status, (hipStream_t)stream);
}

dcnr_status dcnr_requests_ranking_batch(const int64_t* cand_rows, int32_t cap,
                                        const int64_t* offsets, int64_t R, int64_t n,
                                        const int64_t* user_rows, const int64_t* item_cat,
                                        int32_t n_cat, const float* item_num, int32_t n_num,
                                        int64_t n_items, int64_t* user_ids, int64_t* item_ids,
                                        int64_t* cat_features, float* num_features,
                                        dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  TRY(requests_shape("dcnr_requests_ranking_batch", R, cap));
  if (n < 0 || n > R * cap || n_items < 1 || n_cat < 0 || n_num < 0 ||
      (n > 0 && (!cand_rows || !offsets || !user_rows || !user_ids || !item_ids ||
                 (n_cat && (!item_cat || !cat_features)) ||
                 (n_num && (!item_num || !num_features))))) {
    set_error("dcnr_requests_ranking_batch: bad argument (n=%lld of at most R*cap=%lld)",
              (long long)n, (long long)(R * cap));
    return DCNR_BAD_ARG;
  }
  if (R == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  if (n <= 0) return DCNR_OK;
  dim3 blk(16, 16);
  hipLaunchKernelGGL(req_batch_kernel, dim3((unsigned)cdiv(n, 16)), blk, 0, s, cand_rows, cap, offsets,
                     R, n, user_rows, item_cat, n_cat, item_num, n_num, n_items, user_ids, item_ids,
                     cat_features, num_features);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_requests_rank_mmr(const float* logits, int64_t n, const int64_t* cand_rows,
                                   int32_t cap, const int64_t* offsets, int64_t R,
                                   const float* table, const float* inv_norms, int32_t d,
                                   int64_t n_items, const float* lambda_param,
                                   const int32_t* top_k, int64_t* out_rows, float* out_logits,
                                   int32_t* out_count, int32_t* status, void* ws, size_t ws_bytes,
                                   dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  TRY(requests_shape("dcnr_requests_rank_mmr", R, cap));
  if (n < 0 || n > R * cap || d < 1 || d > 256 || n_items < 1 ||
      (R > 0 && (!cand_rows || !offsets || !table || !inv_norms || !lambda_param || !top_k ||
                 !out_count || !status || !ws || (n > 0 && (!logits || !out_rows || !out_logits))))) {
    set_error("dcnr_requests_rank_mmr: bad argument (n=%lld of at most R*cap=%lld, d=%d of 1..256)",
              (long long)n, (long long)(R * cap), d);
    return DCNR_BAD_ARG;
  }
  if (R == 0) return DCNR_OK;
  const size_t need = requests_ws_bytes(R, cap) + 256;
  if (ws_bytes < need) {
    set_error("dcnr_requests_rank_mmr: workspace too small: %zu < %zu", ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  Bump b((void*)(((uintptr_t)ws + 255) & ~(uintptr_t)255));
  const RequestsWs w = requests_ws(b, R, cap);
  ProfScope ps(DCNR_K_SERVE, s);
  TRY(set_max_dyn_lds((const void*)req_rank_mmr_kernel, MMR_LDS_MAX));
  hipLaunchKernelGGL(req_rank_mmr_kernel, dim3((unsigned)R), dim3(SV_NT), MMR_LDS_MAX, s, logits, n,
                     cand_rows, cap, offsets, R, table, inv_norms, d, n_items, lambda_param, top_k,
                     w.rrows, w.rscores, out_rows, out_logits, out_count, status);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

// ---- requests by user.  The store's lengths are checked here; what lies in
// device memory (offsets, rows) the kernels check against them.
namespace {
constexpr int64_t DCNR_STORE_MAX_ITEMS = int64_t(1) << 29;   // hotel row * 4 + class bits in 32

dcnr_status store_shape(const char* who, const dcnr_interactions* st, int64_t n_items) {
  if (!st || st->n_reviewers < 0 || st->n_friend_rows < 0 || st->n_reviews < 0 || n_items < 1 ||
      !st->friend_offsets || !st->review_offsets || (st->n_friend_rows > 0 && !st->friend_rows) ||
      (st->n_reviews > 0 && (!st->review_items || !st->review_rows))) {
    set_error("%s: null or negative store field, or n_items < 1", who);
    return DCNR_BAD_ARG;
  }
  if (n_items > DCNR_STORE_MAX_ITEMS || st->n_reviewers >= INT32_MAX ||
      st->n_reviews > INT32_MAX || st->n_friend_rows > INT32_MAX) {
    set_error("%s: n_items=%lld (max 2^29), n_reviewers=%lld, n_reviews=%lld, n_friend_rows=%lld "
              "(max 2^31 - 1)", who, (long long)n_items, (long long)st->n_reviewers,
              (long long)st->n_reviews, (long long)st->n_friend_rows);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  return DCNR_OK;
}
}  // namespace

dcnr_status dcnr_requests_sources(const dcnr_interactions* store, const int32_t* reviewers,
                                  const int32_t* modes, int64_t R, int64_t n_items,
                                  const int64_t* pos_offsets, int64_t Q_total, int64_t* positives,
                                  const int64_t* neg_offsets, int64_t neg_lo, int64_t neg_hi,
                                  int64_t* neg_rows, int32_t* counts, int32_t* status,
                                  int32_t* host_counts, int32_t* host_status,
                                  dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  TRY(requests_shape("dcnr_requests_sources", R, 1));
  TRY(store_shape("dcnr_requests_sources", store, n_items));
  if (Q_total < 0 || neg_lo < 0 || neg_hi < neg_lo ||
      (R > 0 && (!reviewers || !modes || !pos_offsets || !neg_offsets || !counts || !status ||
                 (Q_total > 0 && !positives) || (neg_hi > neg_lo && !neg_rows)))) {
    set_error("dcnr_requests_sources: bad argument (Q_total=%lld, negatives [%lld, %lld))",
              (long long)Q_total, (long long)neg_lo, (long long)neg_hi);
    return DCNR_BAD_ARG;
  }
  if (R == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  hipLaunchKernelGGL(req_sources_kernel, dim3((unsigned)R), dim3(SV_NT), 0, s, req_store(*store),
                     reviewers, modes, R, n_items, pos_offsets, Q_total, positives, neg_offsets, neg_lo,
                     neg_hi, neg_rows, counts, status, host_counts, host_status);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_requests_recommended_by(const dcnr_interactions* store, const int32_t* reviewers,
                                         int64_t R, int64_t n_items, const int64_t* out_rows,
                                         int64_t n, const int64_t* offsets,
                                         const int32_t* out_count, const int64_t* list_offsets,
                                         int64_t n_list_rows, int32_t* lists, int32_t* by_count,
                                         int64_t* by_offsets, int32_t* by_reviewers,
                                         int32_t* status, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  TRY(requests_shape("dcnr_requests_recommended_by", R, 1));
  TRY(store_shape("dcnr_requests_recommended_by", store, n_items));
  if (n < 0 || n > R * SV_MAX || n_list_rows < 0 ||
      (R > 0 && (!reviewers || !offsets || !out_count || !list_offsets || !by_offsets || !status ||
                 (n > 0 && (!out_rows || !by_count)) ||
                 (n_list_rows > 0 && (!lists || !by_reviewers))))) {
    set_error("dcnr_requests_recommended_by: bad argument (n=%lld, n_list_rows=%lld)",
              (long long)n, (long long)n_list_rows);
    return DCNR_BAD_ARG;
  }
  if (R == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  // (positions no valid segment covers count 0)
  if (n > 0) TRY(fill_zero(by_count, (size_t)n * sizeof(int32_t), s));
  hipLaunchKernelGGL(req_recommended_by_kernel, dim3((unsigned)R), dim3(SV_NT), 0, s,
                     req_store(*store), reviewers, R, n_items, out_rows, n, offsets, out_count,
                     list_offsets, n_list_rows, lists, by_count, status);
  DCNR_LAUNCH_CHECK();
  // by_off = the exclusive sum of by_count over the n positions
  hipLaunchKernelGGL(req_offsets_kernel, dim3(1), dim3(SV_NT), 0, s, by_count,
                     (const int32_t*)nullptr, n, INT_MAX, by_offsets, (int64_t*)nullptr,
                     (int32_t*)nullptr);
  DCNR_LAUNCH_CHECK();
  const int64_t threads = n > n_list_rows ? n : n_list_rows;
  if (threads > 0) {
    hipLaunchKernelGGL(req_by_gather_kernel, dim3((unsigned)cdiv(threads, 256)), dim3(256), 0, s,
                       lists, list_offsets, n_list_rows, offsets, R, n, by_count, by_offsets, by_reviewers);
    DCNR_LAUNCH_CHECK();
  }
  return DCNR_OK;
}

dcnr_status dcnr_csr_insert(const int64_t* old_offsets, int64_t n_old_owners, int64_t n_new_owners,
                            int64_t n_old_entries, int32_t n_payloads,
                            const int32_t* const* old_payloads, const int64_t* touched,
                            const int64_t* insert_prefix, int64_t t, const int64_t* insert_pos,
                            const int32_t* const* insert_payloads, int64_t m, int64_t* new_offsets,
                            int32_t* const* new_payloads, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  bool bad = !old_offsets || !new_offsets || n_old_owners < 0 || n_new_owners < n_old_owners ||
             n_old_entries < 0 || n_payloads < 1 || n_payloads > 2 || t < 0 || m < 0 || t > m ||
             (m > 0 && (t == 0 || !touched || !insert_prefix || !insert_pos || !old_payloads ||
                        !insert_payloads || !new_payloads));
  for (int w = 0; !bad && m > 0 && w < n_payloads; ++w)
    bad = !insert_payloads[w] || !new_payloads[w] || (n_old_entries > 0 && !old_payloads[w]);
  if (bad) {
    set_error("dcnr_csr_insert: bad argument (owners %lld -> %lld, entries=%lld, payloads=%d, "
              "t=%lld, m=%lld)", (long long)n_old_owners, (long long)n_new_owners,
              (long long)n_old_entries, n_payloads, (long long)t, (long long)m);
    return DCNR_BAD_ARG;
  }
  if (m == 0 && n_new_owners == n_old_owners) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  CsrInsert a;
  a.old_off = old_offsets; a.touched = touched; a.prefix = insert_prefix; a.ins_pos = insert_pos;
  a.new_off = new_offsets;
  a.U_old = n_old_owners; a.U_new = n_new_owners; a.M_old = n_old_entries; a.m = m; a.t = t;
  a.n_payloads = n_payloads;
  a.vec = 1;
  for (int w = 0; w < 2; ++w) {
    const bool on = w < n_payloads && m > 0;
    a.old_val[w] = on ? old_payloads[w] : nullptr;
    a.ins_val[w] = on ? insert_payloads[w] : nullptr;
    a.new_val[w] = on ? new_payloads[w] : nullptr;
    if (((uintptr_t)a.old_val[w] | (uintptr_t)a.new_val[w]) & 15) a.vec = 0;
  }
  // without inserts the payloads are the old generation's: the offsets only
  a.n_pay_units = m > 0 ? cdiv(n_old_entries + m, CI_CHUNK) : 0;
  a.n_units = a.n_pay_units + cdiv(n_new_owners + 1, CI_CHUNK);
  int64_t grid = a.n_units < CI_MAX_BLOCKS ? a.n_units : CI_MAX_BLOCKS;
  a.units_per_block = cdiv(a.n_units, grid);
  grid = cdiv(a.n_units, a.units_per_block);
  hipLaunchKernelGGL(csr_insert_kernel, dim3((unsigned)grid), dim3(CI_NT), 0, s, a);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

dcnr_status dcnr_csr_remove(const int64_t* old_offsets, int64_t n_owners, int64_t n_old_entries,
                            int32_t n_payloads, const int32_t* const* old_payloads,
                            const int64_t* removed, int64_t m, int64_t* new_offsets,
                            int32_t* const* new_payloads, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool pay = m > 0 && m < n_old_entries;   // some payload words are copied
  bool bad = !old_offsets || !new_offsets || n_owners < 0 || n_old_entries < 0 || n_payloads < 1 ||
             n_payloads > 2 || m < 0 || m > n_old_entries || (m > 0 && !removed) ||
             (pay && (!old_payloads || !new_payloads));
  for (int w = 0; !bad && pay && w < n_payloads; ++w) bad = !old_payloads[w] || !new_payloads[w];
  if (bad) {
    set_error("dcnr_csr_remove: bad argument (owners=%lld, entries=%lld, payloads=%d, m=%lld)",
              (long long)n_owners, (long long)n_old_entries, n_payloads, (long long)m);
    return DCNR_BAD_ARG;
  }
  if (m == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  CsrRemove a;
  a.old_off = old_offsets; a.removed = removed; a.new_off = new_offsets;
  a.U = n_owners; a.M_old = n_old_entries; a.m = m;
  a.n_payloads = n_payloads;
  a.vec = 1;
  for (int w = 0; w < 2; ++w) {
    const bool on = w < n_payloads && m < n_old_entries;
    a.old_val[w] = on ? old_payloads[w] : nullptr;
    a.new_val[w] = on ? new_payloads[w] : nullptr;
    if (((uintptr_t)a.old_val[w] | (uintptr_t)a.new_val[w]) & 15) a.vec = 0;
  }
  // with every entry removed there are no payloads to write: the offsets only
  a.n_pay_units = cdiv(n_old_entries - m, CI_CHUNK);
  a.n_units = a.n_pay_units + cdiv(n_owners + 1, CI_CHUNK);
  int64_t grid = a.n_units < CI_MAX_BLOCKS ? a.n_units : CI_MAX_BLOCKS;
  a.units_per_block = cdiv(a.n_units, grid);
  grid = cdiv(a.n_units, a.units_per_block);
  hipLaunchKernelGGL(csr_remove_kernel, dim3((unsigned)grid), dim3(CI_NT), 0, s, a);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // extern "C"
