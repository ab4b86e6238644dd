// Device building blocks the two request lanes share (serving.hip: one
// workgroup per request, up to SV_MAX entries; serving_large.hip: grids over
// the entries of the requests above that).  One copy of each, so a request's
// answer is the same bits in either lane: the neighbour sources, the row-set
// CSR and its binary search, a ranking batch's row, and the greedy MMR's
// arithmetic (mmr_sim / mmr_value / mmr_better / block_argmax) with both its
// forms (mmr_table, mmr_lds).
#pragma once
#include "dcnr_internal.h"

#include <cfloat>
#include <climits>

namespace dcnr {
namespace {

constexpr int SV_NT = 1024;
constexpr int SV_MAX = 4096;   // max candidates per call (LDS sort capacity)

// Where a positive's neighbours come from: the top-k lists of this call's
// positives (KnnLists: idx [Q][k], row q for positive q), or the item
// neighbour table built at fit time (NbrTable: nbr [n_items][kt] int32, row p
// for the hotel p, its first k entries).  at(q, p, j, bad): neighbour j >= 1
// of positive number q, the hotel p; sets bad where the table cannot answer.
// positive(p, bad): the positive itself, position 0 of its list.
struct KnnLists {
  const int64_t* idx; int k;
  __device__ KnnLists from(int64_t q0) const { return {idx + q0 * k, k}; }
  __device__ int64_t positive(int64_t p, bool&) const { return p; }
  __device__ int64_t at(int64_t q, int64_t, int j, bool&) const { return idx[q * k + j]; }
};
struct NbrTable {
  const int32_t* nbr; int kt; int64_t n_items;
  __device__ NbrTable from(int64_t) const { return *this; }
  __device__ int64_t positive(int64_t p, bool& bad) const {
    if (p >= n_items) bad = true;
    return p;
  }
  // a negative positive is skipped with its neighbours, as the positive
  // itself is (dcnr_requests_sources pads with -1); one past the table has no
  // row to read, and an entry outside the table is no hotel (the table holds
  // no padding): both are bad data
  __device__ int64_t at(int64_t, int64_t p, int j, bool& bad) const {
    if (p < 0) return -1;
    if (p >= n_items) { bad = true; return -1; }
    const int64_t v = nbr[p * kt + j];
    if (v < 0 || v >= n_items) bad = true;
    return v;
  }
};

// entry t of a request's staged list: positives[q] at j = 0, else neighbour
// j of positive q (t = q * k + j); rows < 0 are skipped (INT64_MAX)
template <class Src>
__device__ __forceinline__ int64_t union_entry(const int64_t* pos, const Src& src, int k, int t, bool& bad) {
  const int64_t q = t / k;
  const int j = t % k;
  const int64_t p = pos[q];
  const int64_t r = j == 0 ? src.positive(p, bad) : src.at(q, p, j, bad);
  return r < 0 ? INT64_MAX : r;
}

// is v in the ascending distinct set[0 .. len)?
__device__ __forceinline__ bool set_contains(const int64_t* set, int64_t len, int64_t v) {
  int64_t lo = 0, hi = len;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (set[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo < len && set[lo] == v;
}

// The row sets a batch of requests names (the city's hotels, its popular
// hotels, a user's negative reviews ...): a CSR of S ascending distinct sets
// and three indices per request, -1 = none (a null index array = none at all)
struct ReqSets {
  const int64_t* rows; int64_t n_rows;
  const int64_t* off; int S;
  const int32_t* allowed; const int32_t* excluded; const int32_t* fallback;
};

constexpr int32_t REQ_OVERFLOW = 1, REQ_BAD_DATA = 2;   // dcnr.h: DCNR_REQ_*

// set `which[r]` of the CSR as (first row, length); false: an index or an
// offset pair outside the CSR
__device__ bool req_set(const ReqSets& st, const int32_t* which, int64_t r, const int64_t*& rows,
                        int64_t& len) {
  rows = nullptr;
  len = -1;   // none
  const int32_t s = which ? which[r] : -1;
  if (s == -1) return true;
  if (s < -1 || s >= st.S) return false;
  const int64_t lo = st.off[s], hi = st.off[s + 1];
  if (lo < 0 || hi < lo || hi > st.n_rows || hi - lo > INT_MAX) return false;
  rows = st.rows + lo;
  len = hi - lo;
  return true;
}

// one row of a ranking batch: user_out[i] = user_row, item_out[i] = row,
// cat_out[i][:] = item_cat[row][:], num_out[i][:] = item_num[row][:] (the
// gathers clamp the row into the tables), by the blockDim.x threads of row i
__device__ __forceinline__ void batch_row(int64_t i, int64_t row, int64_t user_row,
                                          const int64_t* item_cat, int K, const float* item_num,
                                          int F, int64_t n_items, int64_t* user_out,
                                          int64_t* item_out, int64_t* cat_out, float* num_out) {
  const int64_t r = row < 0 ? 0 : (row >= n_items ? n_items - 1 : row);
  if (threadIdx.x == 0) { user_out[i] = user_row; item_out[i] = row; }
  for (int c = threadIdx.x; c < K; c += blockDim.x) cat_out[i * K + c] = item_cat[r * K + c];
  for (int c = threadIdx.x; c < F; c += blockDim.x) num_out[i * F + c] = item_num[r * F + c];
}

// block argmax of (v, -pos): highest v, lowest position on ties
__device__ void block_argmax(float v, int p, float* sv, int* sp, float& bv, int& bp) {
  // wave level
  for (int o = 32; o >= 1; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int op = __shfl_xor(p, o, 64);
    if (ov > v || (ov == v && op < p)) { v = ov; p = op; }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sv[w] = v; sp[w] = p; }
  __syncthreads();
  bv = sv[0];
  bp = sp[0];
  for (int i = 1; i < SV_NT / 64; ++i)
    if (sv[i] > bv || (sv[i] == bv && sp[i] < bp)) { bv = sv[i]; bp = sp[i]; }
  __syncthreads();
}

// Greedy MMR over n candidates in ranked order (rerank_with_mmr, main.py:133-169).
// rows[i] = embedding row of candidate i or -1 (no embedding: never picked
// after the first, contributes no similarity).  sim = cosine similarity
// (zero-norm rows -> 0, as sklearn's normalize + dot).  The first candidate is
// always taken; then up to min(top_k, n) - 1 more while some candidate is
// eligible.  Max-similarity is 0 while no selected item has an embedding.
//
// The building blocks of both forms (candidates' rows re-read from the table,
// or staged in LDS) and of both callers (one request, a batch of them):

// cosine similarity of a candidate (raw row, inverse norm rinv) to the
// selected item (raw row sel, inverse norm is): the sum in c order of
// row[c] * (sel[c] * is), then * rinv
__device__ __forceinline__ float mmr_sim(const float* row, float rinv, const float* sel, float is,
                                         int d) {
  float s = 0.f;
  for (int c = 0; c < d; ++c) s += row[c] * (sel[c] * is);
  return s * rinv;
}

// the MMR value of a candidate; its max similarity counts as 0 while no
// selected item has an embedding (sel false)
__device__ __forceinline__ float mmr_value(float lambda, float score, bool sel, float maxsim) {
  return lambda * score - (1.f - lambda) * (sel ? maxsim : 0.f);
}

// a thread's running best (v, p): higher value first, lower position on ties
__device__ __forceinline__ void mmr_better(float m, int t, float& v, int& p) {
  if (p == INT_MAX || m > v || (m == v && t < p)) { v = m; p = t; }
}

// The table-reading form.  maxsim [n], taken [n] are the workgroup's scratch
// (LDS, or global memory where n candidates do not fit: each element of
// maxsim belongs to one thread, taken changes between barriers only), selv [d]
// is in LDS; emit(i, p), called by thread 0, records that the i-th item
// of the result is candidate p.  Returns the number of items, in every thread.
template <typename Emit>
__device__ int mmr_table(const float* table, const float* inv, int d, const int64_t* rows,
                         const float* scores, int n, float lambda, int top_k, float* maxsim,
                         unsigned char* taken, float* selv, Emit emit) {
  __shared__ float sv[SV_NT / 64];
  __shared__ int sp[SV_NT / 64];
  __shared__ int any_sel;
  for (int t = threadIdx.x; t < n; t += SV_NT) { maxsim[t] = -FLT_MAX; taken[t] = 0; }
  if (threadIdx.x == 0) { any_sel = 0; taken[0] = 1; emit(0, 0); }   // (thread 0 owns t = 0)
  __syncthreads();
  const int want = min(top_k, n);
  int cnt = 1, last = 0;
  for (;;) {
    // fold the last selected item into every candidate's max similarity
    const int64_t sr = rows[last];
    if (sr >= 0) {
      const float is = inv[sr];
      for (int t = threadIdx.x; t < d; t += SV_NT) selv[t] = table[sr * d + t];
      __syncthreads();
      for (int t = threadIdx.x; t < n; t += SV_NT) {
        const int64_t r = rows[t];
        if (r < 0 || taken[t]) continue;
        maxsim[t] = fmaxf(maxsim[t], mmr_sim(table + r * d, inv[r], selv, is, d));
      }
      if (threadIdx.x == 0) any_sel = 1;
      __syncthreads();
    }
    if (cnt >= want) break;
    float v = -FLT_MAX;
    int p = INT_MAX;
    const bool sel = any_sel != 0;
    for (int t = threadIdx.x; t < n; t += SV_NT) {
      if (taken[t] || rows[t] < 0) continue;
      mmr_better(mmr_value(lambda, scores[t], sel, maxsim[t]), t, v, p);
    }
    float bv;
    int bp;
    block_argmax(v, p, sv, sp, bv, bp);
    if (bp == INT_MAX) break;
    if (threadIdx.x == 0) { taken[bp] = 1; emit(cnt, bp); }
    __syncthreads();
    ++cnt;
    last = bp;
  }
  return cnt;
}

constexpr size_t MMR_LDS_MAX = 152 * 1024;   // dynamic LDS of mmr_lds_kernel (+ ~4 KiB static)

// The same greedy MMR with everything a selection round touches on chip:
// the candidates' raw rows (stride d+1: one row per thread, conflict-free)
// and inverse norms in LDS, each thread's candidates (t = tid + j*SV_NT) --
// validity, score, max similarity, taken -- in registers, so a round is one
// dot product per candidate and a block argmax (its two barriers), with no
// global loads.  Arithmetic as in mmr_table (mmr_sim, mmr_value, mmr_better).
// lds_rows [n (d + 1) + n] floats and vld [n] are workgroup scratch in LDS;
// emit and the result as in mmr_table.
template <typename Emit>
__device__ int mmr_lds(const float* table, const float* inv, int d, const int64_t* rows,
                       const float* scores, int n, float lambda, int top_k, float* lds_rows,
                       unsigned char* vld, Emit emit) {
  constexpr int MR = SV_MAX / SV_NT;   // candidates per thread
  __shared__ float sv[SV_NT / 64];
  __shared__ int sp[SV_NT / 64];
  float* invs = lds_rows + (size_t)n * (d + 1);
  for (int e = threadIdx.x; e < n * d; e += SV_NT) {
    const int t = e / d, c = e - t * d;
    const int64_t r = rows[t];
    lds_rows[t * (d + 1) + c] = r >= 0 ? table[r * d + c] : 0.f;
  }
  bool ok[MR], tk[MR];
  float sc[MR], ms[MR];
#pragma unroll
  for (int j = 0; j < MR; ++j) {
    const int t = threadIdx.x + j * SV_NT;
    const int64_t r = t < n ? rows[t] : -1;
    ok[j] = r >= 0;
    tk[j] = t == 0;
    sc[j] = t < n ? scores[t] : 0.f;
    ms[j] = -FLT_MAX;
    if (t < n) {
      invs[t] = r >= 0 ? inv[r] : 0.f;
      vld[t] = r >= 0;
    }
  }
  if (threadIdx.x == 0) emit(0, 0);
  __syncthreads();
  const int want = min(top_k, n);
  int cnt = 1, last = 0;
  bool sel = false;
  for (;;) {
    // fold the last selected item into every candidate's max similarity
    if (vld[last]) {
      const float is = invs[last];
      const float* sr = lds_rows + last * (d + 1);
#pragma unroll
      for (int j = 0; j < MR; ++j) {
        const int t = threadIdx.x + j * SV_NT;
        if (t >= n || !ok[j] || tk[j]) continue;
        ms[j] = fmaxf(ms[j], mmr_sim(lds_rows + t * (d + 1), invs[t], sr, is, d));
      }
      sel = true;
    }
    if (cnt >= want) break;
    float v = -FLT_MAX;
    int p = INT_MAX;
#pragma unroll
    for (int j = 0; j < MR; ++j) {
      const int t = threadIdx.x + j * SV_NT;
      if (t >= n || tk[j] || !ok[j]) continue;
      mmr_better(mmr_value(lambda, sc[j], sel, ms[j]), t, v, p);
    }
    float bv;
    int bp;
    block_argmax(v, p, sv, sp, bv, bp);
    if (bp == INT_MAX) break;
    if (bp % SV_NT == (int)threadIdx.x) tk[bp / SV_NT] = true;   // the owner thread
    if (threadIdx.x == 0) emit(cnt, bp);
    ++cnt;
    last = bp;
  }
  return cnt;
}

// does the LDS-resident form hold n candidates of width d?
__host__ __device__ inline size_t mmr_lds_bytes(int64_t n, int d) {
  return ((size_t)n * (d + 1) + (size_t)n) * sizeof(float);
}

}  // namespace
}  // namespace dcnr
