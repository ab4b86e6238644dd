// The fitted preprocessing applied to rows it was not fitted on
// (preprocess_for_ranking, main.py:215-230, and train.py's order of steps): a
// raw-id dictionary on the device (dcnr_id_map_build, dcnr_id_map_lookup) and
// dcnr_rows_transform, from raw review columns and a fit's ids, category keys,
// medians and scaler to (collab, cat, num, y).  The contract is in
// include/dcnr.h; DESIGN.md section 9 has the why.
//
//   id map   open addressing over 16-byte slots {key, index}: a probe is one
//            128-bit load.  The build claims a slot with a compare-and-swap on
//            its key word and then stores the index; lookups run in later
//            kernels and only read.  Every probe loop ends after `capacity`
//            slots: a full table sets DCNR_REQ_OVERFLOW and the lane returns.
//   insert   dcnr_id_map_insert admits ids the table does not hold.  find: a
//            read-only lookup settles the known rows and sees the reserved id
//            before anything is written.  claim: a row with an unknown id
//            claims its slot's key word by compare-and-swap (or finds it
//            claimed by a row with the same id) and takes an integer atomicMin
//            of its row number on the slot's index word.  mark, scan: a row
//            that finds its own number there is its id's first appearance; the
//            sum scan of those marks numbers the new ids in first-appearance
//            order.  head: the first rows write the index word and new_ids.
//            rest: the other rows read it.  Which slot an id lands in depends
//            on which lane wins a probe chain, as in the build; out, new_ids
//            and the count do not -- no atomic decides a number.
//   flags    one lane per input row: the filter, the two id probes and the
//            category binary searches; keep[i] and the count words (a ballot
//            per counter, LDS adds, one global integer add per workgroup)
//   scan     an inclusive scan of keep (tile sums, one workgroup over the tile
//            sums, tiles again): a row's output position is the number of kept
//            rows before it -- no atomic decides a position
//   emit     one lane per kept row: the lookups again (the tables are read-
//            only and cache-resident; no per-row scratch is written and read
//            back), the derived columns, the NaN fill, the scaler, y
//
// Every atomic is an integer add, or, min or compare-and-swap: the same results
// on every run (the id map's slot positions aside).
#include "device_prims.h"

namespace dcnr {

namespace {

using namespace tscan;

constexpr int RT_NT = 256;
constexpr int RT_MAXB = 4096;                 // workgroups of the grid-stride kernels
constexpr int RT_MAXCAT = 62;                 // category columns: bits 2 .. 63 of unknown_bits
constexpr int64_t ID_EMPTY = INT64_MIN;       // the reserved id: an empty slot

struct alignas(16) Slot {
  int64_t key;
  int64_t index;
};

struct CatOff { int64_t off[RT_MAXCAT + 1]; };

// splitmix64's finalizer: every input bit reaches every output bit, so ids that
// agree in their low 32 bits, or are all multiples of 2^32, spread over the table
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// the index of q, or -1; at most `cap` probes
__device__ __forceinline__ int64_t map_find(const Slot* t, int64_t cap, int64_t q) {
  if (q == ID_EMPTY) return -1;
  const uint64_t mask = (uint64_t)cap - 1ull;
  uint64_t s = mix64((uint64_t)q) & mask;
  for (int64_t p = 0; p < cap; ++p) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(t + s);   // key and index: one load
    if ((int64_t)v.x == q) return (int64_t)v.y;
    if ((int64_t)v.x == ID_EMPTY) return -1;
    s = (s + 1ull) & mask;
  }
  return -1;
}

// ---------------------------------------------------------------- id map
__global__ __launch_bounds__(RT_NT) void im_clear_kernel(Slot* t, int64_t cap, int32_t* status) {
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < cap; i += step) {
    Slot e;
    e.key = ID_EMPTY;
    e.index = -1;
    t[i] = e;
  }
  if (i0 == 0) *status = 0;
}

__global__ __launch_bounds__(RT_NT) void im_insert_kernel(const int64_t* ids, int64_t n, Slot* t, int64_t cap,
                                                          int32_t* status) {
  const uint64_t mask = (uint64_t)cap - 1ull;
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < n; i += step) {
    const int64_t id = ids[i];
    if (id == ID_EMPTY) {
      atomicOr(status, DCNR_REQ_BAD_DATA);
      continue;
    }
    uint64_t s = mix64((uint64_t)id) & mask;
    bool placed = false;
    for (int64_t p = 0; p < cap; ++p) {   // bounded: no lane waits for another
      const unsigned long long old = atomicCAS((unsigned long long*)&t[s].key, (unsigned long long)ID_EMPTY,
                                               (unsigned long long)id);
      if ((int64_t)old == ID_EMPTY) {
        t[s].index = i;
        placed = true;
        break;
      }
      if ((int64_t)old == id) {           // a duplicate id
        atomicOr(status, DCNR_REQ_BAD_DATA);
        placed = true;
        break;
      }
      s = (s + 1ull) & mask;
    }
    if (!placed) atomicOr(status, DCNR_REQ_OVERFLOW);
  }
}

__global__ __launch_bounds__(RT_NT) void im_lookup_kernel(const Slot* t, int64_t cap, const int64_t* raw, int64_t M,
                                                          int64_t dflt, int64_t* out) {
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < M; i += step) {
    const int64_t r = map_find(t, cap, raw[i]);
    out[i] = r < 0 ? dflt : r;
  }
}

// ------------------------------------------------------------ id map insert
// The index word of a slot claimed by this call holds, between the claim and
// the head pass, SIGN | (the least batch row that carries the slot's id): below
// the -1 of an empty slot as an unsigned number, negative as a signed one.
__device__ __forceinline__ bool ins_bad(const int32_t* counts) { return (counts[1] & DCNR_REQ_BAD_DATA) != 0; }

// out[q] = the index of a known id, -1 otherwise; the reserved id sets the status
__global__ __launch_bounds__(RT_NT) void im_ins_find_kernel(const Slot* t, int64_t cap, const int64_t* raw, int64_t M,
                                                            int64_t* out, int32_t* counts) {
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  bool reserved = false;
  for (int64_t i = i0; i < M; i += step) {
    const int64_t id = raw[i];
    reserved |= id == ID_EMPTY;
    out[i] = map_find(t, cap, id);
  }
  if (reserved) atomicOr(counts + 1, DCNR_REQ_BAD_DATA);
}

// every unknown row claims (or finds claimed) its id's slot and offers its row number
__global__ __launch_bounds__(RT_NT) void im_ins_claim_kernel(Slot* t, int64_t cap, const int64_t* raw, int64_t M,
                                                             const int64_t* out, int64_t* slot, int32_t* counts) {
  if (ins_bad(counts)) return;   // decided by the kernel before: the table stays as it was
  const uint64_t mask = (uint64_t)cap - 1ull;
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < M; i += step) {
    if (out[i] >= 0) continue;
    const int64_t id = raw[i];
    uint64_t s = mix64((uint64_t)id) & mask;
    int64_t at = -1;
    for (int64_t p = 0; p < cap; ++p) {   // bounded: no lane waits for another
      const unsigned long long old = atomicCAS((unsigned long long*)&t[s].key, (unsigned long long)ID_EMPTY,
                                               (unsigned long long)id);
      if ((int64_t)old == ID_EMPTY || (int64_t)old == id) {
        at = (int64_t)s;
        break;
      }
      s = (s + 1ull) & mask;
    }
    slot[i] = at;
    if (at >= 0)
      atomicMin((unsigned long long*)&t[at].index, (unsigned long long)(SIGN | (uint64_t)i));
    else
      atomicOr(counts + 1, DCNR_REQ_OVERFLOW);
  }
}

// mark[q] = 1 for the first row of every new id
__global__ __launch_bounds__(RT_NT) void im_ins_mark_kernel(const Slot* t, const int64_t* out, const int64_t* slot,
                                                            int64_t M, uint32_t* mark, const int32_t* counts) {
  const bool bad = ins_bad(counts);
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < M; i += step) {
    uint32_t m = 0u;
    if (!bad && out[i] < 0 && slot[i] >= 0) m = t[slot[i]].index == (int64_t)(SIGN | (uint64_t)i) ? 1u : 0u;
    mark[i] = m;
  }
}

// scan: the inclusive scan of mark.  The heads number their ids n, n + 1, ...
__global__ __launch_bounds__(RT_NT) void im_ins_head_kernel(Slot* t, const int64_t* raw, int64_t M, int64_t n,
                                                            const int64_t* slot, const uint32_t* scan, int64_t* out,
                                                            int64_t* new_ids, int32_t* counts) {
  if (ins_bad(counts)) return;
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < M; i += step) {
    const uint32_t inc = scan[i], before = i ? scan[i - 1] : 0u;
    if (inc != before) {
      const int64_t j = (int64_t)before;
      t[slot[i]].index = n + j;
      new_ids[j] = raw[i];
      out[i] = n + j;
    }
    if (i == M - 1) counts[0] = (int32_t)inc;
  }
}

// the other rows of a new id read what its head wrote
__global__ __launch_bounds__(RT_NT) void im_ins_rest_kernel(const Slot* t, const int64_t* slot, int64_t M,
                                                            int64_t* out, const int32_t* counts) {
  if (ins_bad(counts)) return;
  const int64_t i0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  for (int64_t i = i0; i < M; i += step)
    if (out[i] < 0 && slot[i] >= 0) out[i] = t[slot[i]].index;
}

// --------------------------------------------------------------- the rows
struct RowsIn {
  const int64_t* user; const int64_t* item; const int64_t* cat_key; const double* raw;
  int64_t M; int n_cat, n_raw;
  int fcol; double lo, hi;
  int drop;
  const Slot* ut; int64_t ucap, n_users;
  const Slot* it; int64_t icap, n_items;
  const int64_t* cat_keys;
};

// Row i's codes under the fallback policy and its unknown bits (bit 0 the user,
// bit 1 the hotel, bit 2 + c category c).  WRITE: the codes go to output row j.
template <bool WRITE>
__device__ __forceinline__ uint64_t encode_row(const RowsIn& in, const CatOff& co, int64_t i, int64_t j,
                                               int64_t* collab, int64_t* cat) {
  uint64_t bits = 0ull;
  int64_t u = map_find(in.ut, in.ucap, in.user[i]);
  if (u < 0 || u >= in.n_users) {
    bits |= 1ull;
    u = in.n_users / 2;
  }
  int64_t h = map_find(in.it, in.icap, in.item[i]);
  if (h < 0 || h >= in.n_items) {
    bits |= 2ull;
    h = 0;
  }
  if (WRITE) {
    collab[j * 2] = u;
    collab[j * 2 + 1] = h;
  }
  for (int c = 0; c < in.n_cat; ++c) {
    const int64_t key = in.cat_key[i * in.n_cat + c];
    const int64_t b0 = co.off[c], b1 = co.off[c + 1];
    int64_t lo = b0, hi = b1;   // the first position whose key is not below
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (in.cat_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    int64_t code = lo - b0;
    if (key < 0 || lo >= b1 || in.cat_keys[lo] != key) {
      bits |= 1ull << (2 + c);
      code = 0;
    }
    if (WRITE) cat[j * in.n_cat + c] = code;
  }
  return bits;
}

// counts: {n, rows the filter removed, unknown users, unknown hotels, status},
// then the unknown count per category column (all over the rows that passed)
__global__ __launch_bounds__(RT_NT) void rt_flags_kernel(RowsIn in, CatOff co, uint32_t* keep, int32_t* counts) {
  __shared__ int cnt[3 + RT_MAXCAT];
  const int n_cnt = 3 + in.n_cat, lane = threadIdx.x & 63;
  for (int k = threadIdx.x; k < n_cnt; k += RT_NT) cnt[k] = 0;
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * RT_NT;
  for (int64_t base = (int64_t)blockIdx.x * RT_NT + (threadIdx.x & ~63); base < in.M; base += step) {
    const int64_t i = base + lane;   // (the trip count is the wave's: ballots below)
    const bool valid = i < in.M;
    bool pass = valid;
    uint64_t bits = 0ull;
    if (valid) {
      if (in.fcol >= 0) {
        const double v = in.raw[i * in.n_raw + in.fcol];
        pass = v >= in.hi || v <= in.lo;   // (NaN fails both)
      }
      if (pass) bits = encode_row<false>(in, co, i, 0, nullptr, nullptr);
      keep[i] = (pass && !(in.drop && bits)) ? 1u : 0u;
    }
    const uint64_t out = __ballot(valid && !pass);
    if (out && lane == 0) atomicAdd(&cnt[0], (int)__popcll(out));
    if (__ballot(bits != 0ull)) {
      for (int k = 0; k < 2 + in.n_cat; ++k) {
        const uint64_t b = __ballot((bits >> k) & 1ull);
        if (b && lane == 0) atomicAdd(&cnt[1 + k], (int)__popcll(b));
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < n_cnt; k += RT_NT)
    if (cnt[k]) atomicAdd(counts + (k < 3 ? 1 + k : DCNR_ROWS_TRANSFORM_COUNTS + (k - 3)), cnt[k]);
}

__global__ __launch_bounds__(RT_NT) void rt_emit_kernel(RowsIn in, CatOff co, Derived dv, const uint32_t* pos,
                                                        const uint8_t* target, const double* fit, int fill_nan,
                                                        int32_t* row, int64_t* collab, int64_t* cat, float* num,
                                                        float* y, int64_t* unknown_bits, int32_t* counts) {
  __shared__ double st[3][MAXC];   // median, scale_, min_
  const int n_num = in.n_raw + dv.n;
  if ((int)threadIdx.x < n_num) {
    st[0][threadIdx.x] = fit[threadIdx.x];
    st[1][threadIdx.x] = fit[n_num + threadIdx.x];
    st[2][threadIdx.x] = fit[2 * n_num + threadIdx.x];
  }
  __syncthreads();
  const int64_t M = in.M;
  const int64_t t0 = (int64_t)blockIdx.x * RT_NT + threadIdx.x, step = (int64_t)gridDim.x * RT_NT;
  bool inf = false;
  for (int64_t i = t0; i < M; i += step) {
    const uint32_t p = pos[i];
    if (i == M - 1) counts[0] = (int32_t)p;
    if (p == (i ? pos[i - 1] : 0u)) continue;   // not kept
    const int64_t j = (int64_t)p - 1;
    if (j < 0 || j > i) continue;               // (cannot happen; keeps every store in bounds)
    const uint64_t bits = encode_row<true>(in, co, i, j, collab, cat);
    row[j] = (int32_t)i;
    unknown_bits[j] = (int64_t)bits;
    if (y) y[j] = target[i] ? 1.0f : 0.0f;
    const double* r = in.raw + i * in.n_raw;
    for (int c = 0; c < n_num; ++c) {
      double x = c < in.n_raw ? r[c] : derived_value(dv, c - in.n_raw, r);
      if (fill_nan && is_nan(x)) x = st[0][c];
      inf |= is_inf(x);
      num[j * n_num + c] = scaled(x, st[1][c], st[2][c]);
    }
  }
  if (inf) atomicOr(counts + 4, DCNR_REQ_BAD_DATA);
}

int grid_for(int64_t n) { return (int)std::min<int64_t>(RT_MAXB, std::max<int64_t>(1, cdiv(n, RT_NT))); }

struct Ws {
  uint32_t* keep;      // [M]: the flags, then their inclusive scan
  uint32_t* tile_tot;  // [scan_tiles(M)]
  size_t total;
};

Ws carve(int64_t M, void* base) {
  Bump b(base);
  Ws w;
  w.keep = (uint32_t*)b.take((size_t)M * 4);
  w.tile_tot = (uint32_t*)b.take((size_t)scan_tiles(M) * 4);
  w.total = b.off;
  return w;
}

dcnr_status rows_transform(const dcnr_rows_transform_args& a, void* ws, hipStream_t s) {
  const int64_t M = a.M;
  const int n_counts = DCNR_ROWS_TRANSFORM_COUNTS + a.n_cat;
  const Ws w = carve(M, ws);
  RowsIn in;
  in.user = a.user; in.item = a.item; in.cat_key = a.cat_key; in.raw = a.raw;
  in.M = M; in.n_cat = a.n_cat; in.n_raw = a.n_raw;
  in.fcol = a.filter_col; in.lo = a.filter_lo; in.hi = a.filter_hi;
  in.drop = a.drop_unknown ? 1 : 0;
  in.ut = (const Slot*)a.user_table; in.ucap = a.user_capacity; in.n_users = a.n_users;
  in.it = (const Slot*)a.item_table; in.icap = a.item_capacity; in.n_items = a.n_items;
  in.cat_keys = a.cat_keys;
  CatOff co = {};
  for (int c = 0; c <= a.n_cat; ++c) co.off[c] = a.n_cat ? a.cat_offsets[c] : 0;
  const Derived dv = derived_pack(a.derived, a.n_derived);
  DCNR_HIP(hipMemsetAsync(a.counts, 0, (size_t)n_counts * 4, s));
  hipLaunchKernelGGL(rt_flags_kernel, dim3(grid_for(M)), dim3(RT_NT), 0, s, in, co, w.keep, a.counts);
  DCNR_LAUNCH_CHECK();
  TRY(scan_inplace<false>(w.keep, nullptr, M, w.tile_tot, s));
  hipLaunchKernelGGL(rt_emit_kernel, dim3(grid_for(M)), dim3(RT_NT), 0, s, in, co, dv, (const uint32_t*)w.keep,
                     a.target, a.fit, a.fill_nan ? 1 : 0, a.row, a.collab, a.cat, a.num, a.y, a.unknown_bits,
                     a.counts);
  DCNR_LAUNCH_CHECK();
  if (a.host_counts) TRY(mirror_words(a.counts, n_counts, a.host_counts, s));
  return DCNR_OK;
}

bool pow2(int64_t c) { return c > 0 && (c & (c - 1)) == 0; }

dcnr_status rows_shape(int64_t M, int32_t n_cat, int32_t n_raw, int32_t n_derived) {
  if (M < 0 || n_cat < 0 || n_raw < 0 || n_derived < 0) return DCNR_BAD_ARG;
  if (M >= 2147483647ll || n_cat > RT_MAXCAT || (int64_t)n_raw + n_derived > MAXC)
    return DCNR_UNSUPPORTED_SHAPE;
  return DCNR_OK;
}

struct InsWs {
  int64_t* slot;       // [M]: the slot of every row with an unknown id
  uint32_t* mark;      // [M]: the first-appearance marks, then their inclusive scan
  uint32_t* tile_tot;  // [scan_tiles(M)]
  size_t total;
};

InsWs ins_carve(int64_t M, void* base) {
  Bump b(base);
  InsWs w;
  w.slot = (int64_t*)b.take((size_t)M * 8);
  w.mark = (uint32_t*)b.take((size_t)M * 4);
  w.tile_tot = (uint32_t*)b.take((size_t)scan_tiles(M) * 4);
  w.total = b.off;
  return w;
}

dcnr_status id_map_insert(Slot* t, int64_t cap, int64_t n, const int64_t* raw, int64_t M, int64_t* out,
                          int64_t* new_ids, int32_t* counts, int32_t* host_counts, void* ws, hipStream_t s) {
  const InsWs w = ins_carve(M, ws);
  const dim3 g(grid_for(M)), b(RT_NT);
  DCNR_HIP(hipMemsetAsync(counts, 0, 8, s));
  hipLaunchKernelGGL(im_ins_find_kernel, g, b, 0, s, (const Slot*)t, cap, raw, M, out, counts);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(im_ins_claim_kernel, g, b, 0, s, t, cap, raw, M, (const int64_t*)out, w.slot, counts);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(im_ins_mark_kernel, g, b, 0, s, (const Slot*)t, (const int64_t*)out, (const int64_t*)w.slot, M,
                     w.mark, (const int32_t*)counts);
  DCNR_LAUNCH_CHECK();
  TRY(scan_inplace<false>(w.mark, nullptr, M, w.tile_tot, s));
  hipLaunchKernelGGL(im_ins_head_kernel, g, b, 0, s, t, raw, M, n, (const int64_t*)w.slot, (const uint32_t*)w.mark,
                     out, new_ids, counts);
  DCNR_LAUNCH_CHECK();
  hipLaunchKernelGGL(im_ins_rest_kernel, g, b, 0, s, (const Slot*)t, (const int64_t*)w.slot, M, out,
                     (const int32_t*)counts);
  DCNR_LAUNCH_CHECK();
  if (host_counts) TRY(mirror_words(counts, 2, host_counts, s));
  return DCNR_OK;
}

}  // namespace

}  // namespace dcnr

using namespace dcnr;

extern "C" {

dcnr_status dcnr_id_map_build(const int64_t* ids, int64_t n, void* table, int64_t capacity, int32_t* status,
                              int32_t* host_status, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n < 0 || !table || ((uintptr_t)table & 15) || !status || !pow2(capacity) || capacity <= n || (n > 0 && !ids)) {
    set_error("dcnr_id_map_build: bad argument (n=%lld, capacity=%lld: a power of two above n)", (long long)n,
              (long long)capacity);
    return DCNR_BAD_ARG;
  }
  if (capacity > (1ll << 40)) {
    set_error("dcnr_id_map_build: unsupported capacity %lld", (long long)capacity);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  ProfScope ps(DCNR_K_SERVE, s);
  hipLaunchKernelGGL(im_clear_kernel, dim3(grid_for(capacity)), dim3(RT_NT), 0, s, (Slot*)table, capacity, status);
  DCNR_LAUNCH_CHECK();
  if (n > 0) {
    hipLaunchKernelGGL(im_insert_kernel, dim3(grid_for(n)), dim3(RT_NT), 0, s, ids, n, (Slot*)table, capacity,
                       status);
    DCNR_LAUNCH_CHECK();
  }
  if (host_status) TRY(mirror_word(status, host_status, s));
  return DCNR_OK;
}

dcnr_status dcnr_id_map_lookup(const void* table, int64_t capacity, const int64_t* raw, int64_t M,
                               int64_t default_index, int64_t* out, dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (M < 0 || !table || ((uintptr_t)table & 15) || !pow2(capacity) || (M > 0 && (!raw || !out))) {
    set_error("dcnr_id_map_lookup: bad argument (M=%lld, capacity=%lld)", (long long)M, (long long)capacity);
    return DCNR_BAD_ARG;
  }
  if (M == 0) return DCNR_OK;
  ProfScope ps(DCNR_K_SERVE, s);
  hipLaunchKernelGGL(im_lookup_kernel, dim3(grid_for(M)), dim3(RT_NT), 0, s, (const Slot*)table, capacity, raw, M,
                     default_index, out);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

size_t dcnr_id_map_insert_workspace_size(int64_t M) {
  if (M < 0 || M >= 2147483647ll) return 0;
  return ins_carve(M, nullptr).total + 256;
}

dcnr_status dcnr_id_map_insert(void* table, int64_t capacity, int64_t n, const int64_t* raw, int64_t M, int64_t* out,
                               int64_t* new_ids, int32_t* counts, int32_t* host_counts, void* ws, size_t ws_bytes,
                               dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (M < 0 || n < 0 || !table || ((uintptr_t)table & 15) || !counts || !pow2(capacity) || capacity <= n ||
      (M > 0 && (!raw || !out || !new_ids || !ws))) {
    set_error("dcnr_id_map_insert: bad argument (M=%lld, n=%lld, capacity=%lld: a power of two above n)",
              (long long)M, (long long)n, (long long)capacity);
    return DCNR_BAD_ARG;
  }
  if (M >= 2147483647ll || capacity > (1ll << 40)) {
    set_error("dcnr_id_map_insert: unsupported shape (M=%lld, capacity=%lld)", (long long)M, (long long)capacity);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (M == 0) return zero_counts(counts, host_counts, 2, s);
  const size_t need = ins_carve(M, nullptr).total + 256;
  if (ws_bytes < need) {
    set_error("dcnr_id_map_insert: workspace too small: %zu < %zu", ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TRYP(DCNR_K_SERVE, s,
       id_map_insert((Slot*)table, capacity, n, raw, M, out, new_ids, counts, host_counts, ws_align(ws), s));
  return DCNR_OK;
}

size_t dcnr_rows_transform_workspace_size(int64_t M,int32_t n_cat, int32_t n_raw, int32_t n_derived) {
  if (rows_shape(M, n_cat, n_raw, n_derived) != DCNR_OK) return 0;
  return carve(M, nullptr).total + 256;
}

dcnr_status dcnr_rows_transform(const dcnr_rows_transform_args* a, void* ws, size_t ws_bytes,
                                dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!a) {
    set_error("dcnr_rows_transform: null args");
    return DCNR_BAD_ARG;
  }
  const dcnr_status shape = rows_shape(a->M, a->n_cat, a->n_raw, a->n_derived);
  bool bad = shape == DCNR_BAD_ARG || !a->counts || a->filter_col < -1 ||
             (a->filter_col >= 0 && a->filter_col >= a->n_raw) || !derived_ok(a->derived, a->n_derived, a->n_raw) ||
             a->n_users < 0 || a->n_items < 0 || !pow2(a->user_capacity) || !pow2(a->item_capacity) ||
             a->user_capacity <= a->n_users || a->item_capacity <= a->n_items;
  if (!bad && shape == DCNR_OK && a->n_cat > 0) {
    bad = !a->cat_offsets;
    if (!bad) {
      bad = a->cat_offsets[0] != 0;
      for (int c = 0; c < a->n_cat; ++c) bad |= a->cat_offsets[c + 1] < a->cat_offsets[c];
      bad |= a->cat_offsets[a->n_cat] > 0 && !a->cat_keys;
    }
  }
  if (!bad && a->M > 0) {
    const bool num = a->n_raw + a->n_derived > 0;
    bad = !a->user || !a->item || !ws || !a->user_table || !a->item_table ||
          (((uintptr_t)a->user_table | (uintptr_t)a->item_table) & 15) ||
          (a->n_cat > 0 && (!a->cat_key || !a->cat)) || (a->n_raw > 0 && !a->raw) || (num && (!a->num || !a->fit)) ||
          !a->row || !a->collab || !a->unknown_bits || (a->target != nullptr) != (a->y != nullptr);
  }
  if (bad) {
    set_error("dcnr_rows_transform: bad argument (M=%lld, n_cat=%d, n_raw=%d, n_derived=%d, filter_col=%d)",
              (long long)a->M, a->n_cat, a->n_raw, a->n_derived, a->filter_col);
    return DCNR_BAD_ARG;
  }
  if (shape != DCNR_OK) {
    set_error("dcnr_rows_transform: unsupported shape (M=%lld, n_cat=%d, n_raw=%d, n_derived=%d)", (long long)a->M,
              a->n_cat, a->n_raw, a->n_derived);
    return shape;
  }
  if (a->M == 0) return zero_counts(a->counts, a->host_counts, DCNR_ROWS_TRANSFORM_COUNTS + a->n_cat, s);
  const size_t need = carve(a->M, nullptr).total + 256;
  if (ws_bytes < need) {
    set_error("dcnr_rows_transform: workspace too small: %zu < %zu", ws_bytes, need);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TRYP(DCNR_K_SERVE, s, rows_transform(*a, ws_align(ws), s));
  return DCNR_OK;
}

}  // extern "C"
