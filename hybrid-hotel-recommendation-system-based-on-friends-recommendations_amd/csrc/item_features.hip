// Each hotel's ranking features from its first main_df row, on the device
// (dcnr_item_features_build): what main.py:315 takes with isin +
// drop_duplicates(subset=['item_id']) and preprocess_for_ranking
// (main.py:215-230) encodes and scales, for every hotel at once.
//
// Per main_df row, in ascending row order: hotel row, the row's main_df number,
// the caller's n_cat encoded codes (int32) and the n_num raw values (float64).
//
//   init     firstpos[h] = INT_MAX, the two count words zeroed
//   scan     one pass over review_item (and review_row), four rows per lane
//            where the columns are 16-byte aligned: firstpos[h] = the smallest
//            position that names h, by an integer atomicMin -- the same word
//            whatever the arrival order.  A plain load in front skips the
//            atomic where the slot already holds a smaller position (the slot
//            only ever falls, so a stale value can only cost an atomic, never
//            lose one).  A lane loads its four slots before it branches on
//            them, so the four reads are in flight together.  Items and the
//            row order are validated here; an item outside [0, n_items)
//            touches nothing.
//   gather   one hotel per group of G lanes, G the power of two that holds
//            max(n_cat, n_num): lane c of a group copies code c and scales
//            value c of the hotel's first row, so a wave's stores run along
//            64 / G consecutive table rows and its loads along whole review
//            rows.  The hotels with a row are counted per workgroup, one word
//            each: thousands of waves adding to one address queue up behind
//            each other (one atomic per wave made this kernel 99.6 us at
//            100 000 hotels; it is 8.6 us)
//   finish   one workgroup sums those words; the two count words to their
//            host mirrors
//
// The scale is MinMaxScaler.transform's as prepare_data applies it: scaled()
// of device_prims.h.
//
// Every word is an integer or written by one lane: the same bits on every run.
// Workspace: 4 * n_items bytes and one word per workgroup of the gather.
#include "device_prims.h"

namespace dcnr {

namespace {

constexpr int IF_NT = 256;
constexpr int IF_MAXB = 2048;                 // workgroups of the grid-stride kernels
constexpr int32_t IF_NONE = 0x7FFFFFFF;       // above every position (M < 2^31 - 1)

typedef __attribute__((ext_vector_type(4))) int i32x4;

__global__ __launch_bounds__(IF_NT) void if_init_kernel(int32_t* firstpos, int64_t n_items, int32_t* counts) {
  const int64_t i0 = (int64_t)blockIdx.x * IF_NT + threadIdx.x, step = (int64_t)gridDim.x * IF_NT;
  if (firstpos)
    for (int64_t i = i0; i < n_items; i += step) firstpos[i] = IF_NONE;
  if (i0 < 2) counts[i0] = 0;
}

__device__ __forceinline__ void claim(int32_t* firstpos, int64_t n_items, int h, int32_t pos, bool& bad) {
  if (h < 0 || (int64_t)h >= n_items) {
    bad = true;
    return;
  }
  if (firstpos[h] > pos) atomicMin(firstpos + h, pos);
}

// VEC: item (and row, if given) are 16-byte aligned; a lane takes rows 4 q .. 4 q + 3
template <bool VEC>
__global__ __launch_bounds__(IF_NT) void if_scan_kernel(const int32_t* item, const int32_t* row, int64_t M,
                                                        int64_t n_items, int32_t* firstpos, int32_t* counts) {
  bool bad = false;
  const int64_t t0 = (int64_t)blockIdx.x * IF_NT + threadIdx.x, step = (int64_t)gridDim.x * IF_NT;
  if (VEC) {
    const int64_t quads = M >> 2;
    for (int64_t q = t0; q < quads; q += step) {
      const i32x4 h = *reinterpret_cast<const i32x4*>(item + 4 * q);
      if (row) {
        const i32x4 r = *reinterpret_cast<const i32x4*>(row + 4 * q);
        const int32_t before = q ? row[4 * q - 1] : -1;
        bad |= r[0] <= before || r[1] <= r[0] || r[2] <= r[1] || r[3] <= r[2];
      }
      // the four slots first, so that their loads are in flight together
      // (an item out of range reads nothing and claims nothing)
      int32_t cur[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = h[j] >= 0 && (int64_t)h[j] < n_items;
        bad |= !ok;
        cur[j] = ok ? firstpos[h[j]] : -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cur[j] > (int32_t)(4 * q + j)) atomicMin(firstpos + h[j], (int32_t)(4 * q + j));
    }
    for (int64_t i = 4 * quads + t0; i < M; i += step) {   // the last M % 4 rows
      if (row) bad |= row[i] <= (i ? row[i - 1] : -1);
      claim(firstpos, n_items, item[i], (int32_t)i, bad);
    }
  } else {
    for (int64_t i = t0; i < M; i += step) {
      if (row) bad |= row[i] <= (i ? row[i - 1] : -1);
      claim(firstpos, n_items, item[i], (int32_t)i, bad);
    }
  }
  if (bad) atomicOr(counts + 1, DCNR_REQ_BAD_DATA);
}

__global__ __launch_bounds__(IF_NT) void if_gather_kernel(const int32_t* firstpos, const int32_t* row,
                                                          const int32_t* cat, const double* num,
                                                          const double* scale, const double* mn, int64_t M,
                                                          int64_t n_items, int n_cat, int n_num, int gshift,
                                                          int32_t* first_row, int64_t* item_cat,
                                                          float* item_num, int32_t* partial) {
  __shared__ int part[IF_NT / WAVE];
  const int c = threadIdx.x & ((1 << gshift) - 1);
  const int64_t per = IF_NT >> gshift;   // hotels per workgroup step
  const double sc = c < n_num ? scale[c] : 0.0, mc = c < n_num ? mn[c] : 0.0;
  int found = 0;
  for (int64_t h0 = (int64_t)blockIdx.x * per; h0 < n_items; h0 += (int64_t)gridDim.x * per) {
    const int64_t h = h0 + (threadIdx.x >> gshift);
    if (h >= n_items) continue;
    int64_t p = firstpos ? (int64_t)firstpos[h] : IF_NONE;
    if (p < 0 || p >= M) p = -1;   // (a position the scan wrote lies in [0, M))
    if (c == 0) {
      first_row[h] = p < 0 ? -1 : row ? row[p] : (int32_t)p;
      found += p >= 0 ? 1 : 0;
    }
    if (c < n_cat) item_cat[h * n_cat + c] = p < 0 ? (int64_t)0 : (int64_t)cat[p * n_cat + c];
    if (c < n_num) item_num[h * n_num + c] = p < 0 ? 0.0f : scaled(num[p * n_num + c], sc, mc);
  }
  // partial[blockIdx.x] = the hotels with a row this workgroup met
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) found += __shfl_xor(found, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = found;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < IF_NT / WAVE; ++w) s += part[w];
    if (partial) partial[blockIdx.x] = s;
  }
}

// counts[0] = the sum of the gather's n_parts words (one workgroup); both count
// words to the host mirror with system-scope stores (host memory, or null)
__global__ __launch_bounds__(IF_NT) void if_finish_kernel(const int32_t* partial, int n_parts, int32_t* counts,
                                                          int32_t* host_counts) {
  __shared__ int part[IF_NT / WAVE];
  int n = 0;
  for (int i = threadIdx.x; i < n_parts; i += IF_NT) n += partial[i];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < IF_NT / WAVE; ++w) s += part[w];
    const int32_t st = counts[1];
    counts[0] = s;
    if (host_counts) {
      __hip_atomic_store(host_counts, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(host_counts + 1, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

int blocks_for(int64_t n, int64_t per_block) {
  return (int)std::min<int64_t>(IF_MAXB, std::max<int64_t>(1, cdiv(n, per_block)));
}

}  // namespace

// firstpos [n_items], then partial [IF_MAXB]
static size_t item_features_ws_bytes(int64_t n_items) { return (size_t)rup(n_items * 4, 256) + IF_MAXB * 4; }

static dcnr_status item_features_build(const int32_t* item, const int32_t* row, const int32_t* cat,
                                       const double* num, const double* scale, const double* mn, int64_t M,
                                       int64_t n_items, int n_cat, int n_num, int32_t* first_row,
                                       int64_t* item_cat, float* item_num, int32_t* counts,
                                       int32_t* host_counts, void* ws, hipStream_t s) {
  // (without rows there may be no workspace: no hotel has a row, nothing is counted)
  int32_t* firstpos = M > 0 ? (int32_t*)ws : nullptr;
  int32_t* partial = M > 0 ? (int32_t*)((char*)ws + rup(n_items * 4, 256)) : nullptr;
  int n_parts = 0;
  hipLaunchKernelGGL(if_init_kernel, dim3(blocks_for(firstpos ? n_items : 1, IF_NT)), dim3(IF_NT), 0, s,
                     firstpos, n_items, counts);
  DCNR_LAUNCH_CHECK();
  if (M > 0) {
    const bool vec = (((uintptr_t)item | (uintptr_t)row) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(if_scan_kernel<true>, dim3(blocks_for(M, 4 * IF_NT)), dim3(IF_NT), 0, s, item, row,
                         M, n_items, firstpos, counts);
    else
      hipLaunchKernelGGL(if_scan_kernel<false>, dim3(blocks_for(M, IF_NT)), dim3(IF_NT), 0, s, item, row, M,
                         n_items, firstpos, counts);
    DCNR_LAUNCH_CHECK();
  }
  if (n_items > 0) {
    int gshift = 0;
    while ((1 << gshift) < std::max(n_cat, n_num)) ++gshift;   // (at most 6: 64 columns)
    const int blocks = blocks_for(n_items, IF_NT >> gshift);
    hipLaunchKernelGGL(if_gather_kernel, dim3(blocks), dim3(IF_NT), 0, s, (const int32_t*)firstpos, row, cat,
                       num, scale, mn, M, n_items, n_cat, n_num, gshift, first_row, item_cat, item_num,
                       partial);
    DCNR_LAUNCH_CHECK();
    if (partial) n_parts = blocks;
  }
  hipLaunchKernelGGL(if_finish_kernel, dim3(1), dim3(IF_NT), 0, s, (const int32_t*)partial, n_parts, counts,
                     host_counts);
  DCNR_LAUNCH_CHECK();
  return DCNR_OK;
}

}  // namespace dcnr

using namespace dcnr;

extern "C" {

static dcnr_status item_features_shape(int64_t M, int64_t n_items, int32_t n_cat, int32_t n_num) {
  if (M < 0 || n_items < 0 || n_cat < 0 || n_num < 0) return DCNR_BAD_ARG;
  if (n_cat > 64 || n_num > 64 || n_items > ((int64_t)1 << 29) || M >= 2147483647ll)
    return DCNR_UNSUPPORTED_SHAPE;
  return DCNR_OK;
}

size_t dcnr_item_features_workspace_size(int64_t M, int64_t n_items, int32_t n_cat, int32_t n_num) {
  if (item_features_shape(M, n_items, n_cat, n_num) != DCNR_OK) return 0;
  return item_features_ws_bytes(n_items) + 256;
}

dcnr_status dcnr_item_features_build(const int32_t* review_item, const int32_t* review_row,
                                     const int32_t* review_cat, const double* review_num,
                                     const double* scaler_scale, const double* scaler_min, int64_t M,
                                     int64_t n_items, int32_t n_cat, int32_t n_num, int32_t* first_row,
                                     int64_t* item_cat, float* item_num, int32_t* counts,
                                     int32_t* host_counts, void* ws, size_t ws_bytes,
                                     dcnr_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  const dcnr_status shape = item_features_shape(M, n_items, n_cat, n_num);
  if (shape == DCNR_BAD_ARG || !counts ||
      (n_items > 0 && (!first_row || (n_cat > 0 && !item_cat) || (n_num > 0 && !item_num))) ||
      (n_num > 0 && n_items > 0 && (!scaler_scale || !scaler_min)) ||
      (M > 0 && (!review_item || !ws || (n_cat > 0 && !review_cat) || (n_num > 0 && !review_num)))) {
    set_error("dcnr_item_features_build: bad argument (M=%lld, n_items=%lld, n_cat=%d, n_num=%d)",
              (long long)M, (long long)n_items, n_cat, n_num);
    return DCNR_BAD_ARG;
  }
  if (shape != DCNR_OK) {
    set_error("dcnr_item_features_build: unsupported shape (M=%lld, n_items=%lld, n_cat=%d, n_num=%d)",
              (long long)M, (long long)n_items, n_cat, n_num);
    return shape;
  }
  void* base = ws_align(ws);
  const size_t need = M > 0 ? item_features_ws_bytes(n_items) : 0;
  if (M > 0 && ws_bytes < need + ((char*)base - (char*)ws)) {
    set_error("dcnr_item_features_build: workspace too small: %zu < %zu", ws_bytes, need + 256);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TRYP(DCNR_K_SERVE, s, item_features_build(review_item, review_row, review_cat, review_num,
                                            scaler_scale, scaler_min, M, n_items, n_cat, n_num,
                                            first_row, item_cat, item_num, counts, host_counts, base,
                                            s));
  return DCNR_OK;
}

}  // extern "C"
