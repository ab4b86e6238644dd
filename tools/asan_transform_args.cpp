// The host side of dcnr_id_map_build, dcnr_id_map_lookup and dcnr_rows_transform
// under AddressSanitizer: argument and shape rejection, the derived list and the
// category offsets (both read on the host, here from heap blocks of exactly
// their size) and the workspace check.  Every call below returns before any
// launch, so the program needs no GPU.  Built and run by
//
//     make -C <package>/csrc asan-transform
//
// against lib/libdcnr_asan.so (host code with -fsanitize=address, device code
// as usual).  Exit status 0 and no sanitizer report: clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/dcnr.h"

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                \
    }                                                            \
  } while (0)

// never dereferenced: every call is rejected before a launch
template <typename T> static T* fake(uintptr_t n) { return reinterpret_cast<T*>(uintptr_t(0x10000) * n); }

static dcnr_rows_transform_args good(const int32_t* derived, int n_derived, const int64_t* offsets, int n_cat) {
  dcnr_rows_transform_args a = {};
  a.user = fake<const int64_t>(1); a.item = fake<const int64_t>(2); a.target = fake<const uint8_t>(3);
  a.cat_key = fake<const int64_t>(4); a.raw = fake<const double>(5);
  a.M = 100; a.n_cat = n_cat; a.n_raw = 8;
  a.filter_col = 3; a.filter_lo = 4.0; a.filter_hi = 8.0;
  a.n_derived = n_derived; a.derived = derived;
  a.fill_nan = 1; a.drop_unknown = 0;
  a.user_table = fake<const void>(6); a.user_capacity = 64; a.n_users = 30;
  a.item_table = fake<const void>(7); a.item_capacity = 16; a.n_items = 15;
  a.cat_keys = fake<const int64_t>(8); a.cat_offsets = offsets; a.fit = fake<const double>(9);
  a.row = fake<int32_t>(10); a.collab = fake<int64_t>(11); a.cat = fake<int64_t>(12); a.num = fake<float>(13);
  a.y = fake<float>(14); a.unknown_bits = fake<int64_t>(15); a.counts = fake<int32_t>(16);
  return a;
}

int main() {
  // ---- the id map
  void* table = fake<void>(20);
  int32_t* status = fake<int32_t>(21);
  const int64_t* ids = fake<const int64_t>(22);
  int64_t* out = fake<int64_t>(23);
  EXPECT(dcnr_id_map_build(ids, 10, nullptr, 16, status, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(ids, 10, table, 16, nullptr, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(nullptr, 10, table, 16, status, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(ids, -1, table, 16, status, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(ids, 10, table, 24, status, nullptr, nullptr) == DCNR_BAD_ARG);   // no power of two
  EXPECT(dcnr_id_map_build(ids, 16, table, 16, status, nullptr, nullptr) == DCNR_BAD_ARG);   // no empty slot
  EXPECT(dcnr_id_map_build(ids, 10, table, 0, status, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(ids, 10, (char*)table + 8, 16, status, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_build(ids, 10, table, 1ll << 41, status, nullptr, nullptr) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(dcnr_id_map_lookup(nullptr, 16, ids, 5, -1, out, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup(table, 24, ids, 5, -1, out, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup(table, 16, nullptr, 5, -1, out, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup(table, 16, ids, 5, -1, nullptr, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup(table, 16, ids, -1, -1, out, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup((char*)table + 4, 16, ids, 5, -1, out, nullptr) == DCNR_BAD_ARG);
  EXPECT(dcnr_id_map_lookup(table, 16, nullptr, 0, -1, nullptr, nullptr) == DCNR_OK);        // nothing to do

  // ---- the rows' transform
  EXPECT(dcnr_rows_transform_workspace_size(100, 2, 8, 3) > 0);
  EXPECT(dcnr_rows_transform_workspace_size(0, 0, 0, 0) > 0);
  EXPECT(dcnr_rows_transform_workspace_size(2147483646ll, 62, 61, 3) > 0);
  EXPECT(dcnr_rows_transform_workspace_size(-1, 2, 8, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, -1, 8, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, 2, -1, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, 2, 8, -1) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(2147483647ll, 2, 8, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, 63, 8, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, 2, 62, 3) == 0);
  EXPECT(dcnr_rows_transform_workspace_size(100, 2, 2147483647, 2147483647) == 0);

  void* ws = fake<void>(17);
  const size_t big = size_t(1) << 40;
  EXPECT(dcnr_rows_transform(nullptr, ws, big, nullptr) == DCNR_BAD_ARG);
  for (int n = 0; n <= 64; n += 8) {   // the derived list, exactly n entries long
    std::vector<int32_t>* d = new std::vector<int32_t>(3 * n);
    for (int k = 0; k < n; ++k) { (*d)[3 * k] = k & 1; (*d)[3 * k + 1] = k % 8; (*d)[3 * k + 2] = (k + 1) % 8; }
    std::vector<int64_t>* off = new std::vector<int64_t>{0, 5, 12};
    dcnr_rows_transform_args a = good(n ? d->data() : nullptr, n, off->data(), 2);
    // a valid list: rejected only by the workspace (or the shape: 8 raw + n derived > 64)
    const dcnr_status want = 8 + n > 64 ? DCNR_UNSUPPORTED_SHAPE : DCNR_WORKSPACE_TOO_SMALL;
    EXPECT(dcnr_rows_transform(&a, ws, 0, nullptr) == want);
    if (n) {
      (*d)[3 * (n - 1) + 2] = 8;    // the last entry names a column that is not there
      EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == DCNR_BAD_ARG);
      (*d)[3 * (n - 1) + 2] = 0;
      (*d)[3 * (n - 1)] = 2;        // ... or an op that is neither
      EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == DCNR_BAD_ARG);
    }
    delete off;
    delete d;
  }
  static const int32_t one[3] = {DCNR_DERIVED_RATIO, 0, 1};
  for (int n_cat = 0; n_cat <= 62; n_cat += 31) {   // the offsets, exactly n_cat + 1 entries long
    std::vector<int64_t>* off = new std::vector<int64_t>(n_cat + 1);
    for (int c = 0; c <= n_cat; ++c) (*off)[c] = 3 * c;
    dcnr_rows_transform_args a = good(one, 1, n_cat ? off->data() : nullptr, n_cat);
    EXPECT(dcnr_rows_transform(&a, ws, 0, nullptr) == DCNR_WORKSPACE_TOO_SMALL);
    if (n_cat) {
      (*off)[n_cat] = (*off)[n_cat - 1] - 1;   // the last list ends before it starts
      EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == DCNR_BAD_ARG);
      (*off)[n_cat] = 3 * n_cat;
      (*off)[0] = 1;                           // the first does not start at 0
      EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == DCNR_BAD_ARG);
    }
    delete off;
  }
  static const int64_t offsets[3] = {0, 5, 12};
  {
    dcnr_rows_transform_args a = good(one, 1, offsets, 2);
    const size_t need = dcnr_rows_transform_workspace_size(a.M, a.n_cat, a.n_raw, a.n_derived);
    EXPECT(dcnr_rows_transform(&a, ws, need - 1, nullptr) == DCNR_WORKSPACE_TOO_SMALL);
    EXPECT(dcnr_rows_transform(&a, nullptr, need, nullptr) == DCNR_BAD_ARG);
  }
#define REJECT(field, value, status)                                    \
  do {                                                                  \
    dcnr_rows_transform_args a = good(one, 1, offsets, 2);              \
    a.field = value;                                                    \
    EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == status);        \
  } while (0)
  REJECT(user, nullptr, DCNR_BAD_ARG); REJECT(item, nullptr, DCNR_BAD_ARG); REJECT(target, nullptr, DCNR_BAD_ARG);
  REJECT(y, nullptr, DCNR_BAD_ARG);    // (target and y come or go together)
  REJECT(cat_key, nullptr, DCNR_BAD_ARG); REJECT(raw, nullptr, DCNR_BAD_ARG); REJECT(derived, nullptr, DCNR_BAD_ARG);
  REJECT(user_table, nullptr, DCNR_BAD_ARG); REJECT(item_table, nullptr, DCNR_BAD_ARG);
  REJECT(user_table, fake<char>(6) + 8, DCNR_BAD_ARG);
  REJECT(user_capacity, 48, DCNR_BAD_ARG); REJECT(item_capacity, 8, DCNR_BAD_ARG); REJECT(n_users, 64, DCNR_BAD_ARG);
  REJECT(n_users, -1, DCNR_BAD_ARG); REJECT(n_items, -1, DCNR_BAD_ARG);
  REJECT(cat_keys, nullptr, DCNR_BAD_ARG); REJECT(cat_offsets, nullptr, DCNR_BAD_ARG); REJECT(fit, nullptr, DCNR_BAD_ARG);
  REJECT(row, nullptr, DCNR_BAD_ARG); REJECT(collab, nullptr, DCNR_BAD_ARG); REJECT(cat, nullptr, DCNR_BAD_ARG);
  REJECT(num, nullptr, DCNR_BAD_ARG); REJECT(unknown_bits, nullptr, DCNR_BAD_ARG); REJECT(counts, nullptr, DCNR_BAD_ARG);
  REJECT(M, -1, DCNR_BAD_ARG); REJECT(n_cat, -1, DCNR_BAD_ARG); REJECT(n_raw, -1, DCNR_BAD_ARG);
  REJECT(n_derived, -1, DCNR_BAD_ARG); REJECT(filter_col, 8, DCNR_BAD_ARG); REJECT(filter_col, -2, DCNR_BAD_ARG);
  REJECT(M, 2147483647ll, DCNR_UNSUPPORTED_SHAPE); REJECT(n_raw, 64, DCNR_UNSUPPORTED_SHAPE);
  {
    dcnr_rows_transform_args a = good(one, 1, offsets, 2);
    a.n_cat = 63;   // rejected by the shape before an offset is read
    EXPECT(dcnr_rows_transform(&a, ws, big, nullptr) == DCNR_UNSUPPORTED_SHAPE);
    a = good(one, 1, offsets, 2);
    a.target = nullptr; a.y = nullptr;   // no target at all is fine: only the workspace is missing
    EXPECT(dcnr_rows_transform(&a, ws, 0, nullptr) == DCNR_WORKSPACE_TOO_SMALL);
  }
  EXPECT(dcnr_last_error() != nullptr);
  std::printf("asan_transform_args: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
