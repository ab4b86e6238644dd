// The host side of dcnr_train_table_build under AddressSanitizer: argument and
// shape rejection, the derived list (read on the host, here from heap blocks of
// exactly its size) and the workspace check.  Every call below returns before
// any launch, so the program needs no GPU.  Built and run by
//
//     make -C <package>/csrc asan-train-table
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

static dcnr_train_table_args good(const int32_t* derived, int n_derived) {
  dcnr_train_table_args a = {};
  a.user = fake<const int64_t>(1); a.item = fake<const int64_t>(2); a.target = fake<const uint8_t>(3);
  a.cat_key = fake<const int64_t>(4); a.raw = fake<const double>(5);
  a.M = 100; a.n_cat = 2; a.n_raw = 8;
  a.filter_col = 3; a.filter_lo = 4.0; a.filter_hi = 8.0;
  a.n_derived = n_derived; a.derived = derived;
  a.row = fake<int32_t>(6); a.collab = fake<int64_t>(7); a.cat = fake<int64_t>(8); a.num = fake<float>(9);
  a.y = fake<float>(10); a.user_ids = fake<int64_t>(11); a.item_ids = fake<int64_t>(12);
  a.cat_keys = fake<int64_t>(13); a.stats = fake<double>(14); a.counts = fake<int32_t>(15);
  return a;
}

int main() {
  EXPECT(dcnr_train_table_workspace_size(100, 2, 8, 3) > 0);
  EXPECT(dcnr_train_table_workspace_size(0, 0, 0, 0) > 0);
  EXPECT(dcnr_train_table_workspace_size(2147483646ll, 64, 61, 3) > 0);
  EXPECT(dcnr_train_table_workspace_size(-1, 2, 8, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, -1, 8, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, 2, -1, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, 2, 8, -1) == 0);
  EXPECT(dcnr_train_table_workspace_size(2147483647ll, 2, 8, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, 65, 8, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, 2, 62, 3) == 0);
  EXPECT(dcnr_train_table_workspace_size(100, 2, 2147483647, 2147483647) == 0);

  void* ws = fake<void>(16);
  const size_t big = size_t(1) << 40;
  EXPECT(dcnr_train_table_build(nullptr, ws, big, nullptr) == DCNR_BAD_ARG);
  for (int n = 0; n <= 64; n += 8) {   // the derived list, exactly n entries long
    std::vector<int32_t>* d = new std::vector<int32_t>(3 * n);
    for (int k = 0; k < n; ++k) { (*d)[3 * k] = k & 1; (*d)[3 * k + 1] = k % 8; (*d)[3 * k + 2] = (k + 1) % 8; }
    dcnr_train_table_args a = good(n ? d->data() : nullptr, n);
    // a valid list: rejected only by the workspace (or the shape: 8 raw + n derived > 64)
    const dcnr_status want = 8 + n > 64 ? DCNR_UNSUPPORTED_SHAPE : DCNR_WORKSPACE_TOO_SMALL;
    EXPECT(dcnr_train_table_build(&a, ws, 0, nullptr) == want);
    if (n) {
      (*d)[3 * (n - 1) + 2] = 8;    // the last entry names a column that is not there
      EXPECT(dcnr_train_table_build(&a, ws, big, nullptr) == DCNR_BAD_ARG);
      (*d)[3 * (n - 1) + 2] = 0;
      (*d)[3 * (n - 1)] = 2;        // ... or an op that is neither
      EXPECT(dcnr_train_table_build(&a, ws, big, nullptr) == DCNR_BAD_ARG);
    }
    delete d;
  }
  static const int32_t one[3] = {DCNR_DERIVED_RATIO, 0, 1};
  {
    dcnr_train_table_args a = good(one, 1);
    const size_t need = dcnr_train_table_workspace_size(a.M, a.n_cat, a.n_raw, a.n_derived);
    EXPECT(dcnr_train_table_build(&a, ws, need - 1, nullptr) == DCNR_WORKSPACE_TOO_SMALL);
    EXPECT(dcnr_train_table_build(&a, nullptr, need, nullptr) == DCNR_BAD_ARG);
  }
#define REJECT(field, value, status)                                       \
  do {                                                                     \
    dcnr_train_table_args a = good(one, 1);                                \
    a.field = value;                                                       \
    EXPECT(dcnr_train_table_build(&a, ws, big, nullptr) == status);        \
  } while (0)
  REJECT(user, nullptr, DCNR_BAD_ARG); REJECT(item, nullptr, DCNR_BAD_ARG); REJECT(target, nullptr, DCNR_BAD_ARG);
  REJECT(cat_key, nullptr, DCNR_BAD_ARG); REJECT(raw, nullptr, DCNR_BAD_ARG); REJECT(derived, nullptr, DCNR_BAD_ARG);
  REJECT(row, nullptr, DCNR_BAD_ARG); REJECT(collab, nullptr, DCNR_BAD_ARG); REJECT(cat, nullptr, DCNR_BAD_ARG);
  REJECT(num, nullptr, DCNR_BAD_ARG); REJECT(y, nullptr, DCNR_BAD_ARG); REJECT(user_ids, nullptr, DCNR_BAD_ARG);
  REJECT(item_ids, nullptr, DCNR_BAD_ARG); REJECT(cat_keys, nullptr, DCNR_BAD_ARG);
  REJECT(stats, nullptr, DCNR_BAD_ARG); REJECT(counts, nullptr, DCNR_BAD_ARG);
  REJECT(M, -1, DCNR_BAD_ARG); REJECT(n_cat, -1, DCNR_BAD_ARG); REJECT(n_raw, -1, DCNR_BAD_ARG);
  REJECT(n_derived, -1, DCNR_BAD_ARG); REJECT(filter_col, 8, DCNR_BAD_ARG); REJECT(filter_col, -2, DCNR_BAD_ARG);
  REJECT(M, 2147483647ll, DCNR_UNSUPPORTED_SHAPE); REJECT(n_cat, 65, DCNR_UNSUPPORTED_SHAPE);
  REJECT(n_raw, 64, DCNR_UNSUPPORTED_SHAPE);
  EXPECT(dcnr_last_error() != nullptr);
  std::printf("asan_train_table_args: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
