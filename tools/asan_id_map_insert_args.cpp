// The host side of dcnr_id_map_insert under AddressSanitizer: the size query,
// argument and shape rejection and the workspace check.  Every call below
// returns before any launch, so the program needs no GPU.  Built and run by
//
//     make -C <package>/csrc asan-id-map-insert
//
// against lib/libdcnr_asan.so (host code with -fsanitize=address, device code
// as usual).  Exit status 0 and no sanitizer report: clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

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

int main() {
  EXPECT(dcnr_id_map_insert_workspace_size(0) > 0);
  EXPECT(dcnr_id_map_insert_workspace_size(1) > 0);
  EXPECT(dcnr_id_map_insert_workspace_size(1 << 20) >= size_t(12) << 20);
  EXPECT(dcnr_id_map_insert_workspace_size(2147483646ll) >= size_t(12) * 2147483646ull);
  EXPECT(dcnr_id_map_insert_workspace_size(-1) == 0);
  EXPECT(dcnr_id_map_insert_workspace_size(2147483647ll) == 0);
  EXPECT(dcnr_id_map_insert_workspace_size(INT64_MAX) == 0);

  void* table = fake<void>(1);
  const int64_t* raw = fake<const int64_t>(2);
  int64_t* out = fake<int64_t>(3);
  int64_t* new_ids = fake<int64_t>(4);
  int32_t* counts = fake<int32_t>(5);
  void* ws = fake<void>(6);
  const size_t big = size_t(1) << 40;
  const int64_t M = 100, cap = 64, n = 30;
#define INSERT(table, cap, n, raw, M, out, new_ids, counts, ws, bytes) \
  dcnr_id_map_insert(table, cap, n, raw, M, out, new_ids, counts, nullptr, ws, bytes, nullptr)
  // a needed null pointer
  EXPECT(INSERT(nullptr, cap, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, nullptr, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, raw, M, nullptr, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, raw, M, out, nullptr, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, raw, M, out, new_ids, nullptr, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, raw, M, out, new_ids, counts, nullptr, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, n, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0) == DCNR_BAD_ARG);   // M = 0 too
  EXPECT(INSERT(nullptr, cap, n, nullptr, 0, nullptr, nullptr, counts, nullptr, 0) == DCNR_BAD_ARG);
  // negative sizes
  EXPECT(INSERT(table, cap, n, raw, -1, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, cap, -1, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, -64, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  // the capacity: a power of two above n
  EXPECT(INSERT(table, 48, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, 0, 0, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, 32, 32, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT(table, 16, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  // a misaligned table
  EXPECT(INSERT((char*)table + 8, cap, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  EXPECT(INSERT((char*)table + 4, cap, n, raw, M, out, new_ids, counts, ws, big) == DCNR_BAD_ARG);
  // shapes the call does not take
  EXPECT(INSERT(table, cap, n, raw, 2147483647ll, out, new_ids, counts, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(INSERT(table, 1ll << 41, n, raw, M, out, new_ids, counts, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  // the workspace
  const size_t need = dcnr_id_map_insert_workspace_size(M);
  EXPECT(INSERT(table, cap, n, raw, M, out, new_ids, counts, ws, need - 1) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(INSERT(table, cap, n, raw, M, out, new_ids, counts, ws, 0) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(INSERT(table, cap, n, raw, 2147483646ll, out, new_ids, counts, ws, big >> 20) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(dcnr_last_error() != nullptr);
  std::printf("asan_id_map_insert_args: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
