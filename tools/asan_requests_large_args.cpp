// The host side of the large request lane under AddressSanitizer: the size
// queries, argument and shape rejection and the workspace checks of
// dcnr_requests_large_candidates, dcnr_requests_large_ranking_batch,
// dcnr_requests_large_rank_mmr and dcnr_mmr_rerank_large.  Every call below
// returns before any launch, so the program needs no GPU.  Built and run by
//
//     make -C <package>/csrc asan-requests-large
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
  const int64_t LANES = 1ll << 22, ENTRIES = 1ll << 30;
  // ---- the workspace sizes
  EXPECT(dcnr_requests_large_workspace_size(1, 0) > 0);
  EXPECT(dcnr_requests_large_workspace_size(1, 4097) >= size_t(49) * 4097);
  EXPECT(dcnr_requests_large_workspace_size(5, 20000) >= size_t(49) * 20000);
  EXPECT(dcnr_requests_large_workspace_size(LANES, ENTRIES) >= size_t(49) << 30);
  EXPECT(dcnr_requests_large_workspace_size(0, 100) == 0);
  EXPECT(dcnr_requests_large_workspace_size(-1, 100) == 0);
  EXPECT(dcnr_requests_large_workspace_size(1, -1) == 0);
  EXPECT(dcnr_requests_large_workspace_size(LANES + 1, 100) == 0);
  EXPECT(dcnr_requests_large_workspace_size(1, ENTRIES + 1) == 0);
  EXPECT(dcnr_requests_large_workspace_size(INT64_MAX, INT64_MAX) == 0);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(1) > 0);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(6000) >= size_t(5) * 6000);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(ENTRIES) >= size_t(5) << 30);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(0) == 0);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(-1) == 0);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(ENTRIES + 1) == 0);
  EXPECT(dcnr_mmr_rerank_large_workspace_size(INT64_MAX) == 0);

  const int64_t* pos = fake<const int64_t>(1);
  const int64_t* pos_off = fake<const int64_t>(2);
  const int64_t* knn = fake<const int64_t>(3);
  const int32_t* nbr = fake<const int32_t>(4);
  const int64_t* set_rows = fake<const int64_t>(5);
  const int64_t* set_off = fake<const int64_t>(6);
  const int32_t* sidx = fake<const int32_t>(7);
  const int32_t* lreq = fake<const int32_t>(8);
  const int64_t* st_off = fake<const int64_t>(9);
  int64_t* out_rows = fake<int64_t>(10);
  int32_t* cnt = fake<int32_t>(11);
  int32_t* status = fake<int32_t>(12);
  int64_t* offsets = fake<int64_t>(13);
  void* ws = fake<void>(14);
  const size_t big = size_t(1) << 40;
  const int64_t R = 8, Q = 900, L = 2, N = 9900, NI = 5000;

  // ---- dcnr_requests_large_candidates
  auto CAND = [](const int64_t* pos, const int64_t* pos_off, int64_t R, int64_t Q, const int64_t* knn,
                 const int32_t* nbr, int32_t kt, int32_t k, const int64_t* srows, int64_t nsr,
                 const int64_t* soff, int32_t S, const int32_t* a, const int32_t* e, const int32_t* f,
                 int64_t ni, const int32_t* lreq, const int64_t* stoff, int64_t L, int64_t n,
                 int64_t* orows, int32_t* cnt, int32_t* status, int64_t* offs, void* ws, size_t bytes) {
    return dcnr_requests_large_candidates(pos, pos_off, R, Q, knn, nbr, kt, k, srows, nsr, soff, S, a, e, f,
                                          20, ni, lreq, stoff, L, n, orows, cnt, status, offs, nullptr,
                                          nullptr, ws, bytes, nullptr);
  };
  // ... with everything in front of L as a good call has it
  auto CAND_OK = [&](int64_t L, int64_t n, int64_t* orows, int32_t* cnt, int32_t* status, int64_t* offs,
                     void* ws, size_t bytes) {
    return CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
                st_off, L, n, orows, cnt, status, offs, ws, bytes);
  };
  // no lanes: nothing to do, whatever else is null
  EXPECT(CAND(nullptr, nullptr, R, Q, nullptr, nullptr, 0, 11, nullptr, 0, nullptr, 0, nullptr, nullptr,
              nullptr, NI, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == DCNR_OK);
  // negative lengths
  EXPECT(CAND_OK(-1, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, -1, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, -1, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, -1, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 0, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, -1, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, -1, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, 0, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  // a table narrower than k
  EXPECT(CAND(pos, pos_off, R, Q, nullptr, nbr, 10, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  // a needed null pointer
  EXPECT(CAND(nullptr, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, nullptr, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, nullptr, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, nullptr, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, nullptr, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, nullptr, 0, nullptr, 0, nullptr, nullptr, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);   // indices, no sets
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, nullptr,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              nullptr, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, N, nullptr, cnt, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, N, out_rows, nullptr, status, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, N, out_rows, cnt, nullptr, offsets, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, N, out_rows, cnt, status, nullptr, ws, big) == DCNR_BAD_ARG);
  EXPECT(CAND_OK(L, N, out_rows, cnt, status, offsets, nullptr, big) == DCNR_BAD_ARG);
  // shapes the call does not take
  EXPECT(CAND_OK(LANES + 1, N, out_rows, cnt, status, offsets, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(CAND_OK(L, ENTRIES + 1, out_rows, cnt, status, offsets, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 65, set_rows, 100, set_off, 3, sidx, sidx, sidx, NI, lreq,
              st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 1ll << 31, set_off, 3, sidx, sidx, sidx, NI,
              lreq, st_off, L, N, out_rows, cnt, status, offsets, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(CAND(pos, pos_off, R, Q, knn, nullptr, 0, 11, set_rows, 100, set_off, 3, sidx, sidx, sidx,
              (1ll << 38) + 1, lreq, st_off, L, N, out_rows, cnt, status, offsets, ws, big) ==
         DCNR_UNSUPPORTED_SHAPE);
  // the workspace
  const size_t need = dcnr_requests_large_workspace_size(L, N);
  EXPECT(CAND_OK(L, N, out_rows, cnt, status, offsets, ws, 0) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(CAND_OK(L, N, out_rows, cnt, status, offsets, ws, need / 4) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(CAND_OK(L, ENTRIES, out_rows, cnt, status, offsets, ws, need) == DCNR_WORKSPACE_TOO_SMALL);

  // ---- dcnr_requests_large_ranking_batch
  const int64_t* users = fake<const int64_t>(15);
  const int64_t* icat = fake<const int64_t>(16);
  const float* inum = fake<const float>(17);
  int64_t* uo = fake<int64_t>(18);
  int64_t* io = fake<int64_t>(19);
  int64_t* co = fake<int64_t>(20);
  float* no = fake<float>(21);
#define BATCH(rows, offs, L, n, lreq, R, users, icat, K, inum, F, ni, uo, io, co, no) \
  dcnr_requests_large_ranking_batch(rows, offs, L, n, lreq, R, users, icat, K, inum, F, ni, uo, io, co, no, nullptr)
  EXPECT(BATCH(nullptr, nullptr, 0, 0, nullptr, R, nullptr, nullptr, 3, nullptr, 4, NI, nullptr, nullptr, nullptr,
               nullptr) == DCNR_OK);
  EXPECT(BATCH(out_rows, offsets, L, 0, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_OK);
  EXPECT(BATCH(out_rows, offsets, -1, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, -1, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, 0, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, 0, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, R, users, icat, 3, inum, 4, 0, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, R, users, icat, -1, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(nullptr, offsets, L, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, nullptr, L, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, nullptr, R, users, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, R, nullptr, icat, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, R, users, nullptr, 3, inum, 4, NI, uo, io, co, no) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, L, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, nullptr) == DCNR_BAD_ARG);
  EXPECT(BATCH(out_rows, offsets, LANES + 1, N, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) ==
         DCNR_UNSUPPORTED_SHAPE);
  EXPECT(BATCH(out_rows, offsets, L, ENTRIES + 1, lreq, R, users, icat, 3, inum, 4, NI, uo, io, co, no) ==
         DCNR_UNSUPPORTED_SHAPE);

  // ---- dcnr_requests_large_rank_mmr
  const float* logits = fake<const float>(22);
  const float* table = fake<const float>(23);
  const float* inv = fake<const float>(24);
  const float* lam = fake<const float>(25);
  const int32_t* topk = fake<const int32_t>(26);
  float* out_logits = fake<float>(27);
#define RANK(logits, n, rows, offs, L, table, inv, d, ni, lam, topk, orows, ologits, cnt, status, ws, bytes) \
  dcnr_requests_large_rank_mmr(logits, n, rows, offs, L, table, inv, d, ni, lam, topk, orows, ologits, cnt, \
                               status, ws, bytes, nullptr)
  EXPECT(RANK(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 16, NI, nullptr, nullptr, nullptr, nullptr,
              nullptr, nullptr, nullptr, 0) == DCNR_OK);
  EXPECT(RANK(logits, -1, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, -1, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 0, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 257, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, 0, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(nullptr, N, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, nullptr, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, nullptr, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, nullptr, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, nullptr, topk, out_rows, out_logits, cnt,
              status, ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, lam, nullptr, out_rows, out_logits, cnt,
              status, ws, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, nullptr, cnt, status, ws,
              big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              nullptr, big) == DCNR_BAD_ARG);
  EXPECT(RANK(logits, N, out_rows, offsets, LANES + 1, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt,
              status, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(RANK(logits, ENTRIES + 1, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt,
              status, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, 0) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(RANK(logits, N, out_rows, offsets, L, table, inv, 16, NI, lam, topk, out_rows, out_logits, cnt, status,
              ws, size_t(48) * N) == DCNR_WORKSPACE_TOO_SMALL);

  // ---- dcnr_mmr_rerank_large
  int64_t* out_pos = fake<int64_t>(28);
#define MMR(table, inv, d, rows, scores, n, topk, opos, cnt, ws, bytes) \
  dcnr_mmr_rerank_large(table, inv, d, rows, scores, n, 0.7f, topk, opos, cnt, ws, bytes, nullptr)
  EXPECT(MMR(nullptr, nullptr, 16, nullptr, nullptr, 0, 20, nullptr, nullptr, nullptr, 0) == DCNR_OK);
  EXPECT(MMR(table, inv, 16, out_rows, logits, -1, 20, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 0, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(nullptr, inv, 16, out_rows, logits, 6000, 20, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, nullptr, 16, out_rows, logits, 6000, 20, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, nullptr, logits, 6000, 20, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, out_rows, nullptr, 6000, 20, out_pos, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 20, nullptr, cnt, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 20, out_pos, nullptr, ws, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 20, out_pos, cnt, nullptr, big) == DCNR_BAD_ARG);
  EXPECT(MMR(table, inv, 0, out_rows, logits, 6000, 20, out_pos, cnt, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(MMR(table, inv, 257, out_rows, logits, 6000, 20, out_pos, cnt, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(MMR(table, inv, 16, out_rows, logits, ENTRIES + 1, 20, out_pos, cnt, ws, big) == DCNR_UNSUPPORTED_SHAPE);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 20, out_pos, cnt, ws, 0) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(MMR(table, inv, 16, out_rows, logits, 6000, 20, out_pos, cnt, ws,
             dcnr_mmr_rerank_large_workspace_size(6000) - 1) == DCNR_WORKSPACE_TOO_SMALL);
  EXPECT(dcnr_last_error() != nullptr);
  std::printf("asan_requests_large_args: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
