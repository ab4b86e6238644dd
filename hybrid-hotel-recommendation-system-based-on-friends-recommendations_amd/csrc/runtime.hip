// What every libdcnr translation unit shares at run time: the thread's last
// error, the per-kernel dynamic-LDS limit, the optional per-launch profiling
// (ProfScope, dcnr_profile_*) and dcnr_check_errors.  No kernels.
#include "dcnr_internal.h"

#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace dcnr {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

dcnr_status set_max_dyn_lds(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> done;
  int dev = 0;
  DCNR_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  size_t& cur = done[{kernel, dev}];
  if (bytes > cur) {
    DCNR_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    cur = bytes;
  }
  return DCNR_OK;
}

// ------------------------------------------------------------ profiling
// Optional per-launch HIP-event timing by kernel class (dcnr_profile_*).
// Each record carries the launch's ALGORITHMIC bytes (the operands the
// function must move: inputs read once, outputs written once; 0 = not
// accounted) so the bench prices every kernel class against HBM.
struct ProfRec { int cat; double bytes; hipEvent_t a, b; };
static std::mutex g_pm;
static bool g_prof = false;
static int g_prof_mode = 0;   // 1: every class, each launch alone; 2: gemm_dw only, concurrent
static std::vector<ProfRec> g_recs;
static std::vector<hipEvent_t> g_pool;

static hipEvent_t prof_event() {
  if (!g_pool.empty()) { hipEvent_t e = g_pool.back(); g_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

ProfScope::ProfScope(int c, hipStream_t st, double nbytes) : cat(c), s(st), bytes(nbytes) {
  if (!g_prof || (g_prof_mode == 2 && c != DCNR_K_GEMM_DW)) return;
  std::lock_guard<std::mutex> lk(g_pm);
  a = prof_event();
  (void)hipEventRecord(a, s);
}

ProfScope::~ProfScope() {
  if (!a) return;
  std::lock_guard<std::mutex> lk(g_pm);
  hipEvent_t b = prof_event();
  (void)hipEventRecord(b, s);
  g_recs.push_back(ProfRec{cat, bytes, a, b});
}

bool prof_side_stream_ok() { return !g_prof || g_prof_mode == 2; }

}  // namespace dcnr

using namespace dcnr;

extern "C" {

int dcnr_abi_version(void) { return DCNR_ABI_VERSION; }
const char* dcnr_last_error(void) { return g_err; }

void dcnr_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_pm);
  g_prof = on != 0;
  g_prof_mode = on;
}

dcnr_status dcnr_profile_collect(double* ms, int64_t* launches, int32_t n) {
  return dcnr_profile_collect_bytes(ms, launches, nullptr, n);
}

dcnr_status dcnr_profile_collect_bytes(double* ms, int64_t* launches, double* bytes, int32_t n) {
  std::vector<ProfRec> recs;
  {
    std::lock_guard<std::mutex> lk(g_pm);
    recs.swap(g_recs);
  }
  for (int i = 0; i < n; ++i) {
    if (ms) ms[i] = 0.0;
    if (launches) launches[i] = 0;
    if (bytes) bytes[i] = 0.0;
  }
  dcnr_status st = DCNR_OK;
  for (auto& r : recs) {
    float t = 0.f;
    if (hipEventSynchronize(r.b) != hipSuccess || hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) {
      set_error("profile: event query failed");
      st = DCNR_HIP_ERROR;
    }
    if (r.cat >= 0 && r.cat < n) {
      if (ms) ms[r.cat] += t;
      if (launches) launches[r.cat] += 1;
      if (bytes) bytes[r.cat] += r.bytes;
    }
  }
  std::lock_guard<std::mutex> lk(g_pm);
  for (auto& r : recs) { g_pool.push_back(r.a); g_pool.push_back(r.b); }
  return st;
}

dcnr_status dcnr_check_errors(void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  if (!ws || ws_bytes < 4) { set_error("bad workspace"); return DCNR_BAD_ARG; }
  int flag = 0;
  DCNR_HIP(hipMemcpyAsync(&flag, ws, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
  DCNR_HIP(hipStreamSynchronize((hipStream_t)stream));
  if (flag) {
    set_error("index out of range in self");
    return DCNR_INDEX_OOB;
  }
  return DCNR_OK;
}

}  // extern "C"
