// The train / eval step of libdcnr's C ABI (include/dcnr.h): sequences the
// DCN-R forward/backward kernels on one HIP stream over caller-owned memory.
// (Every other entry point stands beside its kernels, in that subsystem's file.)
//
// Forward  = DCN_RecSys.forward (train.py:155-170):
//   gather+x0+cross (1 kernel) -> initial Linear (MFMA GEMM) ->
//   per ResBlock: L1 GEMM -> BN1 stats/finalize -> BN1+ReLU+dropout ->
//                 L2 GEMM -> BN2 stats/finalize -> BN2 + residual + ReLU
//   -> deep head dot -> logits
// Backward = loss.backward() (train.py:225), reverse order, BN backward with
// deterministic fp64 column reductions, dW by split-K MFMA GEMMs over the batch,
// cross backward + dense embedding-grad scatter in one kernel.
#include "dcnr_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

namespace dcnr {
namespace {

// Flags of the fork/join events between the caller's stream and the side
// stream (both on this device: a device-scope release/acquire orders them;
// without the system-scope fence the step measured 4.019 vs 4.051 ms,
// alternating A/B x3 on one box, profiles/lab/r03x_event_fence_ab.txt).
constexpr unsigned SYNC_EV = hipEventDisableTiming | hipEventDisableSystemFence;

// Measured and rejected side-stream pipe variants:
// the apply pass's own completion event as the dependency (+1.4 %), the
// weight-gradient call after the dX GEMM (+3.5 %), fewer workgroups for the
// overlapped weight-gradient GEMMs, BN statistics reduced by the producing
// GEMM's last workgroup (+2.3-3.7 %).

// One side stream per device (created on first use, never destroyed) for the
// backward's work that does not depend on the deep tower; fork/join events
// per call.
dcnr_status side_stream(hipStream_t* out) {
  static std::mutex mu;
  static hipStream_t streams[64] = {};
  int dev = 0;
  DCNR_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) {
    set_error("side stream: device %d out of range", dev);
    return DCNR_BAD_ARG;
  }
  std::lock_guard<std::mutex> lk(mu);
  if (!streams[dev]) DCNR_HIP(hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking));
  *out = streams[dev];
  return DCNR_OK;
}
// Every exit path orders the side stream's work before the caller's stream:
// an error return between fork() and join() (a failed hook, a too-small
// scratch) must not let the caller free buffers the side stream still
// writes, so the destructor joins whatever was not joined.
struct SideJoin {
  hipStream_t side = nullptr, main = nullptr;
  hipEvent_t fork_ev = nullptr, join_ev = nullptr, mark_ev = nullptr;
  bool recorded = false, joined = false;
  dcnr_status fork(hipStream_t s) {
    TRY(side_stream(&side));
    DCNR_HIP(hipEventCreateWithFlags(&fork_ev, SYNC_EV));
    DCNR_HIP(hipEventCreateWithFlags(&join_ev, SYNC_EV));
    DCNR_HIP(hipEventRecord(fork_ev, s));
    DCNR_HIP(hipStreamWaitEvent(side, fork_ev, 0));
    main = s;
    return DCNR_OK;
  }
  dcnr_status record() {
    DCNR_HIP(hipEventRecord(join_ev, side));
    recorded = true;
    return DCNR_OK;
  }
  dcnr_status join(hipStream_t s) {
    DCNR_HIP(hipStreamWaitEvent(s, join_ev, 0));
    joined = true;
    return DCNR_OK;
  }
  // an intermediate point of the side stream's work that `s` waits for alone
  dcnr_status mark() {
    DCNR_HIP(hipEventCreateWithFlags(&mark_ev, SYNC_EV));
    DCNR_HIP(hipEventRecord(mark_ev, side));
    return DCNR_OK;
  }
  dcnr_status wait_mark(hipStream_t s) {
    DCNR_HIP(hipStreamWaitEvent(s, mark_ev, 0));
    return DCNR_OK;
  }
  ~SideJoin() {
    if (main && join_ev && !joined) {   // error path: join everything enqueued so far
      (void)hipEventRecord(join_ev, side);
      (void)hipStreamWaitEvent(main, join_ev, 0);
    }
    if (mark_ev) (void)hipEventDestroy(mark_ev);
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (join_ev) (void)hipEventDestroy(join_ev);
  }
};

// dcnr_grad_ready_fn of the model desc, if any
dcnr_status grads_ready(const dcnr_model_desc* desc, int group, hipStream_t s) {
  if (!desc->grad_ready) return DCNR_OK;
  const int rc = desc->grad_ready(desc->grad_ready_ctx, group, (void*)s);
  if (rc != 0) {
    set_error("grad_ready hook failed (%d) for gradient group %d", rc, group);
    return DCNR_HIP_ERROR;
  }
  return DCNR_OK;
}

constexpr int MAX_CAT = 64;
constexpr int MAX_RES = 8;
constexpr int MAX_CROSS = 7;
constexpr int64_t PART_CHUNKS = 2100;  // >= rowcol chunk count (2048 target + rounding)

struct Dims {
  int K, D, Dp, H, Hp, L, R, prec, es;
  int widths[2 + MAX_CAT];
  int64_t rows[2 + MAX_CAT];
  float dropout;
};

dcnr_status make_dims(const dcnr_model_desc* d, Dims* o) {
  if (!d) { set_error("null desc"); return DCNR_BAD_ARG; }
  if (d->n_cat < 0 || d->n_cat > MAX_CAT || (d->n_cat > 0 && !d->cat_rows)) {
    set_error("n_cat=%d unsupported (max %d)", d->n_cat, MAX_CAT);
    return DCNR_BAD_ARG;
  }
  if (d->n_res < 1 || d->n_res > MAX_RES) {
    set_error("n_res_blocks=%d unsupported (1..%d)", d->n_res, MAX_RES);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (d->n_cross < 0 || d->n_cross > MAX_CROSS) {
    set_error("n_cross_layers=%d unsupported (0..%d)", d->n_cross, MAX_CROSS);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  if (d->emb_dim < 1 || d->hidden < 1 || d->n_num < 0 || d->n_users < 1 || d->n_items < 1) {
    set_error("bad model dims");
    return DCNR_BAD_ARG;
  }
  if (d->precision != DCNR_PREC_FP32 && d->precision != DCNR_PREC_BF16) {
    set_error("bad precision %d", d->precision);
    return DCNR_BAD_ARG;
  }
  o->K = d->n_cat;
  o->widths[0] = o->widths[1] = d->emb_dim;
  o->rows[0] = d->n_users;
  o->rows[1] = d->n_items;
  int D = 2 * d->emb_dim;
  for (int k = 0; k < d->n_cat; ++k) {
    int64_t n = d->cat_rows[k];
    if (n < 1) { set_error("cat table %d has %lld rows", k, (long long)n); return DCNR_BAD_ARG; }
    int w = (int)std::sqrt((double)n) + 1;  // train.py:139 int(np.sqrt(n_cat)) + 1
    while ((int64_t)(w - 1) * (w - 1) > n) --w;        // guard fp rounding of sqrt
    while ((int64_t)w * w <= n) ++w;
    o->widths[2 + k] = w;
    o->rows[2 + k] = n;
    D += w;
  }
  D += d->n_num;
  o->D = D;
  o->Dp = (int)rup(D, 8);
  o->H = d->hidden;
  o->Hp = (int)rup(d->hidden, 8);
  o->L = d->n_cross;
  o->R = d->n_res;
  o->prec = d->precision;
  o->es = d->precision == DCNR_PREC_BF16 ? 2 : 4;
  o->dropout = d->dropout;
  if (o->D > 1024) {
    set_error("input_dim=%d unsupported (max 1024)", o->D);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  // the row passes (elementwise.hip run_rowcol) give a thread 8 bf16 / 4 fp32
  // columns of a row and a row at most one 256-thread block
  const int hp_max = d->precision == DCNR_PREC_BF16 ? 2048 : 1024;
  if (o->Hp > hp_max) {
    set_error("hidden_dim=%d unsupported in %s precision (padded to %d, max %d)", o->H,
              d->precision == DCNR_PREC_BF16 ? "bf16" : "fp32", o->Hp, hp_max);
    return DCNR_UNSUPPORTED_SHAPE;
  }
  return DCNR_OK;
}

// ------------------------------------------------- algorithmic byte counts
// (profiling only): one [B][Hp] activation, its 1-bit mask, one gathered
// input row (ids + embedding rows + dense features), a weight
double act_b(const Dims& d, int64_t B) { return (double)B * d.Hp * d.es; }
double mask_b(const Dims& d, int64_t B) { return (double)B * d.Hp / 8.0; }
double gather_row_b(const Dims& d, int n_num) {
  double w = 0;
  for (int t = 0; t < 2 + d.K; ++t) w += d.widths[t];
  return 8.0 * (2 + d.K) + 4.0 * w + 4.0 * n_num;
}
double w_b(const Dims& d, int K) { return (double)d.Hp * K * d.es; }

// ------------------------------------------------------------- workspace
struct BnBufs { float *scale, *shift, *mean, *invstd; };

struct Layout {
  int* err;
  void* W0p; void* W0t; float* b0p;
  void* W1p[MAX_RES]; void* W1t[MAX_RES]; float* b1p[MAX_RES];
  void* W2p[MAX_RES]; void* W2t[MAX_RES]; float* b2p[MAX_RES];
  void* x0;
  void* h[MAX_RES + 1];
  void* t1[MAX_RES]; void* t2[MAX_RES];
  void* a1;                 // eval: BN1/ReLU output scratch; train: backward scratch (dt1)
  void* a1s[MAX_RES];       // train: each block's dropout(relu(BN1(t1))), saved for dW2
  float* zc; float* zdeep;
  float* headp;             // eval (Plan::eval_headp): [head parts][B] deep-head partial dots
  char* twp;                // eval (Plan::tower): the packed weight slices
  BnBufs bn[2 * MAX_RES];
  float* part; double* sums; float* coef;
  double* red2; int* red_cnt;   // reduce_fused scratch (counters zeroed by pack_all)
  // backward
  void* G; void* dt2; void* du; void* da;
  // per-block backward buffers: all alias dt2/du/da/a1 unless DCNR_FLAG_KEEP_INTERMEDIATES
  // gives each block its own (Plan::own_dt: dt2k / dt1k a set per block)
  void* duk[MAX_RES]; void* dt2k[MAX_RES]; void* dak[MAX_RES]; void* dt1k[MAX_RES];
  float* dx0;                 // deep part of dL/dx0, [B][Dq] (Dq = Dp rounded up to 32)
  float* slab; int64_t slab_elems;
  float* slab2;   // the side stream's weight gradients alternate slabs (DwPipe)
  float* sc;                 // forward -> backward cross scalars [B][2L+1]
  float* xcoef; float* xalpha;  // [B][L+1] each (cross_bwd.hip)
  void* cscratch; size_t cscratch_bytes;
  // 1-bit keep masks for the backward GEMM epilogues (Plan::masks):
  // mask_a1[j] = [a1_j != 0], mask_h[j] = [h_j > 0] (j >= 1; j = R: Plan::rank1)
  uint8_t* mask_a1[MAX_RES]; uint8_t* mask_h[MAX_RES + 1];
  EmbSortBufs emb;                              // deterministic embedding backward
  double* bce_part;
  uint8_t* rowmap; size_t rowmap_bytes;   // DCNR_FLAG_ROW_MAP: byte per table row (last in ws)
  size_t total;
};

// leading dimension of the deep dx0: 32-float (128-B) rows so that each
// embedding table's segment of a row is line-aligned for embed_bwd.hip
int dq_of(const Dims& d) { return (int)rup(d.Dp, 32); }

// ------------------------------------------------------------------ plan
// The predicates below are called from make_plan alone.
// the backward GEMM epilogues read 1-bit keep masks (bf16 path, mask rows of
// whole 32-bit words) instead of the bf16 activations
bool masks_ok(const Dims& d) { return d.prec == DCNR_PREC_BF16 && d.Hp % 32 == 0; }
// Stats epilogues of the streaming GEMM (BN column partials produced by the
// GEMM that writes the BN input / the BN output gradient) -- bf16 only.
bool epi_stats_ok(const Dims& d) { return masks_ok(d) && gemm_ws_supported(d.Hp, d.Hp); }
// Eval forward with BatchNorm (running statistics) + ReLU (+ residual) in the
// streaming GEMM's epilogue: no t1/t2 round trip through HBM and no rowwise
// passes (bf16, gemm_ws shapes).
bool eval_fuse_ok(const Dims& d) { return d.prec == DCNR_PREC_BF16 && gemm_ws_supported(d.Hp, d.Hp); }

// The eval forward's deep tower as one persistent launch (tower.hip): eval, bf16,
// the shapes it covers (input width <= 512, hidden <= 512), not when the
// stage tests ask for every intermediate, and from TOWER_MIN_B samples (or
// with DCNR_FLAG_FUSED_TOWER): one 128-sample tile per CU walks all 2R+1
// layers in sequence, ~150 us however few tiles there are, while the
// layer-by-layer path spreads each layer over the chip (bench model: 179 vs
// 139 us at 4096 samples, 622 vs 806 us at 131072).
constexpr int64_t TOWER_MIN_B = 16384;
bool tower_ok(const Dims& d, uint32_t flags, int64_t B) {
  const bool size_ok = B >= TOWER_MIN_B || (flags & DCNR_FLAG_FUSED_TOWER);
  return !(flags & DCNR_FLAG_KEEP_INTERMEDIATES) && size_ok && d.prec == DCNR_PREC_BF16 &&
         tower_supported(d.Dp, d.H, d.R);
}

// Which kernels a call runs, decided once from (model, flags, mode, B).  The
// layout (what gets a buffer), the forward (what is written) and the backward
// (what is read) follow these fields and nothing else, so they cannot disagree.
struct Plan {
  bool train, keep;  // mode; DCNR_FLAG_KEEP_INTERMEDIATES
  // ---- eval
  bool tower;        // the fused deep tower: x0, zc and the packed slices are the whole layout
  bool eval_epi;     // BN + ReLU (+ residual) in the GEMM epilogues
  bool eval_headp;   // ... the last GEMM ending in the deep head's partial dots (no h_R)
  // ---- the layer-by-layer forward (train, and eval without the epilogues)
  bool head_fused;   // the last block's BN2 apply + residual + ReLU + head dot + logits in one pass
  // ---- train
  bool masks;        // the forward stores the 1-bit keep masks
  bool stats_epi;    // BN column partials from the forward and dX GEMM epilogues
  bool xbn;          // ... and the BN backward's row passes folded into them (256 < Hp <= 512)
  bool rebuild_hR;   // the backward's BN2 statistics pass rebuilds h_R from t2, h_{R-1} and the
                     // BN2 affine; the head pass stores h_R only with `keep` (stage tests)
  bool rank1;        // the head pass stores [h_R > 0]; the last BN2 apply is the rank-1 form over it
  bool head_stats;   // DCNR_FLAG_HEAD_STATS: dcnr_forward_bce's head pass goes on to dz and the last
                     // block's BN2-backward partials (left in `part`); the backward runs no
                     // statistics pass for that block
  bool r1_resid;     // ... and that block's du is never stored: its dX GEMM (RESID_BN with the
                     // operand transform, R > 1) rebuilds the rank-1 residual in the epilogue
  bool own_dt;       // every block its own dt2 / dt1 buffers (else one shared set)
  bool rowmap;       // DCNR_FLAG_ROW_MAP
  int dw_lag;        // DwPipe: the main stream waits for the dW GEMM this many calls back (1 << 30: never)
};

Plan make_plan(const Dims& d, uint32_t flags, int mode, int64_t B, bool sync_bn = false) {
  Plan p{};
  const bool bf16p = d.prec == DCNR_PREC_BF16;
  p.train = mode == DCNR_TRAIN;
  p.keep = (flags & DCNR_FLAG_KEEP_INTERMEDIATES) != 0;
  p.head_fused = bn_add_relu_head_supported(d.prec, d.Hp);
  if (!p.train) {
    p.tower = tower_ok(d, flags, B);
    p.eval_epi = !p.tower && eval_fuse_ok(d);
    // (32-bit buffer offsets into the head partials: at Hp = 512 up to ~33M
    // rows; larger batches take the unfused, M-chunked tail)
    p.eval_headp = p.eval_epi && !p.keep &&
                   (int64_t)B * gemm_ws_head_parts(d.Hp) * 4 < (int64_t(1) << 31);
    return p;
  }
  p.masks = masks_ok(d);
  p.stats_epi = epi_stats_ok(d);
  p.xbn = p.stats_epi && gemm_ws_xbn_supported(NT_EPI_DROP_BN, d.Hp, d.Hp);
  p.rebuild_hR = bf16p && p.head_fused;
  p.rank1 = p.masks && p.head_fused;
  // (not with the stage tests' stored intermediates, which include that
  // block's du; not with SyncBN, whose hook sums the statistics between the
  // partials and their use)
  p.head_stats = (flags & DCNR_FLAG_HEAD_STATS) && p.rank1 && p.rebuild_hR && !p.keep && !sync_bn;
  // (R = 1: the last block is block 0, whose RESID_SUM GEMM reads the stored du)
  p.r1_resid = p.head_stats && p.xbn && d.R > 1;
  // bf16: every residual block has its own dt2 / dt1 buffers: the side
  // stream's weight-gradient GEMMs read them while the main stream goes on,
  // and the main stream never waits for the side stream inside the backward
  // (4.029-4.044 vs 4.068-4.075 ms per step with two sets alternating by
  // block parity and a wait for call n-3, same box, profiles/lab/r04s_dt_per_block_ab.txt;
  // +0.54 GB of workspace at the bench shape)
  p.own_dt = !p.keep && bf16p && d.R > 1;
  p.rowmap = (flags & DCNR_FLAG_ROW_MAP) != 0;
  p.dw_lag = p.keep || p.own_dt ? 1 << 30 : 1;
  return p;
}

Layout make_layout(const Dims& d, int64_t B, const Plan& pl, void* ws) {
  Layout L;
  memset(&L, 0, sizeof(L));
  Bump b(ws);
  const bool train = pl.train, keep = pl.keep;
  const size_t es = d.es;
  const size_t act = (size_t)B * d.Hp * es;
  L.err = (int*)b.take(256);
  if (pl.tower) {   // x0, zc, the packed slices: nothing of the tower in HBM
    L.x0 = b.take((size_t)B * d.Dp * es);
    L.zc = (float*)b.take(B * 4);
    L.twp = (char*)b.take((size_t)tower_ws_bytes(d.H, d.R));
    L.total = b.off + 256;
    return L;
  }
  L.W0p = b.take((size_t)d.Hp * d.Dp * es);
  L.W0t = train ? b.take((size_t)d.Dp * d.Hp * es) : nullptr;
  L.b0p = (float*)b.take(d.Hp * 4);
  for (int j = 0; j < d.R; ++j) {
    L.W1p[j] = b.take((size_t)d.Hp * d.Hp * es);
    L.W2p[j] = b.take((size_t)d.Hp * d.Hp * es);
    L.W1t[j] = train ? b.take((size_t)d.Hp * d.Hp * es) : nullptr;
    L.W2t[j] = train ? b.take((size_t)d.Hp * d.Hp * es) : nullptr;
    L.b1p[j] = (float*)b.take(d.Hp * 4);
    L.b2p[j] = (float*)b.take(d.Hp * 4);
  }
  L.x0 = b.take((size_t)B * d.Dp * es);
  if (train) {
    for (int j = 0; j <= d.R; ++j) L.h[j] = b.take(act);
    for (int j = 0; j < d.R; ++j) { L.t1[j] = b.take(act); L.t2[j] = b.take(act); }
  } else {
    void* h0 = b.take(act);
    void* h1 = b.take(act);
    for (int j = 0; j <= d.R; ++j) L.h[j] = (j & 1) ? h1 : h0;
    void* t = b.take(act);
    for (int j = 0; j < d.R; ++j) L.t1[j] = L.t2[j] = t;
  }
  L.a1 = b.take(act);
  if (train)
    for (int j = 0; j < d.R; ++j) L.a1s[j] = b.take(act);
  if (pl.masks) {
    const size_t mb = (size_t)B * d.Hp / 8;
    for (int j = 0; j < d.R; ++j) L.mask_a1[j] = (uint8_t*)b.take(mb);
    for (int j = 1; j < d.R; ++j) L.mask_h[j] = (uint8_t*)b.take(mb);
    if (pl.rank1) L.mask_h[d.R] = (uint8_t*)b.take(mb);
  }
  L.zc = (float*)b.take(B * 4);
  L.zdeep = (float*)b.take(B * 4);
  if (pl.eval_headp) L.headp = (float*)b.take((size_t)B * gemm_ws_head_parts(d.Hp) * 4);
  for (int i = 0; i < 2 * d.R; ++i) {
    L.bn[i].scale = (float*)b.take(d.Hp * 4);
    L.bn[i].shift = (float*)b.take(d.Hp * 4);
    L.bn[i].mean = (float*)b.take(d.Hp * 4);
    L.bn[i].invstd = (float*)b.take(d.Hp * 4);
  }
  L.part = (float*)b.take((size_t)PART_CHUNKS * 3 * d.Hp * 4);
  L.sums = (double*)b.take((size_t)(3 * d.Hp + 1) * 8);
  L.coef = (float*)b.take((size_t)3 * d.Hp * 4);
  L.red2 = (double*)b.take((size_t)RED_G * 3 * d.Hp * 8);
  L.red_cnt = (int*)b.take(CNT_SLOTS * 4);
  if (train) {
    L.G = b.take(act);
    L.dt2 = b.take(act);
    L.du = b.take(act);
    L.da = b.take(act);
    L.dx0 = (float*)b.take((size_t)B * dq_of(d) * 4);
    // split-K slabs: the fp32 path adapts its splits to 64; the bf16 kernel's
    // split count depends on the tile count (narrow H -> more splits)
    L.slab_elems = std::max<int64_t>({(int64_t)64 * d.Hp * std::max(d.Hp, d.Dp),
                                      (int64_t)gemm_dw_splits(d.Hp, d.Hp, B) * d.Hp * d.Hp,
                                      (int64_t)gemm_dw_splits(d.Hp, d.Dp, B) * d.Hp * d.Dp});
    L.slab = (float*)b.take((size_t)L.slab_elems * 4);
    L.slab2 = (float*)b.take((size_t)L.slab_elems * 4);
    L.sc = (float*)b.take((size_t)B * (2 * d.L + 1) * 4);
    L.xcoef = (float*)b.take((size_t)B * (d.L + 1) * 4);
    L.xalpha = (float*)b.take((size_t)B * (d.L + 1) * 4);
    L.cscratch_bytes = cross_bwd_scratch_bytes(d.D, d.L, B);
    L.cscratch = b.take(L.cscratch_bytes);
    {
      const int64_t n = (int64_t)(2 + d.K) * B;
      L.emb.ids = (uint32_t*)b.take((size_t)n * 4);
      L.emb.keys = (uint32_t*)b.take((size_t)n * 4);
      L.emb.vals = (uint32_t*)b.take((size_t)n * 4);
      L.emb.keys_s = (uint32_t*)b.take((size_t)n * 4);
      L.emb.vals_s = (uint32_t*)b.take((size_t)n * 4);
      L.emb.tmp_bytes = emb_sort_tmp_bytes(d.rows, d.widths, 2 + d.K, B);
      L.emb.tmp = b.take(L.emb.tmp_bytes);
    }
    // own_dt: blocks 0 and 1 take the shared set and a second one, later blocks a fresh set
    void *dt2b = nullptr, *dt1b = nullptr;
    if (pl.own_dt) {
      dt2b = b.take(act);
      dt1b = b.take(act);
    }
    for (int j = 0; j < d.R; ++j) {
      const bool fresh = pl.own_dt && j > 1;
      L.duk[j] = keep ? b.take(act) : L.du;
      L.dt2k[j] = keep || fresh ? b.take(act) : pl.own_dt && j == 1 ? dt2b : L.dt2;
      L.dak[j] = keep ? b.take(act) : L.da;
      L.dt1k[j] = keep || fresh ? b.take(act) : pl.own_dt && j == 1 ? dt1b : L.a1;
    }
  }
  L.bce_part = (double*)b.take(bce_ws_bytes());
  if (pl.rowmap) {   // last: every other offset as without the flag
    int64_t rows = 0;
    for (int t = 0; t < 2 + d.K; ++t) rows += d.rows[t];
    L.rowmap_bytes = (size_t)rup(rows, 256);
    L.rowmap = (uint8_t*)b.take(L.rowmap_bytes);
  }
  L.total = b.off + 256;
  return L;
}

// ------------------------------------------------------------- params
struct Params {
  const float* tab[2 + MAX_CAT];
  const float *W0, *b0;
  struct Blk {
    const float *w1, *b1, *g1, *be1; float *rm1, *rv1; int64_t* nbt1;
    const float *w2, *b2, *g2, *be2; float *rm2, *rv2; int64_t* nbt2;
  } blk[MAX_RES];
  const float* cb[MAX_CROSS]; const float* cw[MAX_CROSS];
  const float *wf, *bf;
};

Params map_params(const Dims& d, void* const* p) {
  Params P;
  int i = 0;
  for (int t = 0; t < 2 + d.K; ++t) P.tab[t] = (const float*)p[i++];
  P.W0 = (const float*)p[i++];
  P.b0 = (const float*)p[i++];
  for (int j = 0; j < d.R; ++j) {
    auto& B = P.blk[j];
    B.w1 = (const float*)p[i++]; B.b1 = (const float*)p[i++];
    B.g1 = (const float*)p[i++]; B.be1 = (const float*)p[i++];
    B.rm1 = (float*)p[i++]; B.rv1 = (float*)p[i++]; B.nbt1 = (int64_t*)p[i++];
    B.w2 = (const float*)p[i++]; B.b2 = (const float*)p[i++];
    B.g2 = (const float*)p[i++]; B.be2 = (const float*)p[i++];
    B.rm2 = (float*)p[i++]; B.rv2 = (float*)p[i++]; B.nbt2 = (int64_t*)p[i++];
  }
  for (int l = 0; l < d.L; ++l) { P.cb[l] = (const float*)p[i++]; P.cw[l] = (const float*)p[i++]; }
  P.wf = (const float*)p[i++];
  P.bf = (const float*)p[i++];
  return P;
}

struct Grads {
  float* tab[2 + MAX_CAT];
  float *W0, *b0;
  struct Blk { float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2; } blk[MAX_RES];
  float* cb[MAX_CROSS]; float* cw[MAX_CROSS];
  float *wf, *bf;
};

Grads map_grads(const Dims& d, void* const* g) {
  Grads G;
  int i = 0;
  for (int t = 0; t < 2 + d.K; ++t) G.tab[t] = (float*)g[i++];
  G.W0 = (float*)g[i++];
  G.b0 = (float*)g[i++];
  for (int j = 0; j < d.R; ++j) {
    auto& B = G.blk[j];
    B.w1 = (float*)g[i++]; B.b1 = (float*)g[i++]; B.g1 = (float*)g[i++]; B.be1 = (float*)g[i++];
    B.w2 = (float*)g[i++]; B.b2 = (float*)g[i++]; B.g2 = (float*)g[i++]; B.be2 = (float*)g[i++];
  }
  for (int l = 0; l < d.L; ++l) { G.cb[l] = (float*)g[i++]; G.cw[l] = (float*)g[i++]; }
  G.wf = (float*)g[i++];
  G.bf = (float*)g[i++];
  return G;
}

GatherDesc make_gather(const Dims& d, const Params& P, int n_num) {
  GatherDesc g;
  memset(&g, 0, sizeof(g));
  g.n_tab = 2 + d.K;
  int off = 0;
  for (int t = 0; t < g.n_tab; ++t) {
    g.tab[t] = P.tab[t];
    g.rows[t] = d.rows[t];
    g.width[t] = d.widths[t];
    g.off[t] = off;
    off += d.widths[t];
  }
  g.n_num = n_num;
  g.D = d.D;
  return g;
}

CrossParams make_cross(const Dims& d, const Params& P) {
  CrossParams c;
  memset(&c, 0, sizeof(c));
  c.L = d.L;
  for (int l = 0; l < d.L; ++l) { c.w[l] = P.cw[l]; c.b[l] = P.cb[l]; }
  c.wf_cross = P.wf + d.H;
  return c;
}

dcnr_status pack_all(const Dims& d, const Params& P, const Layout& L, bool train, hipStream_t s,
                     bool zero_err = false) {
  // weights -> padded T copies (+ transposes for backward); biases -> padded
  // f32; one launch per MAX_PACK descriptors
  std::vector<PackDesc> v;
  auto add = [&](const float* src, void* dst, void* dst_t, int rows, int cols, int ld, int ld_t,
                 int rows_p, int cols_p) {
    PackDesc p{src, dst, dst_t, rows, cols, ld, ld_t, rows_p, cols_p, 0};   // T = the precision
    v.push_back(p);
  };
  add(P.W0, L.W0p, train ? L.W0t : nullptr, d.H, d.D, d.Dp, d.Hp, d.Hp, d.Dp);
  for (int j = 0; j < d.R; ++j) {
    add(P.blk[j].w1, L.W1p[j], train ? L.W1t[j] : nullptr, d.H, d.H, d.Hp, d.Hp, d.Hp, d.Hp);
    add(P.blk[j].w2, L.W2p[j], train ? L.W2t[j] : nullptr, d.H, d.H, d.Hp, d.Hp, d.Hp, d.Hp);
  }
  auto addb = [&](const float* src, float* dst) {
    PackDesc p{src, dst, nullptr, 1, d.H, d.Hp, 0, 1, 0, 1};
    v.push_back(p);
  };
  addb(P.b0, L.b0p);
  // reduce_fused's column-group counters start at zero (a 1-row pack of 0 columns)
  v.push_back(PackDesc{P.b0, L.red_cnt, nullptr, 0, 0, CNT_SLOTS, 0, 1, 0, 1});
  // (eval, index check on: the gather's error word, in the same launch)
  if (zero_err) v.push_back(PackDesc{P.b0, L.err, nullptr, 0, 0, 8, 0, 1, 0, 1});
  for (int j = 0; j < d.R; ++j) { addb(P.blk[j].b1, L.b1p[j]); addb(P.blk[j].b2, L.b2p[j]); }
  for (size_t o = 0; o < v.size(); o += MAX_PACK) {
    PackBatch pb;
    pb.n = (int)std::min<size_t>(MAX_PACK, v.size() - o);
    for (int i = 0; i < pb.n; ++i) pb.d[i] = v[o + i];
    TRYP(DCNR_K_PACK, s, pack_weights(d.prec, pb, s));
  }
  return DCNR_OK;
}

// C = A . B^T with k-contiguous operands: bf16 -> the weight-stationary
// streaming kernel (gemm_ws.hip) when the weight fits its registers (K <= 512);
// otherwise the generic tiled MFMA kernel (fp32 parity path, K > 512).
dcnr_status gemm_nn(int prec, int epi, const GemmArgs& g, int splits, hipStream_t s) {
  if (prec == DCNR_PREC_BF16 && splits == 1 && gemm_ws_supported(g.K, g.N)) {
    NtArgs a;
    memset(&a, 0, sizeof(a));
    a.X = (const bf16*)g.A; a.ldx = g.lda; a.M = g.M; a.K = (int)g.K;
    a.W = (const bf16*)g.B; a.ldw = g.ldb; a.N = (int)g.N;
    a.C = g.C; a.ldc = g.ldc; a.bias = g.bias;
    a.R = g.resid; a.ldr = g.ldr;
    int ne = epi == EPI_STORE_RESID ? NT_EPI_RESID : (g.out_f32 ? NT_EPI_F32 : NT_EPI_BIAS);
    return gemm_ws(ne, a, s);
  }
  return gemm(prec, false, false, epi, g, splits, s);
}

dcnr_status linear_fwd(const Dims& d, const void* A, int lda, const void* W, int K,
                       const float* bias, void* out, int64_t B, hipStream_t s) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = A; g.lda = lda; g.B = W; g.ldb = K;
  g.C = out; g.ldc = d.Hp; g.bias = bias;
  g.M = B; g.N = d.Hp; g.K = K; g.k_per_split = K;
  return gemm_nn(d.prec, EPI_STORE, g, 1, s);
}

// out = relu((A W^T + b) * bn.scale + bn.shift [+ R]); with rs (the layer's
// gamma, beta, running mean, running var) the kernel makes scale / shift
// itself; with headp (needs R) no out: the deep head's partial dots with wf
dcnr_status linear_bn_relu(const Dims& d, const void* A, const void* W, const float* bias,
                           const BnBufs& bn, const void* R, void* out, int64_t B, hipStream_t s,
                           const float* const* rs = nullptr, const float* wf = nullptr,
                           float* headp = nullptr) {
  NtArgs a;
  memset(&a, 0, sizeof(a));
  a.X = (const bf16*)A; a.ldx = d.Hp; a.M = B; a.K = d.Hp;
  a.W = (const bf16*)W; a.ldw = d.Hp; a.N = d.Hp; a.Nr = d.H;
  a.C = out; a.ldc = d.Hp; a.bias = bias;
  a.R = R; a.ldr = d.Hp;
  a.bn_scale = bn.scale; a.bn_shift = bn.shift;
  if (rs) { a.bn_g = rs[0]; a.bn_b = rs[1]; a.bn_rm = rs[2]; a.bn_rv = rs[3]; }
  a.wf = wf; a.headp = headp; a.ldh = B;
  return gemm_ws(headp ? NT_EPI_BN_RESID_RELU_HEAD : R ? NT_EPI_BN_RESID_RELU : NT_EPI_BN_RELU, a, s);
}

// t = A W^T + b  and  part = BN column partials of t, shifted by b (nc rows)
dcnr_status linear_fwd_stats(const Dims& d, const Layout& L, const void* A, int lda, const void* W,
                             int K, const float* bias, void* out, int64_t B, int* nc,
                             hipStream_t s) {
  NtArgs a;
  memset(&a, 0, sizeof(a));
  a.X = (const bf16*)A; a.ldx = lda; a.M = B; a.K = K;
  a.W = (const bf16*)W; a.ldw = K; a.N = d.Hp;
  a.C = out; a.ldc = d.Hp; a.bias = bias;
  a.part = L.part;
  return gemm_ws(NT_EPI_BIAS_STATS, a, s, nc);
}

// C = mask(H) * (X W^T [+ R]) and part = [sum C, sum C*xhat(T)] (BN backward)
// xbn (optional): X is a BatchNorm backward's du; the GEMM's operand is its
// dt = bn_bwd_dt(du, xt, xbn mean / invstd, L.coef), also written to dt_out
// (the row pass folded into this GEMM, gemm_ws.hip XBN)
struct XbnOperand { const void* xt; const BnBufs* bn; void* dt_out; };
// r1 (optional, RESID_BN with xbn): R is not read; it is the rank-1
// bf16(dz (x) wf) under the 1-bit image `bits` (Plan::r1_resid)
struct Rank1Resid { const float* dz; const float* wf; const uint8_t* bits; };
dcnr_status linear_dx_bn(const Dims& d, const Layout& L, int epi, const void* X, const void* Wt,
                         const void* R, void* C, const uint8_t* Hbits, float hscale,
                         const void* T, const BnBufs& bn, int64_t B, int* nc, hipStream_t s,
                         const XbnOperand* xbn = nullptr, const Rank1Resid* r1 = nullptr) {
  NtArgs a;
  memset(&a, 0, sizeof(a));
  if (xbn) {
    a.Tx = (const bf16*)xbn->xt;
    a.xmean = xbn->bn->mean; a.xinvstd = xbn->bn->invstd; a.xcoef = L.coef;
    a.dt = (bf16*)xbn->dt_out;
  }
  a.X = (const bf16*)X; a.ldx = d.Hp; a.M = B; a.K = d.Hp;
  a.W = (const bf16*)Wt; a.ldw = d.Hp; a.N = d.Hp;
  a.C = C; a.ldc = d.Hp;
  a.R = R; a.ldr = d.Hp;
  a.hscale = hscale;
  a.Hb = (const uint32_t*)Hbits; a.ldhb = d.Hp / 32;
  a.T = (const bf16*)T; a.ldt = d.Hp;
  a.mean = bn.mean; a.invstd = bn.invstd;
  a.part = L.part;
  if (r1) {
    a.R = nullptr;
    a.r1_dz = r1->dz; a.r1_bits = (const uint32_t*)r1->bits; a.wf = r1->wf; a.Nr = d.H;
  }
  return gemm_ws(epi, a, s, nc);
}

// dW[N][Kc] = sum_b dY[b][n] X[b][k]   (real extents Nr x Kr written to out)
// bf16: the 256x256 LDS-DMA weight-gradient kernel (gemm_dw.hip), S batch
// splits, fp32 slabs summed by splitk_reduce
dcnr_status dw_args(const void* dY, int64_t ldy, int N, const void* X, int64_t ldx, int Kc, int64_t B,
                    float* slab, int64_t slab_elems, DwArgs* out) {
  // (the full-chip split count: 32 / 16 splits, leaving CUs to the main
  // stream and halving the slab, measured 2 % / 21 % slower per step)
  const int S = gemm_dw_splits(N, Kc, B);
  if ((int64_t)S * N * Kc > slab_elems) {
    set_error("wgrad: slab too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  DwArgs a;
  memset(&a, 0, sizeof(a));
  a.A = (const bf16*)dY; a.lda = ldy; a.B = (const bf16*)X; a.ldb = ldx;
  a.C = slab; a.ldc = N; a.slab_stride = (int64_t)N * Kc;   // transposed slab [Kc][N]
  a.Btot = B; a.k_per_split = rup(cdiv(B, S), 64);
  a.N = N; a.K = Kc; a.splits = S;
  *out = a;
  return DCNR_OK;
}
dcnr_status wgrad_bf16(const void* dY, int64_t ldy, int N, const void* X, int64_t ldx, int Kc,
                       int64_t B, float* slab, int64_t slab_elems, float* out, int Nr, int Kr,
                       int accumulate, hipStream_t s) {
  DwArgs a;
  TRY(dw_args(dY, ldy, N, X, ldx, Kc, B, slab, slab_elems, &a));
  TRYB(DCNR_K_GEMM_DW, s, 2.0 * B * (N + Kc) + 4.0 * Nr * Kr * (accumulate ? 2 : 1), gemm_dw(a, s));
  TRYB(DCNR_K_REDUCE, s, 4.0 * a.splits * N * Kc + 4.0 * Nr * Kr * (accumulate ? 2 : 1),
       splitk_reduce_t(slab, a.splits, (int64_t)N * Kc, N, Nr, Kr, out, accumulate, s));
  return DCNR_OK;
}

// The backward's bf16 weight gradients run on the side stream: each call's
// gemm_dw + split-K reduce are ordered after the main stream's work so far
// (its dY is complete) and overlap the main stream's next dX GEMM and BN
// passes. The operands stay alive: with a dt2 / dt1 set per block nothing
// writes a call's dY again before the join (lag: never); with one shared set
// (a single residual block) call n's enter() orders the main stream after
// call n-1's GEMM. The reduces share one slab because they are serialised
// on the side stream. join() orders the main stream after all of it. Same kernels, same order per
// output: the gradients are unchanged.
// Round 6: each call's split-K combine runs in the NEXT call's gemm_dw
// launch (its tail, over the workgroups already resident) instead of as a
// launch of its own, which beside the dX GEMMs waited for CUs (150-240 us
// for a 12 us kernel): the calls alternate slabs (L.slab, L.slab2), and the
// last call's combine is launched by join().  Same tiles, same order: the
// gradients are unchanged.
struct DwPipe {
  static constexpr int RING = 4;
  hipStream_t side = nullptr, main = nullptr;
  hipEvent_t in_ev = nullptr, done_ev = nullptr;
  hipEvent_t dw_ev[RING] = {};
  int calls = 0, lag = 1;
  bool pending = false;   // side work enqueued since the last join
  struct Combine { const float* slab; int S; int64_t stride; int ld, Nr, Kr; float* out; int acc; };
  Combine pend{};          // the last call's combine, not yet enqueued (slab != null)
  dcnr_status flush() {
    if (!pend.slab) return DCNR_OK;
    const Combine c = pend;
    pend = Combine{};
    TRYB(DCNR_K_REDUCE, side, 4.0 * c.S * c.stride + 4.0 * c.Nr * c.Kr * (c.acc ? 2 : 1),
         splitk_reduce_t(c.slab, c.S, c.stride, c.ld, c.Nr, c.Kr, c.out, c.acc, side));
    return DCNR_OK;
  }
  dcnr_status init(hipStream_t side_stream, int lag_calls) {
    side = side_stream;
    lag = lag_calls;
    DCNR_HIP(hipEventCreateWithFlags(&in_ev, SYNC_EV));
    DCNR_HIP(hipEventCreateWithFlags(&done_ev, SYNC_EV));
    for (auto& e : dw_ev) DCNR_HIP(hipEventCreateWithFlags(&e, SYNC_EV));
    return DCNR_OK;
  }
  // order the side stream after the main stream's work so far (and the main
  // stream after call (calls - lag)'s GEMM, see above)
  dcnr_status enter(hipStream_t main_s) {
    if (calls >= lag) DCNR_HIP(hipStreamWaitEvent(main_s, dw_ev[(calls - lag) % RING], 0));
    DCNR_HIP(hipEventRecord(in_ev, main_s));
    DCNR_HIP(hipStreamWaitEvent(side, in_ev, 0));
    main = main_s;
    pending = true;
    return DCNR_OK;
  }
  dcnr_status wgrad(const Layout& L, const void* dY, int64_t ldy, int N, const void* X, int64_t ldx,
                    int Kc, int64_t B, float* out, int Nr, int Kr, int accumulate, hipStream_t main_s) {
    TRY(enter(main_s));
    const int call = calls++;
    float* slab = (call & 1) ? L.slab2 : L.slab;
    DwArgs a;
    TRY(dw_args(dY, ldy, N, X, ldx, Kc, B, slab, L.slab_elems, &a));
    double rbytes = 0;
    if (pend.slab) {   // the previous call's combine, in this launch's tail
      a.rslab = pend.slab; a.rsplits = pend.S; a.rstride = pend.stride; a.rld = pend.ld;
      a.rN = pend.Nr; a.rK = pend.Kr; a.rout = pend.out;
      const int vec = pend.Kr % 4 == 0 && (uintptr_t)pend.out % 16 == 0;
      a.racc = (pend.acc ? 1 : 0) | (vec << 1);
      rbytes = 4.0 * pend.S * pend.stride + 4.0 * pend.Nr * pend.Kr * (pend.acc ? 2 : 1);
      if (pend.ld % 4 || pend.stride % 4 || (uintptr_t)pend.slab % 16) {
        set_error("wgrad: slab not 16-B aligned");
        return DCNR_UNSUPPORTED_SHAPE;
      }
    }
    TRYB(DCNR_K_GEMM_DW, side, 2.0 * B * (N + Kc) + 4.0 * Nr * Kr * (accumulate ? 2 : 1) + rbytes,
         gemm_dw(a, side));
    DCNR_HIP(hipEventRecord(dw_ev[call % RING], side));
    pend = Combine{slab, a.splits, (int64_t)N * Kc, N, Nr, Kr, out, accumulate};
    return DCNR_OK;
  }
  dcnr_status join(hipStream_t main_s) {
    if (!pending) return DCNR_OK;
    TRY(flush());
    DCNR_HIP(hipEventRecord(done_ev, side));
    DCNR_HIP(hipStreamWaitEvent(main_s, done_ev, 0));
    pending = false;
    return DCNR_OK;
  }
  ~DwPipe() {
    if (pend.slab && side) (void)flush();   // error path: the last combine too
    if (pending && main) {   // error path: order the side work before the caller's stream
      (void)hipEventRecord(done_ev, side);
      (void)hipStreamWaitEvent(main, done_ev, 0);
    }
    for (auto e : {in_ev, done_ev})
      if (e) (void)hipEventDestroy(e);
    for (auto e : dw_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

dcnr_status linear_dw(const Dims& d, const Layout& L, const void* dY, int ldy, int N,
                      const void* X, int ldx, int Kc, int64_t B, float* out, int Nr, int Kr,
                      int accumulate, hipStream_t s, DwPipe* pipe = nullptr) {
  if (d.prec == DCNR_PREC_BF16 && gemm_dw_supported(N, Kc, ldy, ldx, B)) {
    if (pipe) return pipe->wgrad(L, dY, ldy, N, X, ldx, Kc, B, out, Nr, Kr, accumulate, s);
    return wgrad_bf16(dY, ldy, N, X, ldx, Kc, B, L.slab, L.slab_elems, out, Nr, Kr, accumulate, s);
  }
  // the generic path below writes the slab on this stream: the side stream's
  // split-K reduces of earlier calls may still be reading it
  if (pipe) TRY(pipe->join(s));
  int64_t tiles = cdiv(N, 128) * cdiv(Kc, 128);
  int64_t S = std::max<int64_t>(1, std::min<int64_t>(512 / tiles, cdiv(B, 256)));
  int64_t kps = rup(cdiv(B, S), 64);
  S = cdiv(B, kps);
  if (S * (int64_t)N * Kc > L.slab_elems) {
    S = std::max<int64_t>(1, L.slab_elems / ((int64_t)N * Kc));
    kps = rup(cdiv(B, S), 64);
    S = cdiv(B, kps);
  }
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = dY; g.lda = ldy; g.B = X; g.ldb = ldx;
  g.C = L.slab; g.ldc = Kc;
  g.M = N; g.N = Kc; g.K = B; g.k_per_split = kps; g.slab_stride = (int64_t)N * Kc;
  TRYB(DCNR_K_GEMM_DW, s, (double)d.es * B * (N + Kc) + 4.0 * Nr * Kr, gemm(d.prec, true, true, EPI_SPLITK, g, (int)S, s));
  TRYB(DCNR_K_REDUCE, s, 4.0 * S * N * Kc + 4.0 * Nr * Kr * (accumulate ? 2 : 1),
       splitk_reduce(L.slab, (int)S, (int64_t)N * Kc, Kc, Nr, Kr, out, accumulate, s));
  return DCNR_OK;
}

dcnr_status hook(const dcnr_model_desc* desc, const Dims& d, const Layout& L, hipStream_t s) {
  if (!desc->bn_allreduce) return DCNR_OK;
  int rc = desc->bn_allreduce(desc->bn_allreduce_ctx, L.sums, 3 * (int64_t)d.Hp + 1, (void*)s);
  if (rc != 0) {
    set_error("bn_allreduce hook failed (%d)", rc);
    return DCNR_HIP_ERROR;
  }
  return DCNR_OK;
}

RedFinal red_init(const Layout& L, int mode, double count, int accumulate) {
  RedFinal rf;
  memset(&rf, 0, sizeof(rf));
  rf.mode = mode; rf.count = count; rf.accumulate = accumulate;
  rf.red2 = L.red2; rf.counter = L.red_cnt; rf.sums = L.sums;
  return rf;
}

RedFinal bn_bwd_rf(const Layout& L, int64_t B, const float* gamma, const float* invstd,
                   float* dgamma, float* dbeta, float* dwf, float* dbias_pre, int accumulate) {
  RedFinal rf = red_init(L, RED_BN_BWD, (double)B, accumulate);
  rf.gamma = gamma; rf.invstd = invstd; rf.dgamma = dgamma; rf.dbeta = dbeta; rf.dwf = dwf;
  rf.coef = L.coef;
  rf.dbias_pre = dbias_pre;
  return rf;
}

// nc_pre > 0: the partials of t are already in L.part (from the GEMM epilogue),
// shifted by shiftf (the Linear bias); otherwise a stats pass over t makes them.
dcnr_status bn_layer_fwd(const dcnr_model_desc* desc, const Dims& d, const Layout& L,
                         const void* t, int64_t B, bool train, const float* gamma,
                         const float* beta, float* rm, float* rv, int64_t* nbt,
                         const BnBufs& bb, hipStream_t s, int nc_pre = 0,
                         const float* shiftf = nullptr) {
  BnFinal f{gamma, beta, rm, rv, nbt, bb.scale, bb.shift, bb.mean, bb.invstd};
  if (train) {
    int nc = nc_pre;
    const void* shift = nc_pre ? nullptr : t;
    if (!nc_pre) TRYB(DCNR_K_ROWWISE, s, act_b(d, B), col_stats(d.prec, t, B, d.Hp, d.Hp, L.part, &nc, s));
    if (!desc->bn_allreduce) {  // local BN: reduce + finalize in one launch
      RedFinal rf = red_init(L, RED_BN_FWD, (double)B, 0);
      rf.f = f;
      rf.shiftf = shiftf;
      TRYP(DCNR_K_REDUCE, s, reduce_fused(d.prec, L.part, nc, 2, d.Hp, d.H, shift, rf, s));
      return DCNR_OK;
    }
    RedFinal rf = red_init(L, RED_SUMS, (double)B, 0);
    rf.shiftf = shiftf;
    TRYP(DCNR_K_REDUCE, s, reduce_fused(d.prec, L.part, nc, 2, d.Hp, d.H, shift, rf, s));
    TRY(hook(desc, d, L, s));
  }
  TRYP(DCNR_K_REDUCE, s, bn_finalize2(L.sums, d.Hp, d.H, train ? 1 : 0, f, s));
  return DCNR_OK;
}

// BN backward reductions: part [nc][NK][Hp] -> dgamma, dbeta (+ dW_f deep half
// when dwf != null) and coef.  Fused into one launch unless SyncBN must sum
// the statistics across ranks first.
dcnr_status bn_bwd_reduce(const dcnr_model_desc* desc, const Dims& d, const Layout& L, int nc,
                          int NK, int64_t B, const float* gamma, const float* invstd,
                          float* dgamma, float* dbeta, float* dwf, float* dbias_pre,
                          int accumulate, hipStream_t s) {
  const int Hp = d.Hp, H = d.H;
  if (!desc->bn_allreduce) {
    RedFinal rf = bn_bwd_rf(L, B, gamma, invstd, dgamma, dbeta, dwf, dbias_pre, accumulate);
    TRYP(DCNR_K_REDUCE, s, reduce_fused(DCNR_PREC_FP32, L.part, nc, NK, Hp, H, nullptr, rf, s));
    return DCNR_OK;
  }
  RedFinal rf = red_init(L, RED_SUMS, (double)B, 0);
  TRYP(DCNR_K_REDUCE, s, reduce_fused(DCNR_PREC_FP32, L.part, nc, NK, Hp, H, nullptr, rf, s));
  if (dwf) TRYP(DCNR_K_REDUCE, s, sums_to_grad(L.sums + 2 * Hp, H, dwf, accumulate, s));
  TRYP(DCNR_K_REDUCE, s, sums_to_grad(L.sums + Hp, H, dgamma, accumulate, s));
  TRYP(DCNR_K_REDUCE, s, sums_to_grad(L.sums, H, dbeta, accumulate, s));
  TRY(hook(desc, d, L, s));
  TRYP(DCNR_K_REDUCE, s, bn_bwd_coef(L.sums, Hp, H, gamma, invstd, L.coef, 1, s));
  if (!accumulate) TRYP(DCNR_K_PACK, s, fill_zero(dbias_pre, (size_t)H * 4, s));   // exactly 0 (see finalize)
  return DCNR_OK;
}

// Bias gradient: part [nc][NK][Hp], component 0 -> grad[H] (never needs the hook).
dcnr_status bias_reduce(const Dims& d, const Layout& L, int nc, float* grad, int accumulate,
                        hipStream_t s, int NK = 1) {
  RedFinal rf = red_init(L, RED_BIAS, 0.0, accumulate);
  rf.grad = grad;
  TRYP(DCNR_K_REDUCE, s, reduce_fused(DCNR_PREC_FP32, L.part, nc, NK, d.Hp, d.H, nullptr, rf, s));
  return DCNR_OK;
}

// C = X Wt^T [+ R] for the backward's plain dX GEMMs (all [B][Hp], square Hp)
dcnr_status linear_dx(const Dims& d, const void* X, const void* Wt, const void* R, void* C, int64_t B,
                      hipStream_t s) {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = X; g.lda = d.Hp; g.B = Wt; g.ldb = d.Hp; g.C = C; g.ldc = d.Hp;
  g.resid = R; g.ldr = R ? d.Hp : 0;
  g.M = B; g.N = d.Hp; g.K = d.Hp; g.k_per_split = d.Hp;
  TRYB(DCNR_K_GEMM_DX, s, (R ? 3 : 2) * act_b(d, B) + w_b(d, d.Hp),
       gemm_nn(d.prec, R ? EPI_STORE_RESID : EPI_STORE, g, 1, s));
  return DCNR_OK;
}

// ------------------------------------------------------------- forward
// One forward call's operands, and the tails the plan chooses between.
struct Fwd {
  const dcnr_model_desc* desc; const Dims& d; const Plan& pl; const Layout& L; const Params& P;
  const int64_t *user_ids, *item_ids, *cat_features; const float* num_features;
  int64_t B; float* logits; hipStream_t s; int check;   // check: DCNR_FLAG_CHECK_INDICES
  GatherDesc g; CrossParams cp;
  // Plan::head_stats (dcnr_forward_bce): the loss's operands
  const float* labels = nullptr; float grad_scale = 1.f; float* dz = nullptr;

  // eval, Plan::tower: gather + cross (x0 bf16, zc) -> the fused deep tower + head
  dcnr_status tower() const {
    TowerPack tp;
    memset(&tp, 0, sizeof(tp));
    tp.W0 = P.W0; tp.D = d.D; tp.b0 = P.b0;
    for (int j = 0; j < d.R; ++j) {
      const auto& Bk = P.blk[j];
      tp.w1[j] = Bk.w1; tp.b1[j] = Bk.b1; tp.g1[j] = Bk.g1; tp.be1[j] = Bk.be1; tp.rm1[j] = Bk.rm1; tp.rv1[j] = Bk.rv1;
      tp.w2[j] = Bk.w2; tp.b2[j] = Bk.b2; tp.g2[j] = Bk.g2; tp.be2[j] = Bk.be2; tp.rm2[j] = Bk.rm2; tp.rv2[j] = Bk.rv2;
    }
    tp.wf = P.wf; tp.H = d.H; tp.R = d.R; tp.out = L.twp; tp.err = check ? L.err : nullptr;
    TRYP(DCNR_K_PACK, s, tower_pack(tp, s));
    const GcOut o{nullptr, L.x0, L.zc, 0, d.Dp, nullptr};
    TRYB(DCNR_K_GATHER_CROSS, s, (double)B * (gather_row_b(d, desc->n_num) + (double)d.Dp * d.es + 4.0),
         gather_cross_out(g, cp, user_ids, item_ids, cat_features, num_features, B, o, 1, L.err, check, s));
    TowerArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.x0 = (const bf16*)L.x0; ta.ldx = d.Dp; ta.M = B; ta.Dp = d.Dp; ta.H = d.H; ta.R = d.R;
    ta.wp = L.twp; ta.zc = L.zc; ta.bias = P.bf; ta.logits = logits; ta.err = L.err;
    ta.err_mirror = check ? desc->error_mirror : nullptr;   // (the tower stores the mirror itself)
    // algorithmic bytes: the x0 rows + zc in, the logits out (the packed
    // weights are L2-resident: every CU streams the same 4.7 MB)
    TRYB(DCNR_K_TOWER, s, (double)B * (d.Dp * d.es + 8.0), eval_tower(ta, s));
    return DCNR_OK;
  }

  // The two layer-wise paths' front: weight pack, gather + cross, initial Linear.
  // Train: the weight packing (bf16 copies + transposes of the deep tower's
  // weights) is not read by the gather/cross kernel, so it runs on the side
  // stream under it and the first GEMM waits for it alone (same box, two
  // runs each: 4.033 / 4.045 vs 4.071 / 4.055 ms/step; eval keeps it on the
  // stream: its fork/join cost ~1 % of the eval forward). The embedding
  // backward's id sort needs the ids alone, so it follows there, under this
  // forward (dcnr_forward joins `sj` after the tail, so the caller's id
  // tensors are free to go once the forward's work is done).
  dcnr_status front(SideJoin& sj) const {
    const bool train = pl.train;
    if (train) {
      TRY(sj.fork(s));
      TRY(pack_all(d, P, L, train, sj.side));
      TRY(sj.mark());
    } else {
      TRY(pack_all(d, P, L, train, s, check != 0));
    }
    // (train: the pack runs on the side stream beside the gather, so the
    // error word is zeroed here, before it)
    if (check && train) TRYP(DCNR_K_PACK, s, fill_zero(L.err, 4, s));
    if (train) {
      EmbBwdDesc eb;
      memset(&eb, 0, sizeof(eb));
      eb.n_tab = g.n_tab;
      for (int t = 0; t < g.n_tab; ++t) { eb.rows[t] = g.rows[t]; eb.width[t] = g.width[t]; }
      TRYB(DCNR_K_EMB_SORT, sj.side, 2.0 * 8.0 * g.n_tab * B + 8.0 * B * (2 + d.K) + 4.0 * B * 2,
           emb_sort(eb, user_ids, item_ids, cat_features, B, L.emb, sj.side));
      TRY(sj.record());
    }
    const GcOut o{nullptr, L.x0, L.zc, 0, d.Dp, train ? L.sc : nullptr};
    TRYB(DCNR_K_GATHER_CROSS, s, (double)B * (gather_row_b(d, desc->n_num) + (double)d.Dp * d.es + 4.0),
         gather_cross_out(g, cp, user_ids, item_ids, cat_features, num_features, B, o,
                          d.prec == DCNR_PREC_BF16, L.err, check, s));
    if (train) TRY(sj.wait_mark(s));   // packed weights, biases, zeroed reduction counters
    TRYB(DCNR_K_GEMM_FWD, s, (double)B * d.Dp * d.es + act_b(d, B) + w_b(d, d.Dp),
         linear_fwd(d, L.x0, d.Dp, L.W0p, d.Dp, L.b0p, L.h[0], B, s));
    return DCNR_OK;
  }

  // eval, Plan::eval_epi: BatchNorm (running statistics) + ReLU (+ residual) in
  // the GEMM epilogues.  eval_headp: each GEMM makes its layer's running-stat
  // affine itself and the last block's GEMM ends in the deep head dot (no h_R),
  // summed with zc + bf; else every layer's affine in one launch first
  dcnr_status eval_epi() const {
    const bool hp = pl.eval_headp;
    if (!hp) {
      BnEvalBatch eb;
      memset(&eb, 0, sizeof(eb));
      eb.n = 2 * d.R; eb.N = d.Hp; eb.Nr = d.H;
      for (int j = 0; j < d.R; ++j) {
        const auto& Bk = P.blk[j];
        const BnBufs& b1 = L.bn[2 * j];
        const BnBufs& b2 = L.bn[2 * j + 1];
        eb.f[2 * j] = BnFinal{Bk.g1, Bk.be1, Bk.rm1, Bk.rv1, Bk.nbt1, b1.scale, b1.shift, b1.mean, b1.invstd};
        eb.f[2 * j + 1] = BnFinal{Bk.g2, Bk.be2, Bk.rm2, Bk.rv2, Bk.nbt2, b2.scale, b2.shift, b2.mean, b2.invstd};
      }
      TRYP(DCNR_K_REDUCE, s, bn_eval_finalize(eb, s));
    }
    const int np = gemm_ws_head_parts(d.Hp);
    for (int j = 0; j < d.R; ++j) {
      const auto& Bk = P.blk[j];
      const float* rs1[4] = {Bk.g1, Bk.be1, Bk.rm1, Bk.rv1};
      const float* rs2[4] = {Bk.g2, Bk.be2, Bk.rm2, Bk.rv2};
      const bool last = hp && j == d.R - 1;
      TRYB(DCNR_K_GEMM_FWD, s, 2 * act_b(d, B) + w_b(d, d.Hp),
           linear_bn_relu(d, L.h[j], L.W1p[j], L.b1p[j], L.bn[2 * j], nullptr, L.a1, B, s, hp ? rs1 : nullptr));
      TRYB(DCNR_K_GEMM_FWD, s, (last ? 2 * act_b(d, B) + 4.0 * B * np : 3 * act_b(d, B)) + w_b(d, d.Hp),
           linear_bn_relu(d, L.a1, L.W2p[j], L.b2p[j], L.bn[2 * j + 1], L.h[j], last ? nullptr : L.h[j + 1],
                          B, s, hp ? rs2 : nullptr, last ? P.wf : nullptr, last ? L.headp : nullptr));
    }
    if (!hp) return unfused_head();
    TRYB(DCNR_K_HEAD, s, (4.0 * np + 8.0) * B, head_parts(L.headp, np, L.zc, P.bf, B, logits, s));
    return DCNR_OK;
  }

  dcnr_status unfused_head() const {
    TRYB(DCNR_K_HEAD, s, act_b(d, B) + 4.0 * B, row_dot(d.prec, L.h[d.R], d.Hp, d.H, P.wf, B, L.zdeep, s));
    TRYB(DCNR_K_HEAD, s, 12.0 * B, head_logits(L.zdeep, L.zc, P.bf, B, logits, s));
    return DCNR_OK;
  }

  // t = A W^T + b and the BatchNorm of t (Plan::stats_epi: its column
  // partials from the GEMM's epilogue, else from a pass over t)
  dcnr_status linear_bn(const void* A, const void* W, const float* bias, void* t, const float* gamma,
                        const float* beta, float* rm, float* rv, int64_t* nbt, const BnBufs& bn) const {
    int nc = 0;
    if (pl.stats_epi)
      TRYB(DCNR_K_GEMM_FWD, s, 2 * act_b(d, B) + w_b(d, d.Hp),
           linear_fwd_stats(d, L, A, d.Hp, W, d.Hp, bias, t, B, &nc, s));
    else
      TRYB(DCNR_K_GEMM_FWD, s, 2 * act_b(d, B) + w_b(d, d.Hp), linear_fwd(d, A, d.Hp, W, d.Hp, bias, t, B, s));
    return bn_layer_fwd(desc, d, L, t, B, pl.train, gamma, beta, rm, rv, nbt, bn, s, nc,
                        pl.stats_epi ? bias : nullptr);
  }

  // train, and eval without the epilogues: layer by layer
  dcnr_status layers(uint64_t dropout_seed) const {
    const bool train = pl.train;
    const float p = train ? d.dropout : 0.f;
    for (int j = 0; j < d.R; ++j) {
      const auto& Bk = P.blk[j];
      const BnBufs& bn1 = L.bn[2 * j];
      const BnBufs& bn2 = L.bn[2 * j + 1];
      TRY(linear_bn(L.h[j], L.W1p[j], L.b1p[j], L.t1[j], Bk.g1, Bk.be1, Bk.rm1, Bk.rv1, Bk.nbt1, bn1));
      void* a1 = train ? L.a1s[j] : L.a1;
      TRYB(DCNR_K_ROWWISE, s, 2 * act_b(d, B) + (train ? mask_b(d, B) : 0),
           bn_relu_drop(d.prec, L.t1[j], a1, B, d.Hp, d.Hp, bn1.scale, bn1.shift, p, dropout_seed, j, s,
                        L.mask_a1[j]));
      TRY(linear_bn(a1, L.W2p[j], L.b2p[j], L.t2[j], Bk.g2, Bk.be2, Bk.rm2, Bk.rv2, Bk.nbt2, bn2));
      if (j == d.R - 1 && pl.head_stats) {
        // ... and on to dz and the BN2-backward partials of this block, for
        // the dcnr_backward that follows on this workspace
        int nc = 0;
        TRYB(DCNR_K_ROWWISE, s, (pl.r1_resid ? 2 : 3) * act_b(d, B) + mask_b(d, B) + 20.0 * B,
             bn_add_relu_head_stats(L.t2[j], L.h[j], B, d.Hp, d.Hp, bn2.scale, bn2.shift, bn2.mean, bn2.invstd,
                                    P.wf, d.H, L.zc, P.bf, labels, grad_scale, logits, dz, L.mask_h[d.R],
                                    pl.r1_resid ? nullptr : L.duk[j], L.part, &nc, s));
      } else if (j == d.R - 1 && pl.head_fused) {
        // last block: residual + ReLU + deep head dot + logits in one pass
        const bool store_hR = !pl.rebuild_hR || pl.keep;
        TRYB(DCNR_K_ROWWISE, s, (store_hR ? 3 : 2) * act_b(d, B) + 12.0 * B,
             bn_add_relu_head(d.prec, L.t2[j], L.h[j], store_hR ? L.h[j + 1] : nullptr, B, d.Hp, d.Hp,
                              bn2.scale, bn2.shift, P.wf, d.H, L.zc, P.bf, logits, s, L.mask_h[d.R]));
      } else {
        const bool bits = train && j + 1 < d.R;
        TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B) + (bits ? mask_b(d, B) : 0),
             bn_add_relu2(d.prec, L.t2[j], L.h[j], L.h[j + 1], B, d.Hp, d.Hp, bn2.scale, bn2.shift, s,
                          bits ? L.mask_h[j + 1] : nullptr));
      }
    }
    return pl.head_fused ? DCNR_OK : unfused_head();
  }
};

// ------------------------------------------------------------ backward
// One backward call's operands, what one residual block hands to the next
// (the blocks run last to first), and a block's backward on either path.
struct Bwd {
  const dcnr_model_desc* desc; const Dims& d; const Plan& pl; const Layout& L;
  const Params& P; const Grads& Gr;
  int64_t B; const float* dz; uint64_t dropout_seed; int accumulate; hipStream_t s; DwPipe* pipe;
  const void* Gin = nullptr;   // gradient wrt the current block's output (null: rank-1 dz * wf)
  int nc_du = 0;               // > 0: this block's du and its BN2 partials were made by the previous dX GEMM
  bool b0_done = false;        // the initial layer's bias gradient came with G (NT_EPI_RESID_SUM)

  // dW2 = dt2^T a1 and dW1 = dt1^T h_j, enqueued where they are called
  dcnr_status dw2(int j) const {
    return linear_dw(d, L, L.dt2k[j], d.Hp, d.Hp, L.a1s[j], d.Hp, d.Hp, B, Gr.blk[j].w2, d.H, d.H, accumulate, s, pipe);
  }
  dcnr_status dw1(int j) const {
    return linear_dw(d, L, L.dt1k[j], d.Hp, d.Hp, L.h[j], d.Hp, d.Hp, B, Gr.blk[j].w1, d.H, d.H, accumulate, s, pipe);
  }
  // the BN backward's reductions: dgamma, dbeta (+ dW_f[:H]) and the apply pass's coefficients
  dcnr_status bn2_reduce(int j, int nc, int NK, float* dwf) const {
    return bn_bwd_reduce(desc, d, L, nc, NK, B, P.blk[j].g2, L.bn[2 * j + 1].invstd, Gr.blk[j].g2,
                         Gr.blk[j].be2, dwf, Gr.blk[j].b2, accumulate, s);
  }
  dcnr_status bn1_reduce(int j, int nc) const {
    return bn_bwd_reduce(desc, d, L, nc, 2, B, P.blk[j].g1, L.bn[2 * j].invstd, Gr.blk[j].g1, Gr.blk[j].be1,
                         nullptr, Gr.blk[j].b1, accumulate, s);
  }

  // out = relu(BN2(t2) + h_j): du = g * [out > 0], then the BN2 apply that
  // makes dt2 unless `fold` leaves it to the dX GEMM (last block with
  // Plan::rank1: from the head pass's [h_R > 0] bits instead of du)
  dcnr_status bn2_backward(int j, bool fold) {
    const BnBufs& bn2 = L.bn[2 * j + 1];
    const bool last = !Gin && j == d.R - 1;
    int nc = 0;
    if (nc_du) {   // du and its partials came with the previous block's dX GEMM
      TRY(bn2_reduce(j, nc_du, 2, nullptr));
    } else if (last && pl.head_stats) {   // ... with the forward's head pass (dcnr_forward_bce)
      TRY(bn2_reduce(j, bn2_stats_chunks(B), 3, Gr.wf));
    } else {
      TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B) + (Gin ? act_b(d, B) : 4.0 * B),
           bwd_bn2_stats3(d.prec, Gin, dz, P.wf, L.h[j + 1], L.t2[j], bn2.mean, bn2.invstd, B, d.Hp, d.Hp,
                          L.duk[j], L.part, &nc, s, last && pl.rebuild_hR ? L.h[j] : nullptr, bn2.scale,
                          bn2.shift));
      // dbeta2, dgamma2 and (last block only) dW_f[:H]
      TRY(bn2_reduce(j, nc, 3, Gin ? nullptr : Gr.wf));
    }
    if (last && pl.rank1)
      TRYB(DCNR_K_ROWWISE, s, 2 * act_b(d, B) + mask_b(d, B) + 4.0 * B,
           bwd_bn2_apply_rank1(L.mask_h[d.R], dz, P.wf, L.t2[j], bn2.mean, bn2.invstd, L.coef, B, d.Hp, d.Hp,
                               L.dt2k[j], s));
    else if (!fold)
      TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B),
           bwd_bn2_apply2(d.prec, L.duk[j], L.t2[j], bn2.mean, bn2.invstd, L.coef, B, d.Hp, d.Hp, L.dt2k[j],
                          L.part, &nc, s));
    return DCNR_OK;
  }

  // One block with plain GEMMs and row passes (fp32, or bf16 where the GEMM
  // epilogues do not apply), in launch order.
  dcnr_status block_plain(int j) {
    const BnBufs& bn1 = L.bn[2 * j];
    void *da = L.dak[j], *dt1 = L.dt1k[j];
    int nc = 0;
    TRY(bn2_backward(j, false));
    // ---- layer2: dW2 = dt2^T a1 ; da = dt2 W2
    TRY(dw2(j));
    TRY(linear_dx(d, L.dt2k[j], L.W2t[j], nullptr, da, B, s));
    // ---- relu/dropout + BN1 backward
    TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B),
         bwd_bn1_stats(d.prec, da, L.t1[j], bn1.scale, bn1.shift, bn1.mean, bn1.invstd, B, d.Hp, d.Hp,
                       d.dropout, dropout_seed, j, L.part, &nc, s));
    TRY(bn1_reduce(j, nc));
    TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B),
         bwd_bn1_apply2(d.prec, da, L.t1[j], bn1.mean, bn1.invstd, L.coef, B, d.Hp, d.Hp, dt1, L.part, &nc, s));
    // ---- layer1: dW1 = dt1^T h_j ; G = dt1 W1 + du
    TRY(dw1(j));
    TRY(linear_dx(d, dt1, L.W1t[j], L.duk[j], L.G, B, s));
    Gin = L.G;
    return DCNR_OK;
  }

  // One block through the dX GEMM epilogues (keep masks instead of
  // activations, BN partials from the GEMMs), in launch order.  xbn: the BN
  // backward's row passes are folded into those GEMMs as well -- a GEMM then
  // takes du / da and makes dt2 / dt1 itself, and the weight gradient that
  // reads that dt follows the GEMM instead of preceding it.
  dcnr_status block_epi(int j, bool xbn) {
    const BnBufs& bn1 = L.bn[2 * j];
    const BnBufs& bn2 = L.bn[2 * j + 1];
    void *du = L.duk[j], *dt2 = L.dt2k[j], *da = L.dak[j], *dt1 = L.dt1k[j];
    int nc = 0;
    const bool xbn2 = xbn && !(j == d.R - 1 && pl.rank1);   // the BN2 apply folded into the DROP_BN GEMM
    TRY(bn2_backward(j, xbn2));
    // ---- layer2: dW2 = dt2^T a1 ; dy1 = (dt2 W2) * [a1 != 0] / (1-p): relu and
    // dropout masks from the saved activation's bits, BN1 partials in the same pass
    if (!xbn2) TRY(dw2(j));
    const XbnOperand xo2{L.t2[j], &bn2, dt2};
    TRYB(DCNR_K_GEMM_DX, s, (xbn2 ? 5 : 3) * act_b(d, B) + mask_b(d, B) + w_b(d, d.Hp),
         linear_dx_bn(d, L, NT_EPI_DROP_BN, xbn2 ? du : dt2, L.W2t[j], nullptr, da, L.mask_a1[j],
                      d.dropout > 0.f ? 1.f / (1.f - d.dropout) : 1.f, L.t1[j], bn1, B, &nc, s,
                      xbn2 ? &xo2 : nullptr));
    if (xbn2) TRY(dw2(j));
    TRY(bn1_reduce(j, nc));   // ---- BN1 backward
    if (!xbn) {
      TRYB(DCNR_K_ROWWISE, s, 3 * act_b(d, B),
           bwd_bn1_apply2(d.prec, da, L.t1[j], bn1.mean, bn1.invstd, L.coef, B, d.Hp, d.Hp, dt1, L.part, &nc, s));
      TRY(dw1(j));
    }
    // ---- layer1: dW1 = dt1^T h_j ; G = dt1 W1 + du
    const XbnOperand xo1{L.t1[j], &bn1, dt1};
    if (j > 0) {
      // G is only consumed by block j-1's BN2 backward: emit its du = G * [h_j > 0]
      // (in place over this block's du, the residual operand, unless
      // KEEP_INTERMEDIATES) and the partials
      // (the last block's du with Plan::r1_resid: rank 1, rebuilt in the epilogue, never stored)
      const bool r1 = pl.r1_resid && j == d.R - 1;
      const Rank1Resid rr{dz, P.wf, L.mask_h[d.R]};
      TRYB(DCNR_K_GEMM_DX, s, (xbn ? 6 : 4) * act_b(d, B) - (r1 ? act_b(d, B) - 4.0 * B : 0) +
                                  (r1 ? 2 : 1) * mask_b(d, B) + w_b(d, d.Hp),
           linear_dx_bn(d, L, NT_EPI_RESID_BN, xbn ? da : dt1, L.W1t[j], du, L.duk[j - 1], L.mask_h[j], 1.f,
                        L.t2[j - 1], L.bn[2 * (j - 1) + 1], B, &nc_du, s, xbn ? &xo1 : nullptr,
                        r1 ? &rr : nullptr));
      if (xbn) TRY(dw1(j));
      Gin = L.duk[j - 1];
      return DCNR_OK;
    }
    if (xbn) {
      // block 0: G's column sums (the initial layer's bias gradient) in the
      // epilogue, which reads no mask and no BN input
      int ncg = 0;
      TRYB(DCNR_K_GEMM_DX, s, 5 * act_b(d, B) + w_b(d, d.Hp),
           linear_dx_bn(d, L, NT_EPI_RESID_SUM, da, L.W1t[j], du, L.G, nullptr, 0.f, nullptr, BnBufs{}, B,
                        &ncg, s, &xo1));
      TRY(dw1(j));
      TRY(bias_reduce(d, L, ncg, Gr.b0, accumulate, s, 2));
      b0_done = true;
    } else {
      TRY(linear_dx(d, dt1, L.W1t[j], du, L.G, B, s));
    }
    Gin = L.G;
    nc_du = 0;
    return DCNR_OK;
  }
};

// dcnr_forward (bce null) and dcnr_forward_bce: the forward, then the loss
struct BceOut { const float* labels; float grad_scale; float* loss; float* dlogits; double* part; };

dcnr_status forward_run(const dcnr_model_desc* desc, void* const* params,
                        const int64_t* user_ids, const int64_t* item_ids,
                        const int64_t* cat_features, const float* num_features, int64_t B,
                        int mode, uint64_t dropout_seed, float* logits, void* ws,
                        size_t ws_bytes, dcnr_stream_t stream, const BceOut* bce_out) {
  Dims d;
  TRY(make_dims(desc, &d));
  hipStream_t s = (hipStream_t)stream;
  if (!params || !logits || !ws || B < 0 || (B > 0 && (!user_ids || !item_ids)) ||
      (d.K > 0 && B > 0 && !cat_features) || (desc->n_num > 0 && B > 0 && !num_features)) {
    set_error("dcnr_forward: null argument");
    return DCNR_BAD_ARG;
  }
  if (mode == DCNR_TRAIN && B < 2) {
    set_error("Expected more than 1 value per channel when training");
    return DCNR_BAD_ARG;
  }
  // the head pass's statistics need the loss's operands: dcnr_forward_bce only
  const uint32_t flags = bce_out ? desc->flags : desc->flags & ~DCNR_FLAG_HEAD_STATS;
  const Plan pl = make_plan(d, flags, mode, B, desc->bn_allreduce != nullptr);
  const Layout L = make_layout(d, B, pl, ws);
  if (ws_bytes < L.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, L.total);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  if (B == 0) return DCNR_OK;
  const Params P = map_params(d, params);
  const int check = (desc->flags & DCNR_FLAG_CHECK_INDICES) ? 1 : 0;
  Fwd f{desc, d, pl, L, P, user_ids, item_ids, cat_features, num_features, B, logits, s, check,
        make_gather(d, P, desc->n_num), make_cross(d, P)};
  if (bce_out) { f.labels = bce_out->labels; f.grad_scale = bce_out->grad_scale; f.dz = bce_out->dlogits; }
  if (pl.tower) return f.tower();
  SideJoin sj;
  TRY(f.front(sj));
  TRY(pl.eval_epi ? f.eval_epi() : f.layers(dropout_seed));
  if (pl.train) TRY(sj.join(s));   // the sorted ids (workspace) for dcnr_backward
  // the id-check word to the caller's mirror, after the forward's last kernel
  // on the stream
  if (desc->error_mirror && check) TRYP(DCNR_K_PACK, s, mirror_word((const int*)ws, desc->error_mirror, s));
  // the loss value (and dz, unless the head pass made it): the loss kernels
  // of dcnr_bce_with_logits on the logits, so its bits do not depend on the path
  if (bce_out)
    TRYP(DCNR_K_HEAD, s, bce(logits, bce_out->labels, B, bce_out->loss, pl.head_stats ? nullptr : bce_out->dlogits,
                             bce_out->grad_scale, bce_out->part, s));
  return DCNR_OK;
}


}  // namespace
}  // namespace dcnr

using namespace dcnr;

extern "C" {

int64_t dcnr_input_dim(const dcnr_model_desc* desc) {
  Dims d;
  if (make_dims(desc, &d) != DCNR_OK) return -1;
  return d.D;
}

dcnr_status dcnr_workspace_size(const dcnr_model_desc* desc, int64_t B, int mode, size_t* bytes) {
  Dims d;
  TRY(make_dims(desc, &d));
  if (!bytes || B < 0) { set_error("bad args"); return DCNR_BAD_ARG; }
  *bytes = make_layout(d, B, make_plan(d, desc->flags, mode, B), nullptr).total;
  return DCNR_OK;
}

dcnr_status dcnr_workspace_offset(const dcnr_model_desc* desc, int64_t B, int mode, int kind,
                                  int index, int64_t* offset) {
  Dims d;
  TRY(make_dims(desc, &d));
  if (!offset || B < 0 || kind < 0 || kind >= DCNR_WS_KINDS) { set_error("bad args"); return DCNR_BAD_ARG; }
  // a null base yields offsets as pointers from 0 (Bump takes nullptr -> nullptr),
  // so lay out against a fake non-null base
  char* base = (char*)(uintptr_t)4096;
  Layout L = make_layout(d, B, make_plan(d, desc->flags, mode, B), base);
  const int R = d.R;
  auto blk = [&](int n) { return index >= 0 && index < n; };
  const void* p = nullptr;
  switch (kind) {
    case DCNR_WS_X0: p = L.x0; break;
    case DCNR_WS_H: if (blk(R + 1)) p = L.h[index]; break;
    case DCNR_WS_T1: if (blk(R)) p = L.t1[index]; break;
    case DCNR_WS_T2: if (blk(R)) p = L.t2[index]; break;
    case DCNR_WS_A1: if (blk(R)) p = L.a1s[index]; break;
    case DCNR_WS_MASK_A1: if (blk(R)) p = L.mask_a1[index]; break;
    case DCNR_WS_MASK_H: if (blk(R + 1)) p = L.mask_h[index]; break;   // (j = R: Plan::rank1)
    case DCNR_WS_BN_MEAN: if (blk(2 * R)) p = L.bn[index].mean; break;
    case DCNR_WS_BN_INVSTD: if (blk(2 * R)) p = L.bn[index].invstd; break;
    case DCNR_WS_BN_SCALE: if (blk(2 * R)) p = L.bn[index].scale; break;
    case DCNR_WS_BN_SHIFT: if (blk(2 * R)) p = L.bn[index].shift; break;
    case DCNR_WS_DU: if (blk(R)) p = L.duk[index]; break;
    case DCNR_WS_DT2: if (blk(R)) p = L.dt2k[index]; break;
    case DCNR_WS_DA: if (blk(R)) p = L.dak[index]; break;
    case DCNR_WS_DT1: if (blk(R)) p = L.dt1k[index]; break;
    case DCNR_WS_G: p = L.G; break;
    case DCNR_WS_DX0: p = L.dx0; break;
    case DCNR_WS_ZC: p = L.zc; break;
    case DCNR_WS_XCOEF: p = L.xcoef; break;
    case DCNR_WS_SC: p = L.sc; break;
    case DCNR_WS_ROW_MAP: p = L.rowmap; break;
  }
  *offset = p ? (int64_t)((const char*)p - base) : -1;
  return DCNR_OK;
}

dcnr_status dcnr_gather_cross(const dcnr_model_desc* desc, void* const* params,
                              const int64_t* user_ids, const int64_t* item_ids,
                              const int64_t* cat_features, const float* num_features, int64_t B,
                              float* x0, int64_t ld_x0, float* cross_out, int64_t ld_cross,
                              int32_t* oob_flag, dcnr_stream_t stream) {
  Dims d;
  TRY(make_dims(desc, &d));
  hipStream_t s = (hipStream_t)stream;
  if (!params || B < 0 || (B > 0 && (!user_ids || !item_ids)) ||
      (d.K > 0 && B > 0 && !cat_features) || (desc->n_num > 0 && B > 0 && !num_features)) {
    set_error("dcnr_gather_cross: null argument");
    return DCNR_BAD_ARG;
  }
  if ((x0 && (ld_x0 < d.D || ld_x0 > INT32_MAX)) ||
      (cross_out && (ld_cross < d.D || ld_cross > INT32_MAX))) {
    set_error("dcnr_gather_cross: row stride below D=%d", d.D);
    return DCNR_BAD_ARG;
  }
  if (B == 0 || (!x0 && !cross_out)) return DCNR_OK;
  Params P = map_params(d, params);
  GatherDesc g = make_gather(d, P, desc->n_num);
  CrossParams cp = make_cross(d, P);
  const GcOut o{cross_out, x0, nullptr, (int)ld_cross, (int)ld_x0};
  const int check = oob_flag != nullptr;
  TRYB(DCNR_K_GATHER_CROSS, s, (double)B * (gather_row_b(d, desc->n_num) + 4.0 * d.D * ((x0 ? 1 : 0) + (cross_out ? 1 : 0))),
       gather_cross_out(g, cp, user_ids, item_ids, cat_features, num_features, B, o, 0, oob_flag, check, s));
  return DCNR_OK;
}

dcnr_status dcnr_forward(const dcnr_model_desc* desc, void* const* params,
                         const int64_t* user_ids, const int64_t* item_ids,
                         const int64_t* cat_features, const float* num_features, int64_t B,
                         int mode, uint64_t dropout_seed, float* logits, void* ws,
                         size_t ws_bytes, dcnr_stream_t stream) {
  return forward_run(desc, params, user_ids, item_ids, cat_features, num_features, B, mode, dropout_seed,
                     logits, ws, ws_bytes, stream, nullptr);
}

dcnr_status dcnr_forward_bce(const dcnr_model_desc* desc, void* const* params,
                             const int64_t* user_ids, const int64_t* item_ids,
                             const int64_t* cat_features, const float* num_features, int64_t B,
                             uint64_t dropout_seed, const float* labels, float grad_scale,
                             float* logits, float* loss, float* dlogits, void* bce_ws,
                             size_t bce_ws_bytes_, void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  if (!labels || !loss || !dlogits || !bce_ws || B < 2) {
    set_error("dcnr_forward_bce: bad argument");
    return DCNR_BAD_ARG;
  }
  if (bce_ws_bytes_ < bce_ws_bytes()) {
    set_error("dcnr_forward_bce: loss workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  const BceOut bo{labels, grad_scale, loss, dlogits, (double*)bce_ws};
  return forward_run(desc, params, user_ids, item_ids, cat_features, num_features, B, DCNR_TRAIN,
                     dropout_seed, logits, ws, ws_bytes, stream, &bo);
}

dcnr_status dcnr_backward(const dcnr_model_desc* desc, void* const* params, void* const* grads,
                          const int64_t* user_ids, const int64_t* item_ids,
                          const int64_t* cat_features, const float* num_features, int64_t B,
                          const float* dlogits, uint64_t dropout_seed, int accumulate, void* ws, size_t ws_bytes,
                          dcnr_stream_t stream) {
  Dims d;
  TRY(make_dims(desc, &d));
  hipStream_t s = (hipStream_t)stream;
  if (!params || !grads || !dlogits || !ws || B < 2) {
    set_error("dcnr_backward: bad argument");
    return DCNR_BAD_ARG;
  }
  const Plan pl = make_plan(d, desc->flags, DCNR_TRAIN, B, desc->bn_allreduce != nullptr);
  const Layout L = make_layout(d, B, pl, ws);
  if (ws_bytes < L.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, L.total);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  const Params P = map_params(d, params);
  const Grads Gr = map_grads(d, grads);
  const int Hp = d.Hp, H = d.H;
  if (pl.rowmap && accumulate) {
    set_error("dcnr_backward: DCNR_FLAG_ROW_MAP needs accumulate = 0");
    return DCNR_BAD_ARG;
  }
  // dense embedding grads: zeroed; the per-row sums (emb_segment_sum) then
  // write every row an id references.  (On the side stream under the deep
  // tower instead: 3.99-4.00 vs 3.98-3.99 ms/step, same box; kept here.)
  // DCNR_FLAG_ROW_MAP: only the row map is zeroed; the sums mark the rows
  // they write and the optimizer reads unmarked rows as 0.
  if (pl.rowmap) {
    TRYB(DCNR_K_PACK, s, (double)L.rowmap_bytes, fill_zero(L.rowmap, L.rowmap_bytes, s));
  } else if (!accumulate) {
    void* zp[2 + MAX_CAT];
    int64_t zn[2 + MAX_CAT];
    for (int t = 0; t < 2 + d.K; ++t) { zp[t] = Gr.tab[t]; zn[t] = d.rows[t] * d.widths[t] * 4; }
    double zb = 0;
    for (int t = 0; t < 2 + d.K; ++t) zb += (double)zn[t];
    TRYB(DCNR_K_PACK, s, zb, fill_zero_multi(2 + d.K, zp, zn, s));
  }

  // embedding backward, part 1 (the stable sort of the (table row, sample)
  // pairs) ran under the train forward (dcnr_forward); its result is in ws
  GatherDesc g = make_gather(d, P, desc->n_num);
  EmbBwdDesc eb;
  memset(&eb, 0, sizeof(eb));
  eb.n_tab = g.n_tab;
  eb.touched = L.rowmap;   // (null without DCNR_FLAG_ROW_MAP)
  for (int t = 0; t < g.n_tab; ++t) {
    eb.grad[t] = Gr.tab[t]; eb.rows[t] = g.rows[t]; eb.width[t] = g.width[t]; eb.off[t] = g.off[t];
  }
  // The cross backward depends on dz and the forward's outputs alone: it
  // runs on a side stream under the deep-tower backward and joins before the
  // dense-gradient hook.
  SideJoin sj;
  TRY(sj.fork(s));
  const CrossParams cpx = make_cross(d, P);
  // ---- cross network + head bias (low-rank form, from the forward's
  // per-sample scalars, dz and the stored x0 alone; cross_bwd.hip)
  CrossGrads cg;
  memset(&cg, 0, sizeof(cg));
  for (int l = 0; l < d.L; ++l) { cg.dw[l] = Gr.cw[l]; cg.db[l] = Gr.cb[l]; }
  cg.dwf_cross = Gr.wf + H;
  cg.dbf = Gr.bf;
  TRYB(DCNR_K_CROSS_BWD, sj.side, (double)B * (4.0 * (2 * d.L + 1) + 4.0 + 8.0 * (d.L + 1)) + (double)B * d.Dp * d.es,
       cross_backward(cpx, d.D, L.sc, dlogits, L.x0, d.prec == DCNR_PREC_BF16, d.Dp, B, cg, L.xcoef,
                      L.xalpha, L.cscratch, L.cscratch_bytes, accumulate, sj.side));
  TRY(sj.record());
  DwPipe dwp;
  DwPipe* pipe = nullptr;
  // (a run-time choice, not a plan field: not while kernel classes are being
  // timed, where every launch is priced alone, on the main stream -- except
  // in profile mode 2, which times the side stream's gemm_dw launches in place)
  if (d.prec == DCNR_PREC_BF16 && prof_side_stream_ok()) {
    TRY(dwp.init(sj.side, pl.dw_lag));
    pipe = &dwp;
  }

  Bwd c{desc, d, pl, L, P, Gr, B, dlogits, dropout_seed, accumulate, s, pipe};
  for (int j = d.R - 1; j >= 0; --j) TRY(pl.stats_epi ? c.block_epi(j, pl.xbn) : c.block_plain(j));
  // ---- initial layer: the weight gradient on the side stream (after block
  // 0's); the bias gradient came with G (b0_done) or is a column-sum pass
  // here on the main stream, ahead of the dx0 GEMM.  The side stream's queue
  // sets the backward's tail: with the column sums on it, the optimizer
  // waited 135 us for it while the main stream was done
  // (profiles/r06fin_step_timeline.txt)
  TRY(linear_dw(d, L, L.G, Hp, Hp, L.x0, d.Dp, d.Dp, B, Gr.W0, H, d.D, accumulate, s, pipe));
  if (!c.b0_done) {
    int nc = 0;
    TRYB(DCNR_K_ROWWISE, s, act_b(d, B), col_sum(d.prec, L.G, B, Hp, Hp, L.part, &nc, s));
    TRY(bias_reduce(d, L, nc, Gr.b0, accumulate, s));
  }
  TRY(sj.join(s));   // the side stream's cross gradients, coefficients and sorted ids
  // and the weight gradients; without a hook nothing reads them before the
  // optimizer, so they join at the end (under the dx0 GEMM and embedding sums)
  if (desc->grad_ready) TRY(dwp.join(s));
  TRY(grads_ready(desc, DCNR_GRADS_DENSE, s));   // every non-embedding gradient is enqueued
  GemmArgs gx;
  memset(&gx, 0, sizeof(gx));
  gx.A = L.G; gx.lda = Hp; gx.B = L.W0t; gx.ldb = Hp; gx.C = L.dx0; gx.ldc = dq_of(d); gx.out_f32 = 1;
  gx.M = B; gx.N = d.Dp; gx.K = Hp; gx.k_per_split = Hp;
  TRYB(DCNR_K_GEMM_DX, s, act_b(d, B) + 4.0 * B * d.Dp + w_b(d, d.Dp), gemm_nn(d.prec, EPI_STORE, gx, 1, s));
  // ---- embedding backward part 2: sorted (table row, sample) pairs -> per row
  // sum of the deep dx0 segments + sum of the cross coefficients
  double ew = 0;
  for (int t = 0; t < 2 + d.K; ++t) ew += d.widths[t];
  eb.nv = d.L + 1;
  for (int l = 0; l < d.L; ++l) eb.V[l] = cpx.w[l];
  eb.V[d.L] = cpx.wf_cross;
  TRYB(DCNR_K_EMB_SUM, s, (double)B * (4.0 * ew + (8.0 + 4.0 * (d.L + 1)) * g.n_tab),
       emb_segment_sum(eb, L.emb, B, L.dx0, dq_of(d), L.xcoef, accumulate, s));
  if (!desc->grad_ready) TRY(dwp.join(s));
  TRY(grads_ready(desc, DCNR_GRADS_EMBEDDING, s));
  return DCNR_OK;
}

size_t dcnr_bce_workspace_size(void) { return bce_ws_bytes() + 256; }

dcnr_status dcnr_emb_touched_rows(const dcnr_model_desc* desc, const void* ws, size_t ws_bytes,
                                  int64_t B, int32_t n_tables, const int32_t* tables,
                                  const int64_t* elem_off, int64_t shard_elems, int32_t world,
                                  int64_t* out_offsets, int64_t* table_counts,
                                  int64_t* owner_counts, dcnr_stream_t stream) {
  Dims d;
  TRY(make_dims(desc, &d));
  if (!ws || B < 0 || n_tables < 1 || n_tables > 2 + d.K || !tables || !elem_off ||
      !out_offsets || !table_counts || !owner_counts) {
    set_error("dcnr_emb_touched_rows: bad argument");
    return DCNR_BAD_ARG;
  }
  Layout L = make_layout(d, B, make_plan(d, desc->flags, DCNR_TRAIN, B), (void*)ws);
  if (ws_bytes < L.total) {
    set_error("workspace too small: %zu < %zu", ws_bytes, L.total);
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  TouchedArgs a;
  memset(&a, 0, sizeof(a));
  a.n = n_tables;
  a.shard = shard_elems;
  a.world = world;
  for (int i = 0; i < n_tables; ++i) {
    const int t = tables[i];
    if (t < 0 || t >= 2 + d.K) {
      set_error("dcnr_emb_touched_rows: table %d out of range", t);
      return DCNR_BAD_ARG;
    }
    if (elem_off[i] < 0) {   // (off / shard would round a negative offset into owner 0)
      set_error("dcnr_emb_touched_rows: negative elem_off");
      return DCNR_BAD_ARG;
    }
    uint32_t base = 0;
    for (int u = 0; u < t; ++u) base += (uint32_t)d.rows[u];
    a.tab[i] = t;
    a.base[i] = base;
    a.width[i] = d.widths[t];
    a.elem_off[i] = elem_off[i];
  }
  return emb_touched_rows(a, L.emb, B, out_offsets, table_counts, owner_counts,
                          (hipStream_t)stream);
}

dcnr_status dcnr_bce_with_logits(const float* logits, const float* labels, int64_t B, float* loss,
                                 float* dlogits, float grad_scale, void* ws, size_t ws_bytes,
                                 dcnr_stream_t stream) {
  if (!logits || !labels || !loss || !ws || B < 1) {
    set_error("dcnr_bce_with_logits: bad argument");
    return DCNR_BAD_ARG;
  }
  if (ws_bytes < bce_ws_bytes()) {
    set_error("dcnr_bce_with_logits: workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  hipStream_t s = (hipStream_t)stream;
  TRYP(DCNR_K_HEAD, s, bce(logits, labels, B, loss, dlogits, grad_scale, (double*)ws, s));
  return DCNR_OK;
}

dcnr_status dcnr_linear_bf16(const void* X, int64_t ldx, int64_t M, int32_t K, const void* W,
                             int64_t ldw, int32_t N, const float* bias, void* C, int64_t ldc,
                             int out_f32, dcnr_stream_t stream) {
  if (!X || !W || !C || M < 0 || K < 1 || N < 1) {
    set_error("dcnr_linear_bf16: bad argument");
    return DCNR_BAD_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.A = X; g.lda = ldx; g.B = W; g.ldb = ldw; g.C = C; g.ldc = ldc; g.bias = bias;
  g.M = M; g.N = N; g.K = K; g.k_per_split = K; g.out_f32 = out_f32 ? 1 : 0;
  TRYP(DCNR_K_GEMM_FWD, s, gemm_nn(DCNR_PREC_BF16, EPI_STORE, g, 1, s));
  return DCNR_OK;
}

size_t dcnr_linear_wgrad_workspace_size(int32_t N, int32_t K, int64_t B) {
  if (N < 1 || K < 1 || B < 1) return 0;   // (dcnr_linear_wgrad_bf16 rejects these shapes)
  return (size_t)gemm_dw_splits(N, K, B) * (size_t)N * (size_t)K * sizeof(float);
}

dcnr_status dcnr_linear_wgrad_bf16(const void* dY, int64_t ldy, const void* X, int64_t ldx,
                                   int64_t B, int32_t N, int32_t K, float* dW, int accumulate,
                                   void* ws, size_t ws_bytes, dcnr_stream_t stream) {
  if (!dY || !X || !dW || !ws || B < 1 || N < 1 || K < 1 || !gemm_dw_supported(N, K, ldy, ldx, B)) {
    set_error("dcnr_linear_wgrad_bf16: bad or unsupported arguments");
    return DCNR_BAD_ARG;
  }
  if (ws_bytes < dcnr_linear_wgrad_workspace_size(N, K, B)) {
    set_error("workspace too small");
    return DCNR_WORKSPACE_TOO_SMALL;
  }
  return wgrad_bf16(dY, ldy, N, X, ldx, K, B, (float*)ws, (int64_t)(ws_bytes / 4), dW, N, K,
                    accumulate, (hipStream_t)stream);
}

}  // extern "C"
