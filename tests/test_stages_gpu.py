"""Stage-by-stage parity of the training step: bf16 (the benchmarked path) and
fp32 (the parity path).

The checker is tests/stage_check.py: every tensor a kept-intermediates step
stores is recomputed in torch fp32/fp64 from the kernels' own stored inputs of
that stage and compared (stages, reference lines and tolerances are listed
there).  test_bf16_step_stage_by_stage runs it at the benchmark's shapes,
test_bf16_step_stage_by_stage_paths at small shapes that take every other
kernel path, test_fp32_step_stage_by_stage_paths at the fp32 step's shapes
(fp64 references, one fp32 ulp + 2^-18 x the summed |terms|), and
test_step_stage_by_stage_batch_regimes, in both precisions, at narrow models
whose batch size alone takes the reductions and the fp32 split-K past what
B <= 8192 reaches, and past 262144 / 524288 rows, where the deep tower's GEMMs
run as several launches of 32-bit buffer offsets, and
test_step_stage_by_stage_limits at the limits of the shapes the library
accepts (cross layers, blocks, tables, input and hidden width).  Every small
case then runs the same step again in the layout a real step uses.
"""
import time

import pytest
import torch

import golden_common as gc
from stage_check import ACC_EPS, BF16_ULPS, FLIP_FRAC, REL, expected_plan, stage_check  # noqa: F401

pytestmark = pytest.mark.gpu


def _cfg(full):
    if full == "h384":   # K = 384 < 512: the fused BN-backward operand's partial last chunks
        return dict(n_users=50_000, n_items=5_000, cat_dims={f"c{k}": 100 for k in range(4)},
                    n_num=8, params=dict(emb_dim=32, hidden_dim=384, n_cross_layers=2,
                                         n_res_blocks=3, dropout=0.6)), 8192
    if full:
        return dict(n_users=1_000_000, n_items=100_000, cat_dims={f"c{k}": 1000 for k in range(12)},
                    n_num=8, params=dict(emb_dim=32, hidden_dim=512, n_cross_layers=3,
                                         n_res_blocks=4, dropout=0.6)), 131072
    return dict(gc.CFG3R, params=dict(gc.CFG3R["params"], dropout=0.6)), 1024


@pytest.mark.parametrize("full", [False, True, "h384"], ids=["cfg3r_B1024", "cfg2_B131072", "h384_B8192"])
def test_bf16_step_stage_by_stage(dev, full):
    cfg, B = _cfg(full)
    t0 = time.perf_counter()
    stage_check(dev, cfg, B, 7)
    print(f"  B = {B}: wall {time.perf_counter() - t0:.1f} s")


# golden_common.CFG3R's tables and cross network (D = 456), as tests/test_paths_gpu.py's CFG
def _tables(n_cat=12, emb=32, n_num=8, card=None):
    if card is None:
        card = 1000 if emb == 32 else 250   # embedding width int(sqrt(card)) + 1 = emb
    return dict(n_users=4096, n_items=1024, cat_dims={f"c{k}": card for k in range(n_cat)}, n_num=n_num,
                emb_dim=emb)


# id: (hidden, blocks, dropout, B, tables, seed, plan fields expected true)
# One seed serves every case: no case's flip fraction came near FLIP_FRAC with it.
PATH_CASES = {
    "h40_r1": (40, 1, 0.6, 300, _tables(), 11, ""),
    "h100_r2": (100, 2, 0.6, 300, _tables(), 11, ""),
    "h64_r2_p0": (64, 2, 0.0, 300, _tables(), 11, "masks stats_epi"),
    "h250_r2": (250, 2, 0.6, 300, _tables(), 11, "masks stats_epi"),
    "h384_r2": (384, 2, 0.6, 300, _tables(), 11, "masks stats_epi xbn"),
    "h500_r2": (500, 2, 0.6, 300, _tables(), 11, ""),
    "h512_r3": (512, 3, 0.6, 300, _tables(), 11, "masks stats_epi xbn head_fused rank1"),
    "h512_r1": (512, 1, 0.6, 300, _tables(), 11, "masks stats_epi xbn head_fused rank1"),
    "h1024_r2": (1024, 2, 0.6, 300, _tables(), 11, "masks"),
    "h64_r1_D164": (64, 1, 0.6, 300, _tables(8, 16, 4), 11, "masks stats_epi"),
    "h512_r1_D579": (512, 1, 0.6, 300, _tables(16, 32, 3), 11, "masks stats_epi xbn head_fused rank1"),
    "h384_r2_B33": (384, 2, 0.6, 33, _tables(), 11, "masks stats_epi xbn"),
    "h512_r2_B492": (512, 2, 0.6, 492, _tables(), 11, "masks stats_epi xbn head_fused rank1"),
    "h250_r2_B492": (250, 2, 0.6, 492, _tables(), 11, "masks stats_epi"),
}
INPUT_DIM = {"h64_r1_D164": 164, "h512_r1_D579": 579}


def _run_case(dev, case, precision, hidden, n_res, p, B, tb, seed, flags, input_dim, n_cross=3, bound_x=None):
    """The stage check of one case, then the same step in the production
    layout: logits, loss and every gradient bit-equal to the kept run's."""
    cfg = dict(n_users=tb["n_users"], n_items=tb["n_items"], cat_dims=tb["cat_dims"], n_num=tb["n_num"],
               params=dict(emb_dim=tb["emb_dim"], hidden_dim=hidden, n_cross_layers=n_cross,
                           n_res_blocks=n_res, dropout=p))
    assert {k for k, v in expected_plan(hidden, precision).items() if v} == set(flags.split()), "the case's path"
    t0 = time.perf_counter()
    res = stage_check(dev, cfg, B, seed, precision, bound_x)
    assert res["grads"]["initial_deep_layer.weight"].shape[1] == input_dim
    logits, loss, grads = res["plain_step"]()
    diff = [k for k, g in res["grads"].items() if not torch.equal(g, grads[k])]
    if not torch.equal(logits, res["logits"]):
        diff.append("logits")
    if not torch.equal(loss, res["loss"]):
        diff.append("loss")
    worst = max((q for q in res["rels"] if q[2] == REL), key=lambda q: q[1])
    print(f"  CASE {case}: {'flip' if precision == 'bf16' else 'diff/bound'} "
          f"{max(s[1] for s in res['stats']):.2e} diff "
          f"{max(s[2] for s in res['stats']):.2e} rel {worst[1]:.2e} ({worst[0]}) "
          f"second run {'bit-equal' if not diff else 'DIFFERS ' + str(diff)} "
          f"wall {time.perf_counter() - t0:.1f} s")
    assert not diff, diff


@pytest.mark.parametrize("case", list(PATH_CASES))
def test_bf16_step_stage_by_stage_paths(dev, case):
    """The stage checks on every kernel path of the bf16 train step, at
    B = 300 (4 full 64-row tiles + 44 rows; 9 full 32-row tiles + 12 rows), 33
    or 492, then the same step in the production layout (no keep_intermediates:
    one shared or per-block dt set, RESID_BN in place over du, dt1 over the a1
    scratch, the side stream's weight gradients with their waits), whose
    logits, loss and every gradient must be bit-equal to the kept run's: the
    same kernels see the same inputs and every reduction has a fixed order.

      case          path (make_plan, gemm_ws / gemm_wsp dispatch)
      h40_r1        no masks, block_plain, gemm_ws KTP = 4, one block
      h100_r2       Hp = 104: no masks, block_plain, padded columns
      h64_r2_p0     block_epi without the fold, KTP = 4, RESID_BN, inv_keep = 1
      h250_r2       Hp = 256: KTP = 8, masks with padded bits, bwd_bn1_apply2
      h384_r2       operand fold, N slices 256 + 128, unfused head
      h500_r2       Hp = 504: no masks, gemm_wsp forward (slices 256 + 248), block_plain
      h512_r3       fold, fused head, rank-1 BN2 apply
      h512_r1       last block = block 0: rank-1 apply and RESID_SUM together
      h1024_r2      masks stored, block_plain, generic GEMM (K > 512)
      h64_r1_D164   initial layer, dW0, dx0 at Dp = 168 (gemm_ws KTP = 8)
      h512_r1_D579  Dp = 584: initial layer on the generic GEMM, dx0 with N > 512
      h384_r2_B33   one 32-row tile + 1 row; one short 64-row tile
      h512_r2_B492  16 32-row tiles (the last one 12 rows) on the backward epilogues' 16
      h250_r2_B492  workgroup rows, 8 64-row tiles on the forward's 8: every row of the
                    column partials carries data, the last one the ragged tile's (at
                    B = 300 the last 6 / 3 rows of the partials are zeros, and a reduce
                    that drops the last row goes unnoticed)

    Measured on an MI355X (worst stage flip fraction, worst max |diff| of a
    bf16 stage, worst relative error of a gradient, second run bit-equal):

      case          flip fraction  max |diff|  gradient rel. error      second run
      h40_r1        1.67e-04       3.07e-02    3.78e-06 (cross_b[2])     bit-equal
      h100_r2       1.00e-04       3.10e-02    2.37e-07 (cross_w[0])     bit-equal
      h64_r2_p0     1.04e-04       2.43e-02    2.18e-07 (dW_f[H:])       bit-equal
      h250_r2       1.33e-04       3.10e-02    2.18e-07 (cross_w[2])     bit-equal
      h384_r2       2.00e-04       3.12e-02    2.16e-07 (db_f)           bit-equal
      h500_r2       1.93e-04       3.10e-02    3.43e-07 (cross_w[2])     bit-equal
      h512_r3       2.28e-04       3.12e-02    3.03e-07 (cross_b[2])     bit-equal
      h512_r1       2.80e-04       3.11e-02    1.73e-07 (cross_w[1])     bit-equal
      h1024_r2      3.26e-04       3.24e-02    2.05e-07 (dW_f[H:])       bit-equal
      h64_r1_D164   2.08e-04       3.10e-02    2.15e-07 (cross_w[1])     bit-equal
      h512_r1_D579  2.21e-04       3.12e-02    3.41e-07 (cross_b[1])     bit-equal
      h384_r2_B33   2.37e-04       2.89e-02    3.51e-07 (cross_w[2])     bit-equal
      h512_r2_B492  2.34e-04       3.12e-02    3.41e-07 (cross_w[2])     bit-equal
      h250_r2_B492  1.30e-04       3.11e-02    2.23e-07 (cross_w[1])     bit-equal

    (max |diff| is one bf16 ulp of a value in [4, 8); the gradient errors are fp32
    summation-order differences against fp64 sums of the same stored operands.)
    """
    _run_case(dev, case, "bf16", *PATH_CASES[case], INPUT_DIM.get(case, 456))


# id: (hidden, blocks, dropout, B, tables, seed, plan fields expected true)
F32_CASES = {
    "f32_h40_r1": (40, 1, 0.6, 300, _tables(), 11, ""),
    "f32_h100_r2": (100, 2, 0.6, 300, _tables(), 11, ""),
    "f32_h256_r2": (256, 2, 0.6, 300, _tables(), 11, "head_fused"),
    "f32_h512_r2": (512, 2, 0.6, 300, _tables(), 11, ""),
    "f32_h1024_r1": (1024, 1, 0.6, 300, _tables(), 11, ""),
    "f32_h64_r1_D164": (64, 1, 0.6, 300, _tables(8, 16, 4), 11, ""),
    "f32_h512_r1_D579": (512, 1, 0.6, 300, _tables(16, 32, 3), 11, ""),
    "f32_h100_r2_B33": (100, 2, 0.6, 33, _tables(), 11, ""),
    "f32_h64_r2_p0": (64, 2, 0.0, 300, _tables(), 11, ""),
}
F32_INPUT_DIM = {"f32_h64_r1_D164": 164, "f32_h512_r1_D579": 579}


@pytest.mark.parametrize("case", list(F32_CASES))
def test_fp32_step_stage_by_stage_paths(dev, case):
    """The stage checks on the fp32 train step (block_plain, fp32 storage,
    the generic MFMA GEMM, no masks), with fp64 references and the bound one
    fp32 ulp + 2^-18 x the summed |terms| (tests/stage_check.py), then the same
    step in the production layout, bit-equal.

      case              reaches
      f32_h40_r1        one partial 128-wide GEMM tile, one block
      f32_h100_r2       Hp = 104: padded columns in every fp32 row pass and in the reduce
      f32_h256_r2       the fp32 fused head pass (bn_add_relu_head<float>, a wave per row)
      f32_h512_r2       the benchmark width on the parity path, unfused head
      f32_h1024_r1      tcols = Hp / 4 = NT = 256: one row per pass, the fp32 row-pass limit; K > 512
      f32_h64_r1_D164   Dp = 168: initial layer, dW0, dx0
      f32_h512_r1_D579  Dp = 584: initial layer and dx0 with N > 512
      f32_h100_r2_B33   one 32-row chunk plus one row
      f32_h64_r2_p0     inv_keep = 1, no dropout draw

    Measured on an MI355X (worst stage max |diff| / bound, worst max |diff| of
    a stored stage, worst relative error of a gradient, second run bit-equal):

      case              diff / bound   max |diff|  gradient rel. error               second run
      f32_h40_r1        7.54e-02       2.04e-06    5.85e-07 (db_f)                   bit-equal
      f32_h100_r2       1.02e-01       2.22e-06    2.30e-07 (dW1[0])                 bit-equal
      f32_h256_r2       1.85e-01       3.30e-06    2.85e-07 (dx0)                    bit-equal
      f32_h512_r2       1.27e-01       3.36e-06    4.06e-07 (dx0)                    bit-equal
      f32_h1024_r1      1.47e-01       3.35e-06    5.71e-07 (dx0)                    bit-equal
      f32_h64_r1_D164   9.69e-02       1.10e-06    4.90e-07 (cross_b[2])             bit-equal
      f32_h512_r1_D579  1.24e-01       3.59e-06    4.06e-07 (dx0)                    bit-equal
      f32_h100_r2_B33   8.95e-02       1.55e-06    4.38e-07 (cat_embeddings.7.weight) bit-equal
      f32_h64_r2_p0     3.13e-01       2.20e-06    2.55e-07 (db0)                    bit-equal

    (diff / bound: the worst stored element uses a third of its bound, 2^-18 x the
    summed |terms| = 64 fp32 roundings of them; max |diff| belongs to h0 / t, values
    of a few units summed over 456 - 1024 terms.  Before the BN-backward coefficient
    sums' own terms entered dt2's and dt1's scale (stage_check.bn_back), dt2 / dt1
    reached 1.01 - 2.6 x the bound in f32_h40_r1, f32_h100_r2 and f32_h100_r2_B33, in
    columns whose sums nearly cancel; with them the same elements sit at 0.02 - 0.04.)
    """
    _run_case(dev, case, "fp32", *F32_CASES[case], F32_INPUT_DIM.get(case, 456))


# id: (precision, hidden, blocks, dropout, B, tables, seed, plan fields expected true)
BATCH_CASES = {
    "h100_r2_B8225": ("bf16", 100, 2, 0.6, 8225, _tables(), 11, ""),
    "h250_r2_B8225": ("bf16", 250, 2, 0.6, 8225, _tables(), 11, "masks stats_epi"),
    "h100_r2_B70001": ("bf16", 100, 2, 0.6, 70001, _tables(), 11, ""),
    "f32_h96_r2_D68_B8225": ("fp32", 96, 2, 0.6, 8225, _tables(2, 16, 4), 11, ""),
    "f32_h96_r2_D68_B70001": ("fp32", 96, 2, 0.6, 70001, _tables(2, 16, 4), 11, ""),
    # past the GEMMs' 32-bit-offset launch cut (csrc/gemm_ws.hip launch_ws, csrc/gemm_wsp.hip launch_wsp)
    "h512_r2_B262241": ("bf16", 512, 2, 0.6, 262144 + 97, _tables(2, 16, 4), 11,
                        "masks stats_epi xbn head_fused rank1"),
    "h256_r2_B524385": ("bf16", 256, 2, 0.6, 524288 + 97, _tables(2, 16, 4), 11, "masks stats_epi"),
    "h512_r1_B524385": ("bf16", 512, 1, 0.6, 524288 + 97, _tables(2, 16, 4), 11,
                        "masks stats_epi xbn head_fused rank1"),
}
BATCH_INPUT_DIM = {"f32_h96_r2_D68_B8225": 68, "f32_h96_r2_D68_B70001": 68, "h512_r2_B262241": 68,
                   "h256_r2_B524385": 68, "h512_r1_B524385": 68}


@pytest.mark.parametrize("case", list(BATCH_CASES))
def test_step_stage_by_stage_batch_regimes(dev, case):
    """Narrow models at batch sizes past B = 8192, where the code that depends
    on B alone changes path, under the same stage checks and the same bit-equal
    second run.  The counts below follow csrc/elementwise.hip (run_rowcol,
    reduce_fused) and csrc/step.hip (linear_dw, make_layout) by hand.

    Reduction row passes: rows = max(32, cdiv(B, 2048)) per chunk, nc = cdiv(B, rows)
    chunks; nc > 256 takes the two-stage reduce_fused_kernel, 32 chunk groups of
    per = cdiv(nc, 32) chunks.
      B = 8225   rows = 32, nc = 258 (257 x 32 + 1: the last chunk has 1 row), per = 9:
                 groups 0 - 27 full (252 chunks), group 28 has 6, groups 29 - 31 are empty
      B = 70001  rows = 35, nc = 2001 (2000 x 35 + 1: the last chunk has 1 row), per = 63:
                 groups 0 - 30 full (1953 chunks), group 31 has 48

    fp32 weight-gradient split-K (linear_dw's generic path; Hp = 96, Dp = 72: one
    128 x 128 tile, so S = min(512, cdiv(B, 256)), kps = rup(cdiv(B, S), 64),
    S = cdiv(B, kps); slab_elems = max(64 * 96 * 96, gemm_dw_splits(96, 96, B) * 96 * 96,
    gemm_dw_splits(96, 72, B) * 96 * 72)):
      B = 8225   S = 33, kps = rup(250, 64) = 256, S = cdiv(8225, 256) = 33 (the last
                 split has 33 rows); 33 * 9216 = 304128 <= slab_elems (>= 64 * 9216): no clamp
      B = 70001  gemm_dw_splits = 256 (one 256 x 256 tile; cdiv(70001, 256) = 274 >= 64), so
                 slab_elems = 256 * 96 * 96 = 2359296.  dW1 / dW2 (96 x 96): S = 274,
                 kps = rup(256, 64) = 256, S = 274; 274 * 9216 = 2525184 > 2359296: the
                 clamp branch, S = 2359296 / 9216 = 256, kps = rup(cdiv(70001, 256) = 274, 64)
                 = 320, S = cdiv(70001, 320) = 219 (the last split has 241 rows).
                 dW0 (96 x 72): S = 274, kps = 256; 274 * 6912 = 1893888 <= 2359296: no
                 clamp, 274 splits (the last one 113 rows)

      case                   reaches
      h100_r2_B8225          bf16 block_plain: reduce_fused_kernel<bf16> with ragged and empty
                             groups and a 1-row last chunk, with a shift (the forward BN
                             statistics after col_stats: S0 = S0' + nK, S1 = S1' + 2K S0' + nK^2),
                             NK = 2 (BN1 backward, forward) and NK = 3 (BN2 backward)
      h250_r2_B8225          bf16 block_epi: the last block's bwd_bn2_stats3 partials through
                             the two-stage reduce with ragged groups; everything else still
                             from the GEMM epilogues' partials
      h100_r2_B70001         bf16: rows_per_chunk = 35 with a ragged tail, nc = 2001, last group 48
      f32_h96_r2_D68_B8225   the same reduce regime with T = float; generic split-K dW, S = 33
      f32_h96_r2_D68_B70001  rows_per_chunk = 35; linear_dw's slab clamp (dW1, dW2: S = 219,
                             kps = 320) and 274 splits on the generic kernel (dW0)

      h512_r2_B262241        every gemm_ws launch of the step in two chunks (below); the gemm_wsp
                             forward GEMMs in one
      h256_r2_B524385        gemm_ws BIAS_STATS at 4 and 8 K-tiles, RESID_BN / DROP_BN / RESID
                             without the operand transform, each in two chunks
      h512_r1_B524385        gemm_wsp BIAS_STATS in two chunks, the gemm_ws launches in three

    D = 68: user and item embeddings of 16, two categorical tables of width 16
    (250 rows), 4 numeric features.

    Past the GEMMs' launch cut.  launch_ws (csrc/gemm_ws.hip) and launch_wsp
    (csrc/gemm_wsp.hip) address with 32-bit buffer offsets and cut a call into
    M-chunks, re-basing X, C, R, Hb, r1_dz, r1_bits, headp, T, Tx and dt per chunk
    and appending each chunk's BatchNorm column partials behind the previous one's:
      gemm_ws   floor(2^29 / (2 max(ldx, 2 ldc, ldr, 2 ldhb, ldt))) rows, rounded down to
                the tile rows (64: BIAS, F32, BIAS_STATS; 32: the dX epilogues)
      gemm_wsp  floor(2^29 / (2 max(ldx, ldc))) rows, rounded down to 32
    A launch of mtiles tiles and nslices = cdiv(N, 256) column slices reports
    groups = 256 / nslices rows of `part`, or 8 cdiv(mtiles nslices, 8 nslices) if that
    is fewer (8 in every last chunk here); B = cut + 97 leaves a last chunk of
    one full 64-row tile + 33 rows, or three full 32-row tiles + 1 row.
      Hp = 512 (D = 68, Dp = 72)
        first layer, gemm_ws BIAS_STATS, K = 72 (4 K-tiles): 2 ldc = 1024 binds, cut 262144
        t1 / t2, gemm_wsp BIAS_STATS, K = 512: max(ldx, ldc) = 512, cut 524288
        dX GEMMs (RESID_BN, DROP_BN, RESID_SUM with the operand transform; the last block's
          DROP_BN without it): 2 ldc = 1024 binds, cut 262144; Tx and dt re-based with X
        dx0 (F32, K = 512, N = 72): ldx = 512 binds, cut 524288
        B = 262241: gemm_ws 262144 + 97 rows, 128 + 8 = 136 part rows; gemm_wsp and dx0 unchunked
        B = 524385: gemm_ws 262144 + 262144 + 97, 128 + 128 + 8 = 264 part rows; gemm_wsp and
                    dx0 524288 + 97, gemm_wsp 128 + 8 = 136 part rows
      Hp = 256
        first layer (K = 72, 4 K-tiles) and t1 / t2 (K = 256, 8 K-tiles), gemm_ws BIAS_STATS:
          2 ldc = 512 binds, cut 524288; one slice: 256 + 8 = 264 part rows at B = 524385
        RESID_BN, DROP_BN (264 part rows) and block 0's RESID, K = 256: the same cut
        dx0 (F32): ldx = 256 binds, cut 1048576, unchunked
    136 and 264 rows of `part` against PART_CHUNKS = 2100 (csrc/step.hip); 264 > 256
    chunks also sends GEMM-epilogue partials through the two-stage reduce_fused_kernel
    for the first time (per = cdiv(264, 32) = 9: groups 0 - 28 full, group 29 has 3,
    groups 30 and 31 are empty); at B <= 131072 they are at most 128 rows.
    Row passes (the head pass; at Hp = 256 the last block's bwd_bn2_stats3 and every
    bwd_bn1_apply2): rows = max(32, cdiv(B, 2048))
      B = 262241  rows = 129, nc = 2033 (2032 x 129 + 113), per = 64: group 31 has 49
      B = 524385  rows = 257, nc = 2041 (2040 x 257 + 105), per = 64: group 31 has 57

    Measured on an MI355X (worst stage flip fraction -- fp32: max |diff| / bound --,
    worst max |diff| of a stored stage, worst relative error of a gradient, second
    run bit-equal):

      case                   flip / bound  max |diff|  gradient rel. error   second run
      h100_r2_B8225          1.19e-04      5.77e-02    2.24e-07 (dW_f[H:])   bit-equal
      h250_r2_B8225          1.91e-04      3.12e-02    2.05e-07 (dW1[1])     bit-equal
      h100_r2_B70001         1.32e-04      6.23e-02    3.69e-07 (dW1[1])     bit-equal
      f32_h96_r2_D68_B8225   1.94e-01      1.36e-06    2.93e-07 (dW1[0])     bit-equal
      f32_h96_r2_D68_B70001  4.93e-01      1.32e-06    3.30e-07 (dW1[0])     bit-equal
      h512_r2_B262241        2.88e-04      6.22e-02    3.78e-07 (dW1[1])     bit-equal
      h256_r2_B524385        2.04e-04      6.23e-02    3.54e-07 (dW1[1])     bit-equal
      h512_r1_B524385        2.89e-04      6.24e-02    2.41e-07 (dW1[0])     bit-equal

    (bf16 max |diff|: one bf16 ulp of a value in [8, 16).)

    Wall time of the cases past the cut (stage check + second run, printed per case),
    in one run with test_bf16_step_stage_by_stage[cfg2_B131072] at 2.2 s:
    h512_r2_B262241 0.3 s, h256_r2_B524385 0.4 s, h512_r1_B524385 0.4 s.

    With launch_ws's and launch_wsp's second-chunk C pointer moved one row down (a
    scratch build, not committed) the three cases fail at h0, and
    tests/test_linear_exact_gpu.py's chunk cases from row cut - 1 on.
    """
    precision, *rest = BATCH_CASES[case]
    torch.cuda.empty_cache()   # the cases past the cut hold several GB each: one at a time
    _run_case(dev, case, precision, *rest, BATCH_INPUT_DIM.get(case, 456))


_H64 = "masks stats_epi"
_H512 = "masks stats_epi xbn head_fused rank1"
_T66 = _tables(64, 16, 8, card=12)         # 64 tables of width 4: D = 32 + 256 + 8 = 296
_T66_ODD = _tables(64, 16, 3, card=5)      # 64 tables of width 3: D = 32 + 192 + 3 = 227, Dp = 232
_D1024 = _tables(27, 64, 32, card=1000)    # 27 tables of width 32: D = 128 + 864 + 32 = 1024
_D904 = _tables(24, 64, 8, card=1000)      # 24 tables of width 32: D = 128 + 768 + 8 = 904
# id: (precision, hidden, blocks, dropout, B, tables, seed, plan fields expected true, cross layers)
LIMIT_CASES = {
    "L0": ("bf16", 64, 1, 0.6, 300, _tables(), 11, _H64, 0),
    "L4": ("bf16", 64, 1, 0.6, 300, _tables(), 11, _H64, 4),
    "L5": ("bf16", 64, 1, 0.6, 300, _tables(), 11, _H64, 5),
    "L7": ("bf16", 64, 1, 0.6, 300, _tables(), 11, _H64, 7),
    "L7_f32": ("fp32", 64, 1, 0.6, 300, _tables(), 11, "", 7),
    "L7_B257": ("bf16", 64, 1, 0.6, 257, _tables(), 11, _H64, 7),
    "r8": ("bf16", 64, 8, 0.6, 300, _tables(), 11, _H64, 3),
    "r8_f32": ("fp32", 64, 8, 0.6, 300, _tables(), 11, "", 3),
    "tab32_v4": ("bf16", 64, 1, 0.6, 300, _tables(30, 16, 8, card=12), 11, _H64, 3),
    "tab66": ("bf16", 64, 1, 0.6, 300, _T66, 11, _H64, 3),
    "tab66_odd": ("bf16", 64, 1, 0.6, 300, _T66_ODD, 11, _H64, 3),
    "tab0": ("bf16", 64, 1, 0.6, 300, _tables(0, 32, 0), 11, _H64, 3),
    "D1024_L3": ("bf16", 512, 1, 0.6, 300, _D1024, 11, _H512, 3),
    "D1024_L7": ("bf16", 512, 1, 0.6, 300, _D1024, 11, _H512, 7),
    "D904_L7": ("bf16", 512, 1, 0.6, 300, _D904, 11, _H512, 7),
    "h2041_r1": ("bf16", 2041, 1, 0.6, 300, _tables(), 11, "masks", 3),
    "h2048_r2": ("bf16", 2048, 2, 0.6, 300, _tables(), 11, "masks", 3),
    "h1100_r1": ("bf16", 1100, 1, 0.6, 300, _tables(), 11, "", 3),
    "f32_h1020_r1": ("fp32", 1020, 1, 0.6, 300, _tables(), 11, "", 3),
}
# A case's own bound for a BN-backward stage, as a multiple of the standard one: twice the
# stage's reference (coefficient sums in torch fp32) against the reference (fp64 sums), both
# from the stored inputs (stage_check's bound_x; the figures are in the test's docstring)
LIMIT_BOUNDS = {"h2041_r1": {"dt1[0]": 2 * 2.763}, "h2048_r2": {"dt1[1]": 2 * 1.297}}
LIMIT_INPUT_DIM = {"tab32_v4": 160, "tab66": 296, "tab66_odd": 227, "tab0": 64, "D1024_L3": 1024,
                   "D1024_L7": 1024, "D904_L7": 904}


@pytest.mark.parametrize("case", list(LIMIT_CASES))
def test_step_stage_by_stage_limits(dev, case):
    """The same stage checks and bit-equal second run at the limits of the
    shapes make_dims (csrc/step.hip) accepts: n_cross_layers 0..7, n_res_blocks
    1..8, 0..64 categorical tables, input width <= 1024, padded hidden width
    <= 2048 (bf16) / <= 1024 (fp32).  One past each limit is refused:
    tests/test_host_cpu.py test_model_shape_limits.

    The front (csrc/gather_cross.hip gather_cross_out): the 16-byte-lane kernels
    when every width, offset and n_num is a multiple of 4, D <= 512 and
    4 x tables <= 128 (one id register up to 16 tables, two above), among them
    gather_lowrank_kernel<L> for L = 1..4 and gather_cross_v4_kernel otherwise;
    else the general kernel gather_cross_fwd_kernel<T, RM> (RM = 8 up to 512
    columns, 16 above), whose dynamic LDS is
    ((2L + 1) D + 16 tables rounded up to 4) x 4 + 4 x RM x 64 x 2 bytes next
    to a static table map of 1320 bytes.  The cross backward
    (csrc/cross_bwd.hip) instantiates cross_coef_kernel<L> and
    x0_alpha_kernel<T, L + 1> per L.

      case          reaches
      L0            gather_cross_v4_kernel writing x0 with no cross layer (sc is u_f alone);
                    cross_coef_kernel<0>, x0_alpha_kernel<bf16, 1>
      L4            gather_lowrank_kernel<.., 4>, the last low-rank instantiation;
                    cross_coef_kernel<4>, x0_alpha_kernel<bf16, 5>
      L5            gather_cross_v4_kernel with the elementwise cross stack; cross_coef_kernel<5>
                    (61 batch-sum slots), x0_alpha_kernel<bf16, 6>
      L7            MAX_CROSS: cross_coef_kernel<7> (ns_of(7) = 113 slots a thread, red[4][113]),
                    x0_alpha_kernel<bf16, 8> (red[8][512]), 56 Gram terms of the 64-float gram
                    buffer, 8 basis vectors in the embedding backward (EmbTabs::V[8])
      L7_f32        the same with fp32 x0 (x0_alpha_kernel<float, 8>) under the one-ulp bound
      L7_B257       nblk = nx = 2: cross_coef_kernel's second block holds one sample,
                    x0_alpha_kernel's second block one row (CT = XA_ROWS = 256)
      r8            MAX_RES: Layout::h[9], mask_a1[8], mask_h[9] with mask_h[1..7], bn[16];
                    pack_all's 35 descriptors (W0, b0, the counters, 2 weights + 2 biases a
                    block) in two launches (MAX_PACK = 20)
      r8_f32        the same on block_plain with fp32 storage, no masks
      tab32_v4      emb 16, 30 tables of 12 rows (width 4), n_num 8: D = 160, 32 gathered tables,
                    4 x 32 = 128: gather_lowrank_kernel<1, 4, 2, 1, 3>, the two-register id map
      tab66         emb 16, 64 tables of 12 rows, n_num 8: D = 296, MAX_CAT: 4 x 66 > 128, the
                    general kernel (RM = 8) with 66 tables; emb_ids_kernel at 64 x 256 x 4 = 65536
                    bytes of dynamic LDS; 66-entry table arrays in the embedding backward
      tab66_odd     64 tables of 5 rows (width 3), n_num 3: D = 227, Dp = 232, 3-wide rows at odd
                    offsets (the scalar embedding-backward kernels), padded x0 columns
      tab0          no categorical tables, n_num 0, emb 32: D = 64, two gathered tables, null cat
                    and num pointers, emb_ids_kernel's K = 0 return
      D1024_L3      emb 64, 27 tables of 1000 rows (width 32), n_num 32: D = Dp = 1024, the
                    D limit: gather_cross_fwd_kernel<bf16, 16> at 16 columns a lane and
                    (7168 + 464) x 4 + 8192 = 38720 bytes; the initial layer and dW0 at K = 1024
                    (generic GEMM), dx0 at N = 1024, x0_alpha_kernel's two 512-column passes
      D1024_L7      the same at L = 7: (15360 + 464) x 4 + 8192 = 71488 bytes of dynamic LDS, past
                    the 64 KiB default (launch_fwd raises the kernel's limit; the HIP runtime of
                    the table below launched it without that too)
      D904_L7       24 tables, n_num 8: D = 904, 26 gathered tables: (13560 + 416) x 4 + 8192 =
                    64096 bytes, 65416 with the static map: the widest L = 7 request below 65536
      h2041_r1      Hp = 2048, the hidden limit: bf16 row passes at tcols = Hp / 8 = 256 = NT, one
                    row per pass; masks with 7 padded bit columns; generic GEMM at K = N = 2048;
                    the unfused head on row_dot_kernel (N > 512)
      h2048_r2      the same without padding, two blocks: mask_h[1], du through the generic dX GEMM
      h1100_r1      Hp = 1104: tcols = 138, rpp = 1, 118 idle threads per block; no masks
      f32_h1020_r1  fp32 Hp = 1024 with 4 padded columns at the fp32 row-pass limit (tcols = 256)

    Measured on an MI355X (worst stage flip fraction -- fp32: max |diff| / bound --,
    worst max |diff| of a stored stage, worst relative error of a gradient, second
    run bit-equal):

      case          flip / bound  max |diff|  gradient rel. error                 second run
      L0            1.04e-04      2.56e-02    1.13e-07 (dW_f[H:])                 bit-equal
      L4            1.04e-04      3.08e-02    2.63e-07 (cross_w[1])               bit-equal
      L5            1.04e-04      3.03e-02    2.56e-06 (dW_f[H:])                 bit-equal
      L7            1.04e-04      3.09e-02    2.60e-06 (cross_b[4])               bit-equal
      L7_f32        9.42e-02      2.20e-06    2.64e-06 (cross_b[5])               bit-equal
      L7_B257       1.22e-04      3.11e-02    2.61e-06 (cross_b[4])               bit-equal
      r8            1.56e-04      5.75e-02    2.89e-07 (cross_w[1])               bit-equal
      r8_f32        1.03e-01      2.65e-06    3.30e-07 (cross_w[1])               bit-equal
      tab32_v4      1.04e-04      2.88e-02    3.33e-07 (cat_embeddings.20.weight) bit-equal
      tab66         3.12e-04      3.11e-02    3.78e-07 (cat_embeddings.46.weight) bit-equal
      tab66_odd     5.21e-05      3.03e-02    2.78e-07 (cat_embeddings.35.weight) bit-equal
      tab0          5.21e-05      2.96e-02    2.49e-07 (dW_f[H:])                 bit-equal
      D1024_L3      2.47e-04      3.12e-02    2.84e-07 (dW_f[H:])                 bit-equal
      D1024_L7      1.95e-04      3.12e-02    3.81e-06 (cross_w[6])               bit-equal
      D904_L7       1.82e-04      3.12e-02    5.72e-06 (cross_b[2])               bit-equal
      h2041_r1      4.69e-04    3.12e-02    2.92e-07 (cross_w[1])               bit-equal
      h2048_r2      5.09e-04    3.12e-02    3.01e-07 (cross_w[2])               bit-equal
      h1100_r1      3.52e-04      3.12e-02    3.08e-07 (cross_b[2])               bit-equal
      f32_h1020_r1  1.94e-01      3.30e-06    5.75e-07 (dx0)                      bit-equal

    (L >= 5, in either precision: the cross gradients sit at 2.6e-06 - 5.7e-06, ten times
    the L <= 4 cases' and 1/35 of REL at the most; those cases take the elementwise cross
    stack, whose s_l carry the fp32 rounding of every element of x_l through the layers,
    where the low-rank front forms them from L + 1 dot products of x_0 -- supposed from
    the code, not traced.  Each case takes 0.6 - 0.9 s, the first one of a process 1.8 s.)

    The BN-backward bound at Hp = 2048.  dt = a dr - k1 xh - k2 has k1 and k2 from two sums
    over the batch, which the kernels make in fp32 per 32-row chunk (fp64 above that) and the
    reference in fp64.  Where a column's sum cancels to a small part of its summed |terms|
    the fp32 error of the sum exceeds ACC_EPS x (|k1 xh| + |k2|), and with 2048 columns and
    614400 elements a stage one such element turns up where dr = 0 and the result is
    ~4e-12, far below anything a bf16 ulp of the stage's typical values covers (the fp32
    step's bound carries the sums' own terms for this reason: stage_check.bn_back).  With the
    standard bound h2041_r1 fails at dt1[0] (1 element, 1.585 x the bound) and h2048_r2 at
    dt1[1] (1 element, 2.351 x).  The reference against itself, from the same stored inputs --
    the stage with both sums made by torch in fp32 against the stage with fp64 sums -- is off
    by MORE than the step in the first case: 2.763 x the standard bound at dt1[0] of
    h2041_r1, 1.297 x at dt1[1] of h2048_r2 (every other dt stage of both cases: reference
    vs reference 0.03 - 0.18, the step 0.50).  Those two stages alone get twice their
    figure (LIMIT_BOUNDS: 5.526 and 2.594 x the standard bound; the step's and torch's
    summation orders are two independent draws of the same error); the test prints both
    figures on every run.

    With cross_backward's switch sending n_cross = 5 to cross_coef_kernel<4> (a scratch
    build, not committed) L5 fails at dW_f[H:] (relative error 3.8e+04).
    """
    precision, *rest, n_cross = LIMIT_CASES[case]
    _run_case(dev, case, precision, *rest, LIMIT_INPUT_DIM.get(case, 456), n_cross=n_cross,
              bound_x=LIMIT_BOUNDS.get(case))
