"""Stage-by-stage parity of the bf16 training step (the benchmarked path).

The checker is tests/stage_check.py: every tensor a kept-intermediates step
stores is recomputed in torch fp32/fp64 from the kernels' own stored inputs of
that stage and compared (stages, reference lines and tolerances are listed
there).  test_bf16_step_stage_by_stage runs it at the benchmark's shapes,
test_bf16_step_stage_by_stage_paths at small shapes that take every other
kernel path, and then runs the same step again in the layout a real step uses.
"""
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
    stage_check(dev, cfg, B, 7)


# golden_common.CFG3R's tables and cross network (D = 456), as tests/test_paths_gpu.py's CFG
def _tables(n_cat=12, emb=32, n_num=8):
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
    hidden, n_res, p, B, tb, seed, flags = PATH_CASES[case]
    cfg = dict(n_users=tb["n_users"], n_items=tb["n_items"], cat_dims=tb["cat_dims"], n_num=tb["n_num"],
               params=dict(emb_dim=tb["emb_dim"], hidden_dim=hidden, n_cross_layers=3,
                           n_res_blocks=n_res, dropout=p))
    assert {k for k, v in expected_plan(hidden).items() if v} == set(flags.split()), "the case's path"
    res = stage_check(dev, cfg, B, seed)
    assert res["grads"]["initial_deep_layer.weight"].shape[1] == INPUT_DIM.get(case, 456)
    logits, loss, grads = res["plain_step"]()
    diff = [k for k, g in res["grads"].items() if not torch.equal(g, grads[k])]
    if not torch.equal(logits, res["logits"]):
        diff.append("logits")
    if not torch.equal(loss, res["loss"]):
        diff.append("loss")
    worst = max((q for q in res["rels"] if q[2] == REL), key=lambda q: q[1])
    print(f"  CASE {case}: flip {max(s[1] for s in res['stats']):.2e} diff "
          f"{max(s[2] for s in res['stats']):.2e} rel {worst[1]:.2e} ({worst[0]}) "
          f"second run {'bit-equal' if not diff else 'DIFFERS ' + str(diff)}")
    assert not diff, diff
