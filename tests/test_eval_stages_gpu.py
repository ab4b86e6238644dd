"""Stage-by-stage parity of the eval forward on every scoring path: the fused
tower (T), the default bf16 path (P: gemm_ws epilogues, head partials), the
kept path (K) and the `layers` path (L: fp32, and bf16 past Hp = 512).

The checker is tests/eval_check.py: the eval forward stores next to nothing,
so every block output h_k is made observable -- prefix models (the first k
blocks), a one-hot head (the logit IS the stored bf16 h_k[b, c]) and, for the
tower's h0, a one-block model whose block adds exactly 0 -- and each block is
pinned from the path's own h_{k-1} across the one hidden rounding (a1) with an
interval bound derived from the stored values (the bound, the other checks and
the rounding model of the L path are listed there).  Every case and path is
one test id (a probed path costs R H calls).

  case            paths    reaches
  h40_r2          T P K    tower HT = 64; gemm_ws KTP = 4
  h100_r2         T P K    Hp = 104 padded columns; HT = 128 with 28 padded
  h250_r2         T P K    KTP = 8; HT = 256
  h384_r2         T P K    KTP = 16; slices 256 + 128; 16 head parts
  h500_r1         T P K    Hp = 504, slices 256 + 248; HT = 512 with 12 padded
  h512_r3         T P K    bench width; both h buffers reused
  h512_r2_B1      T P K    one candidate
  h512_r2_B33     T P K    one 32-row tile + 1 row
  h100_r2_B129    T P K    one full 128-sample tower tile + 1 row
  h64_r1_D164     T P K    Dp = 168: the tower's zero-padded layer-0 k-steps
  h512_r1_D579    P K      Dp = 584: no tower, generic initial GEMM
  h1024_r2        L        bf16 `layers` eval: row passes, t2 stored, row_dot
  f32_h100_r2     L        fp32
  f32_h256_r2     L        fp32 fused head pass
  f32_h512_r2_B33 L        fp32
  r8              T P K    MAX_RES = MAX_RES_TW = 8 blocks: the tower's 17 packed layers, both h
                           buffers reused four times (h64)
  L7              T P K    MAX_CROSS: gather_cross_v4_kernel's elementwise cross stack in eval (h64)
  tab66           T P K    MAX_CAT: 66 gathered tables on the general front, D = 296 (h64)
  D1024_L7        P K      D = Dp = 1024 > 512: no tower; the general front at 71488 bytes of
                           dynamic LDS, the generic initial GEMM at K = 1024 (h512, one block)
  h2048_r2        L        Hp = 2048, the bf16 limit: row passes at one row a block, row_dot
  h1100_r1        L        Hp = 1104: tcols = 138, 118 idle threads a block

Measured on an MI355X (worst stage flip fraction, worst |diff| / bound of a
stored or probed activation, worst |diff| / bound of a logit, the worst
|h_R - the kept path's h_R| with the share of differing elements, second run
bit-equal):

  case            path  flip      diff/bound  logit d/b  cross-path h_R       second run
  h40_r2          T     1.67e-04  4.99e-01    1.91e-02   0                    bit-equal
  h40_r2          P     1.67e-04  4.99e-01    1.91e-02   0                    bit-equal
  h40_r2          K     1.67e-04  4.99e-01    1.91e-02   -                    bit-equal
  h100_r2         T     6.67e-05  4.99e-01    1.56e-02   1.22e-04 (3.3e-05)   bit-equal
  h100_r2         P     3.33e-05  4.99e-01    1.56e-02   0                    bit-equal
  h100_r2         K     3.33e-05  4.99e-01    1.56e-02   -                    bit-equal
  h250_r2         T     8.00e-05  4.99e-01    1.63e-02   3.91e-03 (2.4e-04)   bit-equal
  h250_r2         P     8.00e-05  4.99e-01    1.45e-02   0                    bit-equal
  h250_r2         K     8.00e-05  4.99e-01    1.53e-02   -                    bit-equal
  h384_r2         T     1.22e-04  4.98e-01    1.37e-02   1.95e-03 (1.1e-04)   bit-equal
  h384_r2         P     1.22e-04  4.98e-01    1.17e-02   0                    bit-equal
  h384_r2         K     1.22e-04  4.98e-01    1.63e-02   -                    bit-equal
  h500_r1         T     4.47e-04  7.14e-01    1.44e-02   3.91e-03 (1.1e-04)   bit-equal
  h500_r1         P     3.73e-04  7.14e-01    1.44e-02   0                    bit-equal
  h500_r1         K     3.73e-04  7.14e-01    1.44e-02   -                    bit-equal
  h512_r3         T     2.02e-04  4.98e-01    1.36e-02   7.81e-03 (1.4e-03)   bit-equal
  h512_r3         P     2.02e-04  4.98e-01    1.06e-02   0                    bit-equal
  h512_r3         K     2.02e-04  4.98e-01    1.06e-02   -                    bit-equal
  h512_r2_B1      T     0         4.93e-01    1.89e-03   0                    bit-equal
  h512_r2_B1      P     0         4.93e-01    1.89e-03   0                    bit-equal
  h512_r2_B1      K     0         4.93e-01    1.89e-03   -                    bit-equal
  h512_r2_B33     T     0         4.97e-01    9.47e-03   9.77e-04 (1.8e-04)   bit-equal
  h512_r2_B33     P     1.78e-04  4.97e-01    9.47e-03   0                    bit-equal
  h512_r2_B33     K     1.78e-04  4.97e-01    9.47e-03   -                    bit-equal
  h100_r2_B129    T     1.55e-04  4.99e-01    1.00e-02   1.22e-04 (7.8e-05)   bit-equal
  h100_r2_B129    P     7.75e-05  4.99e-01    9.25e-03   0                    bit-equal
  h100_r2_B129    K     7.75e-05  4.99e-01    1.00e-02   -                    bit-equal
  h64_r1_D164     T     0         4.99e-01    2.00e-02   0                    bit-equal
  h64_r1_D164     P     0         4.99e-01    2.02e-02   0                    bit-equal
  h64_r1_D164     K     0         4.99e-01    1.96e-02   -                    bit-equal
  h512_r1_D579    P     8.46e-05  4.98e-01    9.56e-03   0                    bit-equal
  h512_r1_D579    K     8.46e-05  4.98e-01    1.15e-02   -                    bit-equal
  h1024_r2        L     1.41e-03  5.00e-01    1.53e-02   -                    bit-equal
  f32_h100_r2     L     -         6.96e-02    1.70e-02   -                    bit-equal
  f32_h256_r2     L     -         9.11e-02    1.83e-02   -                    bit-equal
  f32_h512_r2_B33 L     -         4.98e-02    5.18e-03   -                    bit-equal
  r8              T     1.04e-04  5.00e-01    1.55e-02   7.81e-03 (1.2e-03)   bit-equal
  r8              P     1.04e-04  5.00e-01    1.56e-02   0                    bit-equal
  r8              K     1.04e-04  5.00e-01    1.56e-02   -                    bit-equal
  L7              T     5.21e-05  4.99e-01    1.69e-02   0                    bit-equal
  L7              P     5.21e-05  4.99e-01    1.82e-02   0                    bit-equal
  L7              K     5.21e-05  4.99e-01    1.90e-02   -                    bit-equal
  tab66           T     1.56e-04  4.99e-01    2.37e-02   0                    bit-equal
  tab66           P     1.56e-04  4.99e-01    2.30e-02   0                    bit-equal
  tab66           K     1.56e-04  4.99e-01    1.57e-02   -                    bit-equal
  D1024_L7        P     9.77e-05  4.98e-01    2.30e-02   0                    bit-equal
  D1024_L7        K     9.77e-05  4.98e-01    2.30e-02   -                    bit-equal
  h2048_r2        L     4.39e-03  5.00e-01    4.20e-03   -                    bit-equal
  h1100_r1        L     1.59e-03  5.00e-01    8.41e-03   -                    bit-equal

(bf16 diff / bound 0.5: the stored value is the reference rounded, half a bf16
ulp away at the most, against a bound of one ulp and more; 0.71 at h500_r1 is
one flipped element.  The default path's h_R equals the kept path's in every
case -- the same gemm_ws epilogues -- though its last GEMM never stores it; the
tower's differs from it in a rounding flip of at most 1.4e-3 of the elements,
by one bf16 ulp of a value in [1, 2) at the most.  fp32: the worst element
uses a tenth of its bound.  The one-hot probe and the h0 device reproduced the
kept path's stored h_k and h0 bit for bit in every K case.  A probed case costs
R H (the tower and the kept path: (R + 2) H) forward calls and stays below
0.3 s; the whole module ran in 7 s before the six limit cases, which stay below 0.4 s a
path.)
"""
import pytest

from eval_check import eval_check
from stage_check import ACC_EPS, BF16_ULPS, FLIP_FRAC, REL  # noqa: F401  (the bounds in force)
from test_stages_gpu import _D1024, _T66, _tables

pytestmark = pytest.mark.gpu

# id: (precision, hidden, blocks, B, tables, seed, paths, input width[, cross layers (default 3)])
# One seed serves every case: no case's flip fraction came near FLIP_FRAC with it.
CASES = {
    "h40_r2": ("bf16", 40, 2, 300, _tables(), 11, "TPK", 456),
    "h100_r2": ("bf16", 100, 2, 300, _tables(), 11, "TPK", 456),
    "h250_r2": ("bf16", 250, 2, 300, _tables(), 11, "TPK", 456),
    "h384_r2": ("bf16", 384, 2, 300, _tables(), 11, "TPK", 456),
    "h500_r1": ("bf16", 500, 1, 300, _tables(), 11, "TPK", 456),
    "h512_r3": ("bf16", 512, 3, 300, _tables(), 11, "TPK", 456),
    "h512_r2_B1": ("bf16", 512, 2, 1, _tables(), 11, "TPK", 456),
    "h512_r2_B33": ("bf16", 512, 2, 33, _tables(), 11, "TPK", 456),
    "h100_r2_B129": ("bf16", 100, 2, 129, _tables(), 11, "TPK", 456),
    "h64_r1_D164": ("bf16", 64, 1, 300, _tables(8, 16, 4), 11, "TPK", 164),
    "h512_r1_D579": ("bf16", 512, 1, 300, _tables(16, 32, 3), 11, "PK", 579),
    "h1024_r2": ("bf16", 1024, 2, 300, _tables(), 11, "L", 456),
    "f32_h100_r2": ("fp32", 100, 2, 300, _tables(), 11, "L", 456),
    "f32_h256_r2": ("fp32", 256, 2, 300, _tables(), 11, "L", 456),
    "f32_h512_r2_B33": ("fp32", 512, 2, 33, _tables(), 11, "L", 456),
    # the limits of the accepted shapes (test_stages_gpu.LIMIT_CASES has the train step's)
    "r8": ("bf16", 64, 8, 300, _tables(), 11, "TPK", 456),
    "L7": ("bf16", 64, 1, 300, _tables(), 11, "TPK", 456, 7),
    "tab66": ("bf16", 64, 1, 300, _T66, 11, "TPK", 296),
    "D1024_L7": ("bf16", 512, 1, 300, _D1024, 11, "PK", 1024, 7),
    "h2048_r2": ("bf16", 2048, 2, 300, _tables(), 11, "L", 456),
    "h1100_r1": ("bf16", 1100, 1, 300, _tables(), 11, "L", 456),
}
IDS = [(case, path) for case, v in CASES.items() for path in v[6]]


@pytest.mark.parametrize("case,path", IDS, ids=[f"{c}-{p}" for c, p in IDS])
def test_eval_stage_by_stage(dev, case, path):
    precision, hidden, n_res, B, tb, seed, _, input_dim, *n_cross = CASES[case]
    cfg = dict(n_users=tb["n_users"], n_items=tb["n_items"], cat_dims=tb["cat_dims"], n_num=tb["n_num"],
               params=dict(emb_dim=tb["emb_dim"], hidden_dim=hidden, n_cross_layers=(n_cross or [3])[0],
                           n_res_blocks=n_res, dropout=0.6))
    res = eval_check(dev, cfg, B, seed, precision, path)
    assert res["input_dim"] == input_dim
    stages = [s for s in res["stats"] if s[0] != "logits"]
    logit = next(s for s in res["stats"] if s[0] == "logits")
    assert len(stages) >= 1 + n_res
    flips = [s[1] for s in stages if s[1] is not None]
    cross = res["cross"]
    print(f"  CASE {case} {path}: flip {max(flips):.2e}" if flips else f"  CASE {case} {path}: flip -", end="")
    print(f" diff/bound {max(s[2] for s in stages):.2e} logit diff/bound {logit[2]:.2e} cross "
          + (f"{cross[0]:.2e} ({cross[1]:.1e} of h_R)" if cross else "-")
          + f" second run {'bit-equal' if res['second'] else 'DIFFERS'}")
