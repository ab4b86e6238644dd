"""The train step's fused pair dcnr_forward_bce -> dcnr_backward with
DCNR_FLAG_HEAD_STATS: the forward's head pass goes on from each row's logit to
dz and to the last residual block's BN2-backward column partials, and the
backward runs no statistics pass over that block (and rebuilds that block's
rank-1 du in its dX GEMM's epilogue instead of reading a stored one).  Only
where the arithmetic runs changes, so every result must equal, bit for bit,
the three-call path dcnr_forward -> dcnr_bce_with_logits -> dcnr_backward.

Shapes (the head pass reduces over chunks of max(32, B / 2048) rows, four
thread rows per chunk; the dX GEMMs take 32-row tiles): B = 33 (a second
chunk and a second tile of one row), 1000 (32 chunks, the last of 8 rows: a
partial tile) and 4099 (129 chunks, the last of 3 rows: a thread row with
nothing to do); and, once, B = 262144 + 33, past the dX GEMMs' 32-bit-offset
launch cut (test_fused_pair_equals_three_calls_past_launch_cut)."""
import copy
import time

import pytest
import torch

import golden_common as gc
from stage_check import REL, bf, check_rel, unpack_bits

pytestmark = pytest.mark.gpu

HIDDEN = 512   # the fused head pass needs a wave per row: hidden padded to 512


def _cfg(n_res, dropout, hidden=HIDDEN):
    return dict(n_users=64, n_items=48, cat_dims={"a": 7, "b": 5}, n_num=3,
                params=dict(emb_dim=8, hidden_dim=hidden, n_cross_layers=3, n_res_blocks=n_res,
                            dropout=dropout))


def _model(cfg, dev, precision="bf16", seed=11):
    import dcnr
    torch.manual_seed(seed)
    m = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                        dict(cfg["params"]), precision=precision)
    gc.perturb_state(m, seed + 1)
    return m.to(dev).train()


def _batch(cfg, B, dev, seed=5, labels=None):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.randint(0, cfg["n_users"], (B,), device=dev, generator=g)
    i = torch.randint(0, cfg["n_items"], (B,), device=dev, generator=g)
    c = torch.stack([torch.randint(0, k, (B,), device=dev, generator=g)
                     for k in cfg["cat_dims"].values()], 1)
    n = torch.rand((B, cfg["n_num"]), device=dev, generator=g)
    y = (torch.rand((B,), device=dev, generator=g) < 0.5).float()
    if labels is not None:
        y = torch.full_like(y, float(labels))
    return u, i, c, n, y


def _step(m, sd0, batch, seed_d, fused, grad_scale, accumulate, g0):
    """One forward + loss + backward from the state ``sd0`` on either path.
    Returns (logits, loss, dz, grads, state after, workspace)."""
    from dcnr import _lib
    from dcnr.model import run_backward, run_forward
    from dcnr.ops import bce_with_logits
    m.load_state_dict(sd0)
    u, i, c, n, y = batch
    if fused:
        fl = _lib.FLAG_HEAD_STATS
        logits, ws, loss, dz = run_forward(m, True, seed_d, u, i, c, n, extra_flags=fl,
                                           bce=(y, grad_scale))
    else:
        fl = 0
        logits, ws = run_forward(m, True, seed_d, u, i, c, n)
        loss, dz = bce_with_logits(logits, y, True, grad_scale)
    grads = [g.clone() for g in g0]
    run_backward(m, u, i, c, n, dz, ws, grads, seed_d, accumulate=accumulate, extra_flags=fl)
    torch.cuda.synchronize()
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return logits, loss, dz, grads, state, ws


def _assert_same(a, b, names):
    for k, what in enumerate(("logits", "loss", "dz")):
        assert torch.equal(a[k], b[k]), what
    for name, ga, gb in zip(names, a[3], b[3]):
        assert torch.equal(ga, gb), ("grad", name, float((ga - gb).abs().max()))
    for k in a[4]:   # parameters untouched; BN running statistics and num_batches_tracked
        assert torch.equal(a[4][k], b[4][k]), ("state", k)


def _fused_pair_equals_three_calls(dev, B, n_res, dropout, grad_scales, accumulates):
    from dcnr import _lib
    cfg = _cfg(n_res, dropout)
    m = _model(cfg, dev)
    sd0 = copy.deepcopy(m.state_dict())
    batch = _batch(cfg, B, dev)
    names = [k for k, _ in m.named_parameters()]
    g = torch.Generator(device=dev).manual_seed(9)
    g0 = [torch.randn(p.shape, device=dev, generator=g) * 1e-3 for p in m.param_tensors()]
    seed_d = 0x5EED0000 + B
    for grad_scale in grad_scales:
        for accumulate in accumulates:
            old = _step(m, sd0, batch, seed_d, False, grad_scale, accumulate, g0)
            new = _step(m, sd0, batch, seed_d, True, grad_scale, accumulate, g0)
            _assert_same(old, new, names)
            assert torch.isfinite(new[1]) and all(torch.isfinite(x).all() for x in new[3])
            if n_res == 1:
                # one block: its du is stored by the head pass (the block-0 dX
                # GEMM reads it) where the statistics pass stored it
                off = m.workspace_offset(B, _lib.TRAIN, "du", 0)
                assert off >= 0
                nb = B * HIDDEN * 2
                assert torch.equal(old[5][off:off + nb], new[5][off:off + nb]), "stored du"


@pytest.mark.parametrize("dropout", [0.0, 0.6])
@pytest.mark.parametrize("n_res", [1, 2])
@pytest.mark.parametrize("B", [33, 1000, 4099])
def test_fused_pair_equals_three_calls(dev, B, n_res, dropout):
    _fused_pair_equals_three_calls(dev, B, n_res, dropout, (1.0, 0.5), (False, True))


def test_fused_pair_equals_three_calls_past_launch_cut(dev):
    """B = 262144 + 33: the dX GEMMs (hidden 512: 2 * ldc = 1024 binds, 2^29 /
    2048 = 262144 rows, csrc/gemm_ws.hip launch_ws) run as two launches, the
    second of one 32-row tile and one row.  With DCNR_FLAG_HEAD_STATS the last
    block's dX GEMM rebuilds its rank-1 residual from r1_dz + m0 and
    r1_bits + m0 * ldhb, offsets no kept-intermediates step takes
    (DCNR_FLAG_KEEP_INTERMEDIATES switches head_stats, r1_resid and own_dt
    off, so tests/test_stages_gpu.py's h512_r2_B262241 pins the stored-du path
    and this case the rebuilt one).  One grad_scale, both accumulate values;
    the same bit equality as at the small shapes.  Measured on an MI355X: 0.3 s
    (tests/test_stages_gpu.py's cfg2_B131072 case: 2.2 s in the same session)."""
    B = 262144 + 33
    assert B > (1 << 29) // (2 * 2 * HIDDEN) // 32 * 32
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    _fused_pair_equals_three_calls(dev, B, 2, 0.6, (0.5,), (False, True))
    torch.cuda.empty_cache()
    print(f"  B = {B}: wall {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("label", [0, 1])
def test_constant_labels(dev, label):
    cfg = _cfg(2, 0.6)
    m = _model(cfg, dev)
    sd0 = copy.deepcopy(m.state_dict())
    batch = _batch(cfg, 1000, dev, labels=label)
    names = [k for k, _ in m.named_parameters()]
    g0 = [torch.zeros_like(p) for p in m.param_tensors()]
    old = _step(m, sd0, batch, 77, False, 1.0, False, g0)
    new = _step(m, sd0, batch, 77, True, 1.0, False, g0)
    _assert_same(old, new, names)


def test_fused_pair_is_deterministic(dev):
    cfg = _cfg(2, 0.6)
    m = _model(cfg, dev)
    sd0 = copy.deepcopy(m.state_dict())
    batch = _batch(cfg, 4099, dev)
    names = [k for k, _ in m.named_parameters()]
    g0 = [torch.zeros_like(p) for p in m.param_tensors()]
    a = _step(m, sd0, batch, 123, True, 1.0, False, g0)
    b = _step(m, sd0, batch, 123, True, 1.0, False, g0)
    _assert_same(a, b, names)


def test_fused_pair_against_fp64(dev):
    """What the head pass now produces, against a torch fp64 recomputation
    from the step's own stored inputs (stage_check's method and bounds):
    logits and dz (rel 1e-5), and from the partials dbeta2, dgamma2 of the
    last block and dW_f[:H] (rel REL)."""
    from dcnr import _lib
    cfg = _cfg(2, 0.6)
    B, H, R = 1000, HIDDEN, 2
    m = _model(cfg, dev)
    sd0 = copy.deepcopy(m.state_dict())
    batch = _batch(cfg, B, dev)
    y = batch[4]
    g0 = [torch.zeros_like(p) for p in m.param_tensors()]
    logits, loss, dz, grads, _, ws = _step(m, sd0, batch, 321, True, 1.0, False, g0)
    gd = dict(zip([k for k, _ in m.named_parameters()], grads))

    def T(kind, idx=0, cols=H, dtype=torch.bfloat16, rows=B):
        off = m.workspace_offset(B, _lib.TRAIN, kind, idx, extra_flags=_lib.FLAG_HEAD_STATS)
        assert off >= 0, (kind, idx)
        nb = rows * cols * torch.tensor([], dtype=dtype).element_size()
        return ws[off:off + nb].view(dtype).view(rows, cols)

    V = lambda kind, idx: T(kind, idx, dtype=torch.float32, rows=1)[0]   # noqa: E731
    bi = 2 * (R - 1) + 1
    t2, hin = T("t2", R - 1).float(), T("h", R - 1).float()
    # h_R is not stored on this path: rebuilt as the pass forms it, one fp32
    # fma and one fp32 add (the fma through fp64, whose product is exact),
    # rounded to bf16 -- so the bounds below are stage_check's for a stored h_R
    pre = (t2.double() * V("bn_scale", bi).double() + V("bn_shift", bi).double()).float() + hin
    hR = bf(torch.clamp_min(pre, 0))
    off = m.workspace_offset(B, _lib.TRAIN, "mask_h", R, extra_flags=_lib.FLAG_HEAD_STATS)
    assert torch.equal(unpack_bits(ws[off:off + B * H // 8], B, H), hR > 0), "mask_h[R]"
    wf = sd0["final_linear.weight"][0].float()
    zc = T("zc", cols=1, dtype=torch.float32)[:, 0]
    check_rel("logits", logits, hR @ wf[:H] + zc + sd0["final_linear.bias"][0], 1e-5)
    # (fp32 terms, a few ulp each from expf / log1pf, summed in fp64)
    check_rel("loss", loss.reshape(1),
              torch.nn.functional.binary_cross_entropy_with_logits(logits.double(), y.double()).reshape(1), 1e-6)
    check_rel("dz", dz, (torch.sigmoid(logits.double()) - y.double()) / B, 1e-5)
    du = bf(dz[:, None] * wf[:H]) * (hR > 0).float()
    xh = (t2 - V("bn_mean", bi)) * V("bn_invstd", bi)
    check_rel("dbeta2", gd[f"res_blocks.{R - 1}.bn2.bias"], du.double().sum(0), REL)
    check_rel("dgamma2", gd[f"res_blocks.{R - 1}.bn2.weight"], (du.double() * xh.double()).sum(0), REL)
    check_rel("dW_f[:H]", gd["final_linear.weight"][0, :H], hR.double().T @ dz.double(), REL)


@pytest.mark.parametrize("precision,hidden,row_map", [("bf16", HIDDEN, True), ("bf16", HIDDEN, False),
                                                      ("fp32", 64, True)])
def test_trainer_paths_equal(dev, precision, hidden, row_map):
    """FusedTrainer with the fused pair (default) and without, 3 steps; an
    fp32 model goes through the same calls and the plan keeps the
    statistics pass."""
    import dcnr
    cfg = _cfg(2, 0.6, hidden)
    B = 1000
    m1 = _model(cfg, dev, precision)
    m2 = copy.deepcopy(m1)
    kw = dict(lr=1e-3, weight_decay=1e-4, dense_table_grads=not row_map)
    t1 = dcnr.FusedTrainer(m1, **kw)
    t2 = dcnr.FusedTrainer(m2, head_stats=False, **kw)
    assert t1.head_stats and not t2.head_stats and t1.row_map == row_map == t2.row_map
    losses = []
    for t in (t1, t2):
        torch.manual_seed(3)   # the dropout seeds follow the device generator
        ls = []
        for k in range(3):
            u, i, c, n, y = _batch(cfg, B, dev, seed=20 + k)
            loss, logits = t.step(u, i, c, n, y, return_logits=True)
            ls.append((loss.clone(), logits.clone()))
        losses.append(ls)
    torch.cuda.synchronize()
    for (la, za), (lb, zb) in zip(*losses):
        assert torch.equal(la, lb) and torch.equal(za, zb)
    assert torch.equal(t1.flat, t2.flat)
    assert torch.equal(t1.m, t2.m) and torch.equal(t1.v, t2.v)
