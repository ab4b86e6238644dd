"""The weight gradient's split-K combine (splitk_t_sum / splitk_t_store,
csrc/dcnr_internal.h): 32 k x 32 n tiles, one whole 128-B slab line per
wave-level load, used by gemm_dw's tail and by splitk_reduce_t.

1. In-tail against stand-alone.  dcnr_backward on a small bf16 model twice
   from identical inputs: plainly (the weight gradients go down the side-stream
   pipe, each call's combine in the next gemm_dw launch's tail, the last one at
   the join) and with launch profiling on (every launch on the caller's stream:
   gemm_dw, then the stand-alone splitk_reduce_t).  Same per-element sum either
   way, so every gradient must be torch.equal.  1 and 3 residual blocks: 3 and
   7 calls in the chain, so both slabs are combined in a tail.

2. dcnr_linear_wgrad_bf16 against a fixed-order emulation: fp32 partials of
   each batch split, summed over ascending z in fp32 on the host.  The inputs
   are small integers (|x| <= 3), so each partial is an integer of at most
   9 * B <= 73728 < 2^24: exact in fp32 in any accumulation order, exact from
   an fp64 matmul, and the ascending-z chain (and the accumulate add onto an
   integer-valued dW) is exact too.  torch.equal is then a fair demand.
   Shapes: two full 256 x 256 tiles each way; the initial layer's ragged K;
   N and K no multiples of the 32 x 32 combine tile (264 = 8 * 32 + 8,
   40 = 32 + 8) at the minimum of 8 splits; a single partial tile."""
import copy

import pytest
import torch

import golden_common as gc

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- in-tail vs stand-alone
def _cfg(hidden, wide, n_res):
    if wide:   # input width 32 * 2 + 12 * 32 + 8 = 456
        cat, n_num, emb = {f"c{k}": 1000 for k in range(12)}, 8, 32
    else:      # input width 8 * 2 + 2 * 8 + 8 = 40
        cat, n_num, emb = {"a": 63, "b": 63}, 8, 8
    return dict(n_users=64, n_items=48, cat_dims=cat, n_num=n_num,
                params=dict(emb_dim=emb, hidden_dim=hidden, n_cross_layers=3, n_res_blocks=n_res,
                            dropout=0.0))


def _backward(m, sd0, batch, ws_fwd, dz, seed, accumulate, g0, profiled, n_dw):
    from dcnr import _lib
    from dcnr.model import run_backward
    m.load_state_dict(sd0)
    u, i, c, n = batch
    ws = ws_fwd.clone()
    grads = [g.clone() for g in g0]
    _lib.profile_enable(1 if profiled else 0)
    try:
        run_backward(m, u, i, c, n, dz, ws, grads, seed, accumulate=accumulate)
        torch.cuda.synchronize()
    finally:
        _lib.profile_enable(0)
        prof = _lib.profile_collect()
    # the profiled run took the stand-alone path: one gemm_dw launch per Linear
    assert prof["gemm_dw"][1] == (n_dw if profiled else 0), prof
    return grads


@pytest.mark.parametrize("n_res", [1, 3])
@pytest.mark.parametrize("hidden,wide,B", [(512, True, 4096), (384, False, 2048), (64, False, 256)])
def test_tail_combine_equals_standalone(dev, hidden, wide, B, n_res):
    import dcnr
    from dcnr.model import run_forward
    from dcnr.ops import bce_with_logits
    cfg = _cfg(hidden, wide, n_res)
    torch.manual_seed(11)
    m = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                        dict(cfg["params"]), precision="bf16")
    gc.perturb_state(m, 12)
    m = m.to(dev).train()
    sd0 = copy.deepcopy(m.state_dict())
    g = torch.Generator(device=dev).manual_seed(5)
    u = torch.randint(0, cfg["n_users"], (B,), device=dev, generator=g)
    i = torch.randint(0, cfg["n_items"], (B,), device=dev, generator=g)
    c = torch.stack([torch.randint(0, k, (B,), device=dev, generator=g)
                     for k in cfg["cat_dims"].values()], 1)
    n = torch.rand((B, cfg["n_num"]), device=dev, generator=g)
    y = (torch.rand((B,), device=dev, generator=g) < 0.5).float()
    seed = 0x5EED0000 + B
    logits, ws = run_forward(m, True, seed, u, i, c, n)
    _, dz = bce_with_logits(logits, y, True, 1.0)
    torch.cuda.synchronize()
    names = [k for k, _ in m.named_parameters()]
    g0 = [torch.randn(p.shape, device=dev, generator=g) * 1e-3 for p in m.param_tensors()]
    for accumulate in (False, True):   # (no DCNR_FLAG_ROW_MAP here, so accumulate = 1 is allowed)
        n_dw = 1 + 2 * n_res   # the initial Linear and two per residual block
        tail = _backward(m, sd0, (u, i, c, n), ws, dz, seed, accumulate, g0, False, n_dw)
        alone = _backward(m, sd0, (u, i, c, n), ws, dz, seed, accumulate, g0, True, n_dw)
        for name, a, b in zip(names, tail, alone):
            if "embedding" not in name:   # every dense gradient tensor
                assert torch.isfinite(a).all(), name
                assert torch.equal(a, b), (name, accumulate, float((a - b).abs().max()))


# ---------------------------------------------------------------- fixed-order emulation
def _splits(N, K, B):
    """gemm_dw_splits and the rows per split of dw_args (csrc/gemm_dw.hip,
    csrc/step.hip), checked against the library's workspace size."""
    tiles = -(-N // 256) * -(-K // 256)
    s = max(8, (256 // tiles) // 8 * 8)
    while s > 8 and -(-B // s) < 64:
        s -= 8
    per = (-(-B // s) + 63) // 64 * 64
    return s, per


_REF = {}


def _reference(N, K, B):
    """(dY, X, base, ref) on the host: bf16 inputs, an integer-valued dW to
    accumulate onto, and ref[acc] = (base if acc else +0) + the ascending-z
    fp32 chain over the splits' partials.  Computed once per shape; the
    exactness the docstring claims is asserted here (on the CPU, no device)."""
    key = (N, K, B)
    if key in _REF:
        return _REF[key]
    g = torch.Generator().manual_seed(N * 7 + K * 3 + B)
    dY = torch.randint(-3, 4, (B, N), generator=g).to(torch.bfloat16)
    X = torch.randint(-3, 4, (B, K), generator=g).to(torch.bfloat16)
    base = torch.randint(-64, 65, (N, K), generator=g).float()
    S, per = _splits(N, K, B)
    acc = torch.zeros(N, K, dtype=torch.float32)
    tot = torch.zeros(N, K, dtype=torch.float64)
    for z in range(S):
        lo, hi = min(B, z * per), min(B, (z + 1) * per)
        p64 = dY[lo:hi].double().t() @ X[lo:hi].double()
        p32 = p64.float()
        assert torch.equal(p32.double(), p64) and float(p64.abs().max()) <= 9.0 * (hi - lo)
        acc = acc + p32           # plain fp32 adds, ascending z, from +0
        tot += p64
    assert torch.equal(acc.double(), tot) and float(tot.abs().max()) < 2 ** 24 - 64
    full = dY.double().t() @ X.double()
    assert torch.equal(full, tot)
    ref = {0: acc, 1: base + acc}
    assert torch.equal(ref[1].double(), base.double() + tot)
    _REF[key] = (dY, X, base, ref)
    return _REF[key]


def _run_wgrad(dev, N, K, B, accumulate, offset):
    from dcnr import _lib
    dY, X, base, ref = _reference(N, K, B)
    lib = _lib.load()
    nbytes = int(lib.dcnr_linear_wgrad_workspace_size(N, K, B))
    assert nbytes == _splits(N, K, B)[0] * N * K * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dYd, Xd = dY.to(dev), X.to(dev)
    buf = torch.full((N * K + 4,), float("nan"), device=dev)
    dW = buf[offset:offset + N * K].view(N, K)
    assert dW.data_ptr() % 16 == 4 * offset
    if accumulate:
        dW.copy_(base.to(dev))
    _lib.check(lib.dcnr_linear_wgrad_bf16(dYd.data_ptr(), N, Xd.data_ptr(), K, B, N, K,
                                          dW.data_ptr(), accumulate, ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr(dev)), "wgrad")
    torch.cuda.synchronize()
    out = dW.cpu()
    bad = (out != ref[accumulate]) | out.isnan()
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:4].tolist())
    assert torch.equal(out, ref[accumulate])
    # nothing written outside dW
    assert buf[:offset].isnan().all() and buf[offset + N * K:].isnan().all()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N,K,B", [(512, 512, 8192), (512, 456, 4096), (264, 40, 640), (8, 8, 128)])
def test_wgrad_equals_fixed_order_emulation(dev, N, K, B, accumulate):
    _run_wgrad(dev, N, K, B, accumulate, 0)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_wgrad_scalar_store_path(dev, accumulate):
    """dW 4 bytes off a 16-B boundary: the combine's scalar store path."""
    _run_wgrad(dev, 264, 40, 640, accumulate, 1)
