"""The eval checker (tests/eval_check.py) against an emulated path, on the CPU.

The emulation computes what a scoring path computes, in torch fp32 with the
storage roundings at the stored points, each GEMM summed in 32-column steps
over a permuted column order, the running-stat affine in fp32 as the kernels
form it (inv = fp32(1 / sqrt(var + eps)), sc = gamma inv, sh = beta - mean sc)
and, on the epilogue form, the Linear bias folded into the shift -- so it
differs from the checker's fp64 references the way a correct kernel does, and
must pass.  Each fault below is what a kernel's edge produces; each must fail
the check it is meant for (matched by the failing stage's name).
"""
import pytest
import torch

from eval_check import check_block, check_path, rnd

H, HP, D, DP, R, B = 100, 104, 43, 48, 2, 70   # B: two full 32-row tiles + 6 rows
FAULTS = {
    # fault: (the stage whose check must fail)
    "drop_col_lin1": r"'h\[1\]'",      # the first Linear's k-loop stops one column short
    "drop_col_lin2": r"'h\[2\]'",      # the second Linear's
    "drop_col_head": r"'logits'",      # the head dot's (one column: ~1/H of the dot)
    "no_resid_tail": r"'h\[2\]'",      # the residual missing in the rows of the ragged last tile
    "no_bias": r"'h\[1\]'",            # b2 not applied
    "no_b0": r"'h0'",                  # b0 not applied
    "no_eps": r"'scale'",              # eps left out of the affine (visible where the affine is stored)
    "bn1_for_bn2": r"'h\[1\]'",        # the affine taken from the wrong layer
    "pad_leak": r"padded columns",     # a nonzero padded column of h0, read by the next layer
    "head_unrounded": r"'logits'",     # the head reads the fp32 h_R, not the stored one
}


def _params(seed, h=H, d=D, r=R):
    g = torch.Generator().manual_seed(seed)
    uni = lambda n, k: (torch.rand((n, k), generator=g) * 2 - 1) / k ** 0.5   # noqa: E731  (nn.Linear's init)
    blocks = []
    for _ in range(r):
        p = {}
        for l in ("1", "2"):
            p["W" + l], p["b" + l] = uni(h, h), uni(1, h)[0]
            p["g" + l] = torch.rand(h, generator=g) + 0.5
            p["be" + l] = torch.randn(h, generator=g) * 0.1
            p["rm" + l] = torch.randn(h, generator=g) * 0.1
            p["rv" + l] = torch.rand(h, generator=g) + 0.5
        blocks.append(p)
    return dict(H=h, D=d, W0=uni(h, d), b0=uni(1, h)[0], blocks=blocks,
                wf=uni(1, h + d)[0], bf=uni(1, 1)[0],
                cross_w=[uni(1, d)[0] for _ in range(3)], cross_b=[torch.randn(d, generator=g) * 0.05 for _ in range(3)])


def _pad(w, rows, cols, fill=0.0):
    out = torch.full((rows, cols), fill, dtype=w.dtype)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _gemm(X, W, perm, drop=None):
    """X W^T in fp32, 32 columns a step over the permuted column order."""
    X, W = X[:, perm], W[:, perm]
    if drop is not None:
        keep = perm != drop
        X, W = X[:, keep], W[:, keep]
    acc = torch.zeros(X.shape[0], W.shape[0])
    for k in range(0, X.shape[1], 32):
        acc = acc + X[:, k:k + 32] @ W[:, k:k + 32].T
    return acc


def _affine(p, l, hp, eps=True):
    inv = (1.0 / torch.sqrt(p["rv" + l].double() + (1e-5 if eps else 0.0))).float()
    sc = p["g" + l] * inv
    sh = p["be" + l] - p["rm" + l] * sc
    return _pad(sc[None], 1, hp)[0], _pad(sh[None], 1, hp)[0]


def emulate(P, x0f, mode, layers=False, fault=None, seed=5):
    h, d = P["H"], P["D"]
    hp, dp = (h + 7) // 8 * 8, (d + 7) // 8 * 8
    g = torch.Generator().manual_seed(seed)
    r32 = lambda t: rnd(t, mode).float()   # noqa: E731
    wq = (lambda w: w.to(torch.bfloat16).float()) if mode == "bf16" else (lambda w: w)   # noqa: E731
    relu = lambda t: torch.clamp_min(t, 0)   # noqa: E731
    nb = x0f.shape[0]
    x0 = _pad(r32(x0f), nb, dp)
    h0 = r32(_gemm(x0, _pad(wq(P["W0"]), hp, dp), torch.randperm(dp, generator=g))
             + (0 if fault == "no_b0" else _pad(P["b0"][None], 1, hp)[0]))
    wfill = 0.0
    if fault == "pad_leak":   # the pad holds a value, and the next layer's k-loop reads it
        h0[:, h:] = 0.5
        wfill = 0.25
    hs, blocks, aff = [h0], [], []
    v_last = None
    for j, p in enumerate(P["blocks"]):
        X = hs[-1]
        perm = torch.randperm(hp, generator=g)
        W1 = _pad(wq(p["W1"]), hp, hp)
        W1[:h, h:] = wfill
        W2 = _pad(wq(p["W2"]), hp, hp)
        b1, b2 = _pad(p["b1"][None], 1, hp)[0], _pad(p["b2"][None], 1, hp)[0]
        sc1, sh1 = _affine(p, "1", hp, fault != "no_eps")
        sc2, sh2 = _affine(p, "2", hp, fault != "no_eps")
        aff += [(sc1, sh1), (sc2, sh2)]
        if fault == "no_bias" and j == 0:
            b2 = torch.zeros_like(b2)
        u1, u2 = (sc1, sh1), ((sc1, sh1) if fault == "bn1_for_bn2" and j == 0 else (sc2, sh2))
        acc1 = _gemm(X, W1, perm, h - 1 if fault == "drop_col_lin1" and j == 0 else None)
        o = dict(X=X)
        if layers:
            a1 = r32(relu(r32(acc1 + b1) * u1[0] + u1[1]))
        else:
            a1 = r32(relu(acc1 * u1[0] + (b1 * u1[0] + u1[1])))
        acc2 = _gemm(a1, W2, perm, h - 1 if fault == "drop_col_lin2" and j == 1 else None)
        res = X.clone()
        if fault == "no_resid_tail" and j == 1:
            res[nb // 32 * 32:] = 0
        if layers:
            o["t2"] = r32(acc2 + b2)
            o["sc2"], o["sh2"] = sc2, sh2
            v_last = relu(o["t2"] * u2[0] + u2[1] + res)
        else:
            v_last = relu(acc2 * u2[0] + (b2 * u2[0] + u2[1]) + res)
        o["got"] = r32(v_last)
        hs.append(o["got"])
        blocks.append(o)
    x = x0f
    for w, b in zip(P["cross_w"], P["cross_b"]):
        x = x + x * (x @ w)[:, None] + b
    zc = x @ P["wf"][h:]
    hu = (v_last if fault == "head_unrounded" else hs[-1])[:, :h]
    perm = torch.randperm(h, generator=g)
    if fault == "drop_col_head":
        perm = perm[perm != h - 1]
    z = _gemm(hu, P["wf"][None, :h], perm)[:, 0] + zc + P["bf"]
    return dict(x0=x0, x0f=x0f, zc=zc, h0=h0, blocks=blocks, affine=aff, logits=z, hR=hs[-1])


def _inputs(seed, nb=B, d=D):
    return torch.randn((nb, d), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("layers", [False, True], ids=["epilogue", "layers"])
@pytest.mark.parametrize("h", [100, 256])
def test_emulated_path_passes(mode, layers, h):
    """A correct path in another summation order passes every check, with room:
    the worst |diff| / bound stays below 1 and the bf16 flip fraction far
    below the cap."""
    P = _params(3, h=h)
    stats = check_path(emulate(P, _inputs(4), mode, layers), P, mode)
    assert len(stats) >= 2 + R
    worst = max(s[2] for s in stats)
    flips = max((s[1] for s in stats if s[1] is not None), default=0.0)
    print(f"{mode} {'layers' if layers else 'epilogue'} H={h}: worst diff/bound {worst:.2f} flips {flips:.1e}")
    assert worst < 1.0 and flips < 0.01


@pytest.mark.parametrize("fault", list(FAULTS))
def test_fault_fails_the_check(fault):
    P = _params(3)
    with pytest.raises(AssertionError, match=FAULTS[fault]):
        check_path(emulate(P, _inputs(4), "bf16", fault=fault), P, "bf16")


@pytest.mark.parametrize("fault", ["drop_col_lin1", "drop_col_lin2", "no_resid_tail", "no_bias", "bn1_for_bn2"])
def test_fault_fails_the_check_fp32_layers(fault):
    """The same block faults on the form that stores t1 and t2, in fp32."""
    P = _params(3)
    with pytest.raises(AssertionError, match=r"h\[[12]\]"):
        check_path(emulate(P, _inputs(4), "fp32", layers=True, fault=fault), P, "fp32")


def test_pad_leak_fails_the_block_bound_too():
    """A padded column cannot be seen through a probe; what it leaks into the
    real columns of the next layer fails that block's bound."""
    P = _params(3)
    em = emulate(P, _inputs(4), "bf16", fault="pad_leak")
    o = em["blocks"][0]
    with pytest.raises(AssertionError, match=r"'h\[1\]'"):
        check_block("h[1]", o["got"][:, :H], o["X"][:, :H], P["blocks"][0], "bf16", [])


def test_dropped_column_is_many_elements():
    """One dropped column of a1 (B = 300, H = 100) moves h_2 by less than 1e-2
    in relative norm, the strength of the end-to-end eval comparisons, and puts
    more than a thousand of its elements out of bound."""
    P = _params(3)
    em = emulate(P, _inputs(4, nb=300), "bf16", fault="drop_col_lin2")
    ok = emulate(P, _inputs(4, nb=300), "bf16")
    o = em["blocks"][1]
    want = ok["blocks"][1]["got"]
    assert (o["got"] - want).norm() / want.norm() < 1e-2
    with pytest.raises(AssertionError) as e:
        check_block("h[2]", o["got"][:, :H], o["X"][:, :H], P["blocks"][1], "bf16", [])
    assert e.value.args[0][1] > 1000, e.value.args[0][:4]
