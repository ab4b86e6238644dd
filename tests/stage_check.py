"""Stage-by-stage check of one training step, bf16 or fp32, on whichever
kernel path the step's plan takes (csrc/step.hip make_plan).

End to end a bf16 step cannot be pinned element-wise to any other
implementation (tests/test_bf16_train_gpu.py explains the sensitivity), and
the fp32 step's end-to-end comparison (a norm-relative 5e-3 on the gradients)
cannot see a dropped row or a mis-handled padded column, but every STAGE can
be pinned: each tensor the kernels store is recomputed here, in torch
fp32/fp64 on the device (bf16) or in fp64 throughout (fp32), from the kernels'
OWN stored inputs of that stage, and compared.  The workspace keeps every
block's backward buffers (DCNR_FLAG_KEEP_INTERMEDIATES) and tells where each
tensor lives (dcnr_workspace_offset).  Stages and reference lines (the bounds
in the right column are the bf16 step's; the fp32 step's follow below):

  forward  (train.py:155-170, ResBlock 112-122)
    x0          gather + concat, bf16 store                       exact
    h0, t1, t2  Linear (bf16 operands, fp32 accumulate) + bias     <= BF16_ULPS ulp
    BN stats    mean / invstd of the stored t (fp64 sums)          rel 1e-5
    a1          dropout(relu(t1 * scale + shift)), keep mask       <= BF16_ULPS ulp
    h_{j+1}     relu(t2 * scale + shift + h_j)                     <= BF16_ULPS ulp
    masks       1-bit [a1 != 0], [h_j > 0] images                  exact
    logits      h_R . w_f[:H] + zc + b_f                           rel 1e-5
    sc          s_l, x_0 . w_m, x_0 . w_f[H:] (cross scalars)      rel 1e-5
  backward (loss.backward(), train.py:225)
    du_{R-1}    dz w_f[:H] * [h_R > 0]                             <= BF16_ULPS ulp
    dt2, dt1    BN backward apply (coefficients from fp64 sums)     <= BF16_ULPS ulp
    da          (dt2 W2) / (1-p) * [a1 != 0]                        <= BF16_ULPS ulp
    du_{j-1}    (dt1 W1 + du_j) * [h_j > 0];  G = dt1_0 W1 + du_0  <= BF16_ULPS ulp
    dW, db, dgamma, dbeta, dW_f, cross, embedding grads (fp32 sums)  rel 2e-4
    dx0_cross   sum_k xcoef_k V_k (low-rank cross backward)         rel 2e-4
    (the cross weight grads' x_0 part is summed over the stored bf16 x0)

A bf16 value within BF16_ULPS units in the last place (plus ACC_EPS times
the magnitude of the summed terms): the kernels and this recomputation
accumulate in different orders, which moves a value across a bf16 rounding
boundary now and then (the fraction of such elements is recorded and bounded
by FLIP_FRAC).  A case may state a bound of its own for a BN-backward stage
(``bound_x``), a multiple of this one that comes from measuring the
reference against itself (bn_back32); tests/test_stages_gpu.py's limit cases
say where and why.

precision="fp32" (the parity path: block_plain, no masks, fp32 storage).  The
stages, buffers and every "rel" bound above are the same; what changes is the
rounding model of a stored value:

  storage    activations and gradients are read as fp32, the weights are the
             fp32 parameters themselves, the stored x0 equals the gathered
             rows exactly.
  reference  every reference of a stored tensor is computed in fp64 (an fp32
             torch matmul is accurate against a bf16 ulp, not against an fp32
             one).
  bound      |got - ref| <= one fp32 ulp of ref + ACC_EPS x the summed |terms|
             (the same ``scale`` the bf16 checks pass).  ACC_EPS = 2^-18 is 64
             fp32 roundings of the summed magnitude: above the sqrt(K) 2^-24
             typical error of a K <= 1024 fp32 sum, below its K 2^-24 worst
             case (the GEMM's v_mfma_f32_16x16x4_f32 makes exact fp32 fma
             chains).  No flip fraction; max |diff| / bound is recorded per
             stage instead.
  dt2, dt1   the summed |terms| include the B terms of each BN-backward
             coefficient sum (a sum(|dr xh|) / B |xh| + a sum(|dr|) / B), at
             min(ACC_EPS, B 2^-24): the kernels' fp32 chunk sums are off by a few
             roundings of these magnitudes, which |k1 xh| + |k2| alone fall
             below where the signs cancel (bn_back).
  da         the GEMM stores fp32 dt2 W2 and bwd_bn1_stats overwrites it with
             that * keep/(1-p) * [fma(t1, scale, shift) > 0]: masked elements
             exactly 0, the others within inv_keep x the GEMM's bound plus one
             fp32 ulp of the fp64 dt2 W2 inv_keep (check_da_fp32).
  plan       no masks are materialised (every mask offset is -1); the fused
             head pass runs at Hp == 256 (a wave per row at 4 columns a lane).

What follows the plan (Hp = hidden rounded up to 8):

  masks      exist iff Hp % 32 == 0, mask_h[R] iff in addition Hp == 512 (the
             fused head pass); dcnr_workspace_offset must say so (>= 0 / -1),
             and a mask's padded columns' bits must be 0.
  da         with the BN statistics in the GEMM epilogues (masks and
             Hp <= 512) the dX GEMM's epilogue applies 1/(1-p) [a1 != 0] to
             its fp32 accumulator: one rounding.  Otherwise (block_plain) the
             GEMM stores bf16(dt2 W2) and bwd_bn1_stats overwrites it with
             bf16(that * keep/(1-p) * [fma(t1, scale, shift) > 0]): two
             roundings.  check_da_plain applies BF16_ULPS and ACC_EPS to the
             first rounding, where the summation order enters, and asks the
             second one, an exact elementwise product of the stored value,
             to be exact.
  padding    for hidden != Hp the columns hidden..Hp-1 of every stored
             activation and gradient, and the columns D..Dp-1 of x0, must
             be exactly 0.
"""
import numpy as np
import torch

import golden_common as gc
from helpers import dropout_mask_torch

BF16_ULPS = 1
ACC_EPS = 2.0 ** -18     # fp32 accumulation-order allowance, relative to the summed |terms|
FLIP_FRAC = 0.02
REL = 2e-4


def bf(t):
    return t.to(torch.bfloat16).float()


def ulp_bf16(x):
    """One bf16 unit in the last place at |x| (8 significant bits)."""
    a = x.abs().clamp_min(1e-30)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def tol_bf16(ref, scale):
    return BF16_ULPS * ulp_bf16(ref.float()) + ACC_EPS * scale.float() + 1e-30


def check_bf16(name, got, ref, stats, scale, factor=1.0):
    """``scale``: the magnitude of the terms that were summed into each value
    (|X| @ |W|^T for a GEMM, the sum of |terms| for an elementwise stage):
    different fp32 summation orders / FMA contractions differ by a few fp32
    ulps of it, which near a cancellation can exceed a bf16 ulp of the
    result.  ``factor``: a case's own multiple of the bound for this stage
    (stage_check's ``bound_x``)."""
    got, ref = got.float(), ref.float()
    d = (got - ref).abs()
    assert torch.isfinite(got).all(), name
    tol = factor * tol_bf16(ref, scale)
    bad = d > tol * 1.0001
    # values that are exactly zero on one side only: legitimate only as a
    # rounding flip of a tiny value (never for masked elements)
    nb = int(bad.sum())
    flips = float((got != bf(ref)).float().mean())   # vs the reference rounded to bf16
    stats.append((name, flips, float(d.max())))
    assert nb == 0, (name, nb, float(d.max()), got[bad][:5].tolist(), ref[bad][:5].tolist())
    assert flips <= FLIP_FRAC, (name, flips)


def check_da_plain(name, got, m_ref, mask, inv_keep, stats, scale):
    """block_plain's stored da = bf16(c * inv_keep) * mask with c = the dX
    GEMM's stored bf16(dt2 W2), which is no longer in memory.  ``m_ref``: the
    recomputed dt2 W2 (fp32).  Masked elements must be exactly 0; for every
    other element some bf16 c with bf16(c * inv_keep) == got must lie within
    check_bf16's tolerance of m_ref (the candidates: the five bf16 values
    around got / inv_keep; a product by inv_keep < 4 maps at most two
    neighbouring c to one bf16 value)."""
    got, m_ref = got.float(), m_ref.float()
    assert torch.isfinite(got).all(), name
    assert (got[~mask] == 0).all(), (name, "masked elements not 0")
    tol = BF16_ULPS * ulp_bf16(m_ref) + ACC_EPS * scale.float() + 1e-30
    qb = bf(got.abs() / inv_keep).to(torch.bfloat16).view(torch.int16).to(torch.int32)
    ok = torch.zeros_like(mask)
    for k in range(-2, 3):
        c = (qb + k).clamp(0, 0x7F7F).to(torch.int16).view(torch.bfloat16).float() * torch.sign(got)
        ok |= (bf(c * inv_keep) == got) & ((c - m_ref).abs() <= tol * 1.0001)
    bad = mask & ~ok
    nb = int(bad.sum())
    ref = bf(bf(m_ref) * inv_keep) * mask.float()
    flips = float((got != ref).float().mean())
    stats.append((name, flips, float((got - ref).abs().max())))
    assert nb == 0, (name, nb, got[bad][:5].tolist(), (m_ref * inv_keep)[bad][:5].tolist())
    assert flips <= FLIP_FRAC, (name, flips)


def ulp_fp32(x):
    """One fp32 unit in the last place at |x| (24 significant bits; the
    subnormals' spacing below 2^-126)."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def _fp32_stat(name, got, d, tol, bad, stats, refs):
    nb = int(bad.sum())
    stats.append((name, float((d / tol).max()), float(d.max())))
    assert nb == 0, (name, nb, float(d.max()), float((d / tol).max()), bad.nonzero()[:5].tolist(),
                     got[bad][:5].tolist(), refs[bad][:5].tolist())


def check_fp32(name, got, ref, stats, scale):
    """A stored fp32 tensor against its fp64 reference: one fp32 ulp of the
    reference plus ACC_EPS times ``scale`` (check_bf16's argument).  Records
    (name, max |diff| / bound, max |diff|)."""
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), name
    d = (got - ref).abs()
    tol = ulp_fp32(ref) + ACC_EPS * scale.double()
    _fp32_stat(name, got, d, tol, d > tol, stats, ref)


def check_da_fp32(name, got, m_ref, mask, inv_keep, stats, scale):
    """The fp32 step's stored da = fp32(c * inv_keep) * mask with c = the dX
    GEMM's stored fp32 dt2 W2 (overwritten in place).  ``m_ref``: dt2 W2 in
    fp64.  Masked elements must be exactly 0; the others lie within inv_keep
    times the GEMM's bound (check_fp32's, at m_ref) plus the product's own
    rounding, one fp32 ulp of m_ref * inv_keep."""
    got, m_ref = got.double(), m_ref.double()
    assert torch.isfinite(got).all(), name
    assert (got[~mask] == 0).all(), (name, "masked elements not 0")
    ref = m_ref * inv_keep * mask.double()
    d = (got - ref).abs()
    tol = inv_keep * (ulp_fp32(m_ref) + ACC_EPS * scale.double()) + ulp_fp32(m_ref * inv_keep)
    _fp32_stat(name, got, d, tol, mask & (d > tol), stats, ref)


def check_rel(name, got, ref, tol=REL, rels=None):
    got, ref = got.double(), ref.double()
    e = ((got - ref).norm() / ref.norm().clamp_min(1e-300)).item()
    if rels is not None:
        rels.append((name, e, tol))
    assert e <= tol, (name, e)


def unpack_bits(b, B, Hp):
    sh = torch.arange(8, device=b.device, dtype=torch.uint8)
    return ((b.view(B, Hp // 8)[:, :, None] >> sh) & 1).reshape(B, Hp).bool()


def expected_plan(H, precision="bf16"):
    """make_plan's train fields for a model of hidden width H.  fp32: no masks,
    no GEMM epilogues; the fused head pass (bn_add_relu_head_supported: a wave
    per row, 4 fp32 columns a lane) at Hp == 256."""
    Hp = (H + 7) // 8 * 8
    if precision == "fp32":
        return dict(masks=False, stats_epi=False, xbn=False, head_fused=Hp == 256, rank1=False)
    masks = Hp % 32 == 0
    stats_epi = masks and Hp <= 512
    head_fused = Hp == 512
    return dict(masks=masks, stats_epi=stats_epi, xbn=stats_epi and Hp > 256,
                head_fused=head_fused, rank1=masks and head_fused)


def stage_check(dev, cfg, B, seed, precision="bf16", bound_x=None):
    """One kept-intermediates train step of a model built from ``cfg`` at B
    samples (weights from ``seed``, state perturbed with ``seed + 1``, inputs
    from ``seed - 2``), every stage checked.  ``bound_x`` (bf16): {stage: factor}
    for the BN-backward stages (dt2[j], dt1[j]) whose bound a case widens to
    ``factor`` times the standard one; for each of them the reference is first
    measured against itself (bn_back32) and the figure printed -- the factor
    is to be twice that figure, written down with the case.  Returns a dict: ``logits``,
    ``loss``, ``grads`` (by parameter name), ``stats`` ((stage, flip fraction
    -- fp32: max |diff| / bound --, max |diff|) per stored stage), ``rels``
    ((name, relative error, bound) per fp32
    quantity), ``plan`` (expected_plan) and ``plain_step``: a callable that
    runs the same step (same weights, inputs and dropout seed) without
    keep_intermediates and returns (logits, loss, grads)."""
    import dcnr
    from dcnr import _lib
    from dcnr.model import dropout_seed, run_backward, run_forward
    from dcnr.ops import bce_with_logits
    assert precision in ("bf16", "fp32"), precision
    is_bf = precision == "bf16"
    st = torch.bfloat16 if is_bf else torch.float32   # the storage type
    cd = torch.float32 if is_bf else torch.float64    # the references' arithmetic
    torch.manual_seed(seed)
    m = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                        dict(cfg["params"]), precision=precision)
    gc.perturb_state(m, seed + 1)
    m = m.to(dev).train()
    m.keep_intermediates = True
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator(device=dev).manual_seed(seed - 2)
    K = len(cfg["cat_dims"])
    cards = list(cfg["cat_dims"].values())
    u = torch.randint(0, cfg["n_users"], (B,), device=dev, generator=g)
    i = torch.randint(0, cfg["n_items"], (B,), device=dev, generator=g)
    c = (torch.stack([torch.randint(0, n, (B,), device=dev, generator=g) for n in cards], 1) if cards
         else torch.zeros((B, 0), dtype=torch.int64, device=dev))   # no categorical tables
    n = torch.rand((B, cfg["n_num"]), device=dev, generator=g)
    y = (torch.rand((B,), device=dev, generator=g) < 0.5).float()
    p = cfg["params"]["dropout"]
    R, H = cfg["params"]["n_res_blocks"], cfg["params"]["hidden_dim"]
    Hp = (H + 7) // 8 * 8
    D = m._dims["input_dim"]
    Dp = (D + 7) // 8 * 8
    plan = expected_plan(H, precision)
    names = [k for k, _ in m.named_parameters()]

    seed_d = dropout_seed(dev)

    def step():
        logits, ws = run_forward(m, True, seed_d, u, i, c, n)
        loss, dz = bce_with_logits(logits, y)
        grads = [torch.empty_like(q) for q in m.param_tensors()]
        run_backward(m, u, i, c, n, dz, ws, grads, seed_d)
        torch.cuda.synchronize()
        return logits, loss, dz, ws, dict(zip(names, grads))

    logits, loss, dz, ws, gd = step()

    def plain_step():
        m.keep_intermediates = False
        try:
            lg, ls, _, _, gr = step()
        finally:
            m.keep_intermediates = True
        return lg, ls, gr

    def offset(kind, idx=0):
        return m.workspace_offset(B, _lib.TRAIN, kind, idx)

    def T(kind, idx=0, cols=Hp, dtype=st, rows=B):
        off = offset(kind, idx)
        assert off >= 0, (kind, idx)
        nb = rows * cols * torch.tensor([], dtype=dtype).element_size()
        return ws[off:off + nb].view(dtype).view(rows, cols)

    def V(kind, idx):   # fp32 [Hp] vector
        return T(kind, idx, cols=Hp, dtype=torch.float32, rows=1)[0]

    def bits(kind, idx):
        off = offset(kind, idx)
        assert off >= 0, (kind, idx)
        b = unpack_bits(ws[off:off + B * Hp // 8], B, Hp)
        assert not b[:, H:].any(), (kind, idx, "padded columns' bits")
        return b

    # ---- the masks the plan stores, and no others ------------------------
    for j in range(R):
        assert (offset("mask_a1", j) >= 0) == plan["masks"], ("mask_a1", j)
    assert offset("mask_h", 0) == -1, "mask_h[0]"
    for j in range(1, R):
        assert (offset("mask_h", j) >= 0) == plan["masks"], ("mask_h", j)
    assert (offset("mask_h", R) >= 0) == plan["rank1"], ("mask_h", R)

    f32 = torch.float32
    # the weights as packed: rounded to bf16, or the fp32 parameters themselves (in fp64)
    Wb = (lambda k: bf(sd0[k].float())) if is_bf else (lambda k: sd0[k].double())   # noqa: E731
    rd = lambda t: t.to(cd)                          # noqa: E731 (a stored tensor, for the references)
    chk = check_bf16 if is_bf else check_fp32
    pad = lambda w, r, cl: torch.nn.functional.pad(w, (0, cl - w.shape[1], 0, r - w.shape[0]))  # noqa: E731
    stats, rels = [], []
    rel = lambda name, got, ref, tol=REL: check_rel(name, got, ref, tol, rels)  # noqa: E731

    # ---- forward -------------------------------------------------------
    parts = [sd0["user_embedding.weight"][u], sd0["item_embedding.weight"][i]]
    parts += [sd0[f"cat_embeddings.{k}.weight"][c[:, k]] for k in range(K)]
    x0f = torch.cat(parts + [n], 1)
    x0p = rd(T("x0", cols=Dp))
    x0 = x0p[:, :D]
    assert torch.equal(x0, rd(bf(x0f) if is_bf else x0f)), "x0 gather"
    W0 = Wb("initial_deep_layer.weight")
    h = rd(T("h", 0))
    chk("h0", h[:, :H], x0 @ W0.T + sd0["initial_deep_layer.bias"], stats,
        x0.abs() @ W0.abs().T + sd0["initial_deep_layer.bias"].abs())
    keep = [dropout_mask_torch(seed_d, j, B, H, p, dev) for j in range(R)]
    inv_keep = float(np.float32(1.0 / (1.0 - p)))
    # block_plain's exact second rounding needs the kernels' own fp32 factor
    inv_keep_k = float(np.float32(1) / (np.float32(1) - np.float32(p))) if p > 0 else 1.0
    if not is_bf:   # one fp32 ulp is the bound here: the kernels' own factor in the forward too
        inv_keep = inv_keep_k
    hs = [h]
    for j in range(R):
        pre = f"res_blocks.{j}"
        for l, (tk, bi) in enumerate((("t1", 2 * j), ("t2", 2 * j + 1))):
            Xin = hs[j] if l == 0 else a1
            t = rd(T(tk, j))
            W = pad(Wb(f"{pre}.layer{l + 1}.weight"), Hp, Hp)
            b = pad(sd0[f"{pre}.layer{l + 1}.bias"][None], 1, Hp)[0]
            chk(f"{tk}[{j}]", t[:, :H], (Xin @ W.T + b)[:, :H], stats,
                (Xin.abs() @ W.abs().T + b.abs())[:, :H])
            t64 = t[:, :H].double()   # all B rows, the last partial tile's included
            mu = t64.mean(0)
            var = (t64 * t64).mean(0) - mu * mu
            rel(f"mean{bi}", V("bn_mean", bi)[:H], mu, 1e-5)
            rel(f"invstd{bi}", V("bn_invstd", bi)[:H], 1.0 / torch.sqrt(var + 1e-5), 1e-5)
            gam = sd0[f"{pre}.bn{l + 1}.weight"].float()
            rel(f"scale{bi}", V("bn_scale", bi)[:H], gam * V("bn_invstd", bi)[:H], 1e-6)
            sc, sh = V("bn_scale", bi), V("bn_shift", bi)
            if l == 0:
                a1 = rd(T("a1", j))
                ref = torch.clamp_min(t * sc + sh, 0)[:, :H] * keep[j].float() * inv_keep
                chk(f"a1[{j}]", a1[:, :H], ref, stats, ((t * sc).abs() + sh.abs())[:, :H] * inv_keep)
                if plan["masks"]:
                    assert torch.equal(bits("mask_a1", j)[:, :H], a1[:, :H] != 0), f"mask_a1[{j}]"
            else:
                hn = rd(T("h", j + 1))
                chk(f"h[{j + 1}]", hn[:, :H], torch.clamp_min(t * sc + sh + hs[j], 0)[:, :H],
                    stats, ((t * sc).abs() + sh.abs() + hs[j].abs())[:, :H])
                if plan["masks"] and (j + 1 < R or plan["rank1"]):
                    assert torch.equal(bits("mask_h", j + 1)[:, :H], hn[:, :H] > 0), f"mask_h[{j + 1}]"
                hs.append(hn)
    wf = sd0["final_linear.weight"][0].to(cd)
    zc = T("zc", cols=1, dtype=f32)[:, 0]
    rel("logits", logits, hs[R][:, :H] @ wf[:H] + zc + sd0["final_linear.bias"][0], 1e-5)
    # cross network in fp64 from the fp32 gathered rows: zc = x_L . w_f[H:]
    x = x0f.double()
    xs, ss = [], []
    for l in range(cfg["params"]["n_cross_layers"]):
        xs.append(x)
        wl = sd0[f"cross_network.{l}.w.weight"][0].double()
        s_ = x @ wl
        ss.append(s_)
        x = x + x * s_[:, None] + sd0[f"cross_network.{l}.b"].double()
    rel("zc", zc, x @ wf[H:].double(), 1e-5)
    # the cross backward's saved scalars: s_l, u_m = x_0 . w_m, u_f = x_0 . w_f[H:]
    Lc = cfg["params"]["n_cross_layers"]
    scs = T("sc", cols=2 * Lc + 1, dtype=f32)
    us = [x0f.double() @ sd0[f"cross_network.{q}.w.weight"][0].double() for q in range(Lc)]
    for l in range(Lc):
        rel(f"s[{l}]", scs[:, l], ss[l], 1e-5)
        rel(f"u[{l}]", scs[:, Lc + l], us[l], 1e-5)
    rel("u_f", scs[:, 2 * Lc], x0f.double() @ wf[H:].double(), 1e-5)

    # ---- backward ------------------------------------------------------
    def bn_back(dr, t, bi, gam_key):
        mu, inv = V("bn_mean", bi)[:H], V("bn_invstd", bi)[:H]
        xh = (t[:, :H] - mu) * inv
        s0 = dr[:, :H].double().sum(0)
        s1 = (dr[:, :H].double() * xh.double()).sum(0)
        a = sd0[gam_key].float() * inv
        k1 = (a.double() * s1 / B).to(cd)
        k2 = (a.double() * s0 / B).to(cd)
        scale = (a * dr[:, :H]).abs() + (k1 * xh).abs() + k2.abs()
        if not is_bf:
            # k1 and k2 are themselves sums over the B rows, which the kernels make
            # in fp32 per chunk: an error of a few fp32 roundings of a sum(|dr xh|) / B
            # and a sum(|dr|) / B, whatever is left of k1 and k2 after the signs
            # cancel (a column whose s1 nearly vanishes, an element with dr = 0).
            # Against a bf16 ulp that never shows; against ACC_EPS x (|k1 xh| + |k2|)
            # it does (measured: 1 - 2.5 roundings of these magnitudes, up to 2.6 x
            # the bound without them).  So the sums' terms enter the scale as the
            # terms they are, at ACC_EPS and at most B 2^-24 (the worst case of a
            # B-term fp32 sum, which is the smaller one for B < 64).
            A1 = a.double() * (dr[:, :H] * xh).abs().sum(0) / B
            A0 = a.double() * dr[:, :H].abs().sum(0) / B
            scale = scale + min(1.0, B * 2.0 ** -24 / ACC_EPS) * (A1 * xh.abs() + A0)
        return a * dr[:, :H] - k1 * xh - k2, s0, s1, scale

    def bn_back32(dr, t, bi, gam_key):
        """bn_back's stage with the two coefficient sums made in torch fp32 (its
        own order) instead of fp64: a second draw of the error any fp32
        summation of them carries, from the same stored inputs."""
        mu, inv = V("bn_mean", bi)[:H], V("bn_invstd", bi)[:H]
        xh = (t[:, :H].float() - mu) * inv
        d32 = dr[:, :H].float()
        a = sd0[gam_key].float() * inv
        return a * d32 - (a * (d32 * xh).sum(0) / B) * xh - a * d32.sum(0) / B

    def chk_dt(name, got, dr, t, bi, gam_key):
        ref, s0, s1, sc_ = bn_back(dr, t, bi, gam_key)
        fx = (bound_x or {}).get(name)
        if fx is None:
            chk(name, got[:, :H], ref, stats, sc_)
        else:
            assert is_bf, "bound_x: bf16 stages only"
            tol = tol_bf16(ref, sc_)
            fig = float(((bn_back32(dr, t, bi, gam_key) - ref.float()).abs() / tol).max())
            kern = float(((got[:, :H].float() - ref.float()).abs() / tol).max())
            print(f"  BOUND {name}: reference (fp32 sums) vs reference (fp64 sums) {fig:.3f} of the standard "
                  f"bound; the step {kern:.3f}; this case's bound {fx:.3f}")
            check_bf16(name, got[:, :H], ref, stats, sc_, factor=fx)
        return s0, s1

    du = rd(T("du", R - 1))
    ref = dz[:, None] * wf[:H] * (hs[R][:, :H] > 0).float()
    chk(f"du[{R - 1}]", du[:, :H], ref, stats, ref.abs())
    rel("dW_f[:H]", gd["final_linear.weight"][0, :H], hs[R][:, :H].double().T @ dz.double())
    for j in reversed(range(R)):
        pre = f"res_blocks.{j}"
        du = rd(T("du", j))
        dt2 = rd(T("dt2", j))
        s0, s1 = chk_dt(f"dt2[{j}]", dt2, du, rd(T("t2", j)), 2 * j + 1, f"{pre}.bn2.weight")
        rel(f"dbeta2[{j}]", gd[f"{pre}.bn2.bias"], s0)
        rel(f"dgamma2[{j}]", gd[f"{pre}.bn2.weight"], s1)
        a1 = rd(T("a1", j))
        rel(f"dW2[{j}]", gd[f"{pre}.layer2.weight"], dt2[:, :H].double().T @ a1[:, :H].double())
        assert gd[f"{pre}.layer2.bias"].abs().max() == 0
        W2 = pad(Wb(f"{pre}.layer2.weight"), Hp, Hp)
        da = rd(T("da", j))
        t1 = rd(T("t1", j))
        if plan["stats_epi"]:   # one rounding: the dX GEMM's epilogue masks its accumulator
            check_bf16(f"da[{j}]", da[:, :H], ((dt2 @ W2) * inv_keep * (a1 != 0).float())[:, :H], stats,
                       ((dt2.abs() @ W2.abs()) * inv_keep)[:, :H])
        else:   # two roundings; the ReLU sign from the fp32 fma of t1 (its sign is the exact sum's)
            pos = (t1.double() * V("bn_scale", 2 * j).double() + V("bn_shift", 2 * j).double()) > 0
            (check_da_plain if is_bf else check_da_fp32)(
                f"da[{j}]", da[:, :H], (dt2 @ W2)[:, :H], keep[j] & pos[:, :H], inv_keep_k,
                stats, (dt2.abs() @ W2.abs())[:, :H])
        dt1 = rd(T("dt1", j))
        s0, s1 = chk_dt(f"dt1[{j}]", dt1, da, t1, 2 * j, f"{pre}.bn1.weight")
        rel(f"dbeta1[{j}]", gd[f"{pre}.bn1.bias"], s0)
        rel(f"dgamma1[{j}]", gd[f"{pre}.bn1.weight"], s1)
        rel(f"dW1[{j}]", gd[f"{pre}.layer1.weight"], dt1[:, :H].double().T @ hs[j][:, :H].double())
        assert gd[f"{pre}.layer1.bias"].abs().max() == 0
        W1 = pad(Wb(f"{pre}.layer1.weight"), Hp, Hp)
        Gj = dt1 @ W1 + du
        Gs = (dt1.abs() @ W1.abs() + du.abs())[:, :H]
        if j > 0:   # (G is one buffer, overwritten per block on the plain path: checked for block 0)
            chk(f"du[{j - 1}]", rd(T("du", j - 1))[:, :H],
                (Gj * (hs[j] > 0).float())[:, :H], stats, Gs)
        else:
            G = rd(T("G"))
            chk("G", G[:, :H], Gj[:, :H], stats, Gs)
    rel("db0", gd["initial_deep_layer.bias"], G[:, :H].double().sum(0))
    rel("dW0", gd["initial_deep_layer.weight"], G[:, :H].double().T @ x0.double())
    Dq = (Dp + 31) // 32 * 32
    dx0 = T("dx0", cols=Dq, dtype=f32)[:, :D]
    rel("dx0", dx0, G[:, :H].double() @ W0.double())
    # cross backward (fp64 from the fp32 gathered rows).  The weight gradients'
    # x_0 part is summed over the STORED x0 (bf16 here, like dW0's): x_l enters
    # them as x_l + a_l (x0 - x0f), a_l = prod_{j<l} (1 + s_j)
    dxs = x0.double() - x0f.double()
    a_l = [torch.ones(B, dtype=torch.float64, device=dev)]
    for l in range(Lc):
        a_l.append(a_l[-1] * (1.0 + ss[l]))
    dx = dz.double()[:, None] * wf[H:].double()
    rel("dW_f[H:]", gd["final_linear.weight"][0, H:],
        (x + a_l[Lc][:, None] * dxs).T @ dz.double())
    rel("db_f", gd["final_linear.bias"], dz.double().sum().reshape(1))
    for l in reversed(range(cfg["params"]["n_cross_layers"])):
        xl, sl = xs[l], ss[l]
        wl = sd0[f"cross_network.{l}.w.weight"][0].double()
        rel(f"cross_b[{l}]", gd[f"cross_network.{l}.b"], dx.sum(0))
        gx = (dx * xl).sum(1)
        rel(f"cross_w[{l}]", gd[f"cross_network.{l}.w.weight"][0],
            (gx[:, None] * (xl + a_l[l][:, None] * dxs)).sum(0))
        dx = dx * (1.0 + sl)[:, None] + gx[:, None] * wl[None, :]
    # dx0_cross = sum_k xcoef[b][k] V_k, V = (w_0 .. w_{L-1}, w_f[H:])
    xco = T("xcoef", cols=Lc + 1, dtype=f32).double()
    Vs = [sd0[f"cross_network.{q}.w.weight"][0].double() for q in range(Lc)] + [wf[H:].double()]
    rel("dx0_cross", sum(xco[:, k:k + 1] * Vs[k][None] for k in range(Lc + 1)), dx)
    dxe = dx0.double() + dx
    off = 0
    tabs = [("user_embedding.weight", u), ("item_embedding.weight", i)]
    tabs += [(f"cat_embeddings.{k}.weight", c[:, k]) for k in range(K)]
    for name, idx in tabs:
        w = sd0[name].shape[1]
        ref = torch.zeros(sd0[name].shape, dtype=torch.float64, device=dev)
        ref.index_add_(0, idx, dxe[:, off:off + w])
        off += w
        rel(name, gd[name], ref)

    # ---- padded columns: exactly 0 in everything the step stored ----------
    if Dp != D:
        assert not x0p[:, D:].any(), "x0 padded columns"
    if Hp != H:
        for kind, idxs in (("h", range(R + 1)), ("t1", range(R)), ("t2", range(R)), ("a1", range(R)),
                           ("du", range(R)), ("dt2", range(R)), ("da", range(R)), ("dt1", range(R)),
                           ("G", range(1))):
            for j in idxs:
                tp = T(kind, j)[:, H:].float()
                assert not tp.any(), (kind, j, "padded columns", int((tp != 0).sum()))

    what = "fraction of elements off by a bf16 rounding flip" if is_bf else "max |diff| / bound"
    print(f"\n  stage, {what}, max |diff|")
    for name, fr, mx in stats:
        print(f"    {name:10s} {fr:.2e} {mx:.2e}")
    worst = max((q for q in rels if q[2] == REL), key=lambda q: q[1])
    print(f"  worst {'flip' if is_bf else '|diff|/bound'} {max(s[1] for s in stats):.2e}"
          f"  worst max|diff| {max(s[2] for s in stats):.2e}"
          f"  worst gradient rel {worst[1]:.2e} ({worst[0]})")
    return dict(logits=logits, loss=loss, grads=gd, stats=stats, rels=rels, plan=plan,
                plain_step=plain_step)
