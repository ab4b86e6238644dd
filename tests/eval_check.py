"""Stage-by-stage check of the eval forward, bf16 or fp32, on every scoring
path (csrc/step.hip make_plan, eval fields):

  T  the fused tower (csrc/tower.hip; DCNR_FLAG_FUSED_TOWER, or B >= 16384):
     x0 and zc are all it stores
  P  the default bf16 path (Plan::eval_epi with eval_headp): BN + ReLU
     (+ residual) in the gemm_ws epilogues, the last GEMM ends in the head
     partials (head_parts); h_0 .. h_{R-1} pass through two alternating buffers
  K  the kept path (DCNR_FLAG_KEEP_INTERMEDIATES): bn_eval_finalize stores every
     affine, the same epilogues store h_R too, row_dot + head_logits
  L  the `layers` path (fp32, or bf16 with Hp > 512): plain GEMMs into one t
     buffer, bn_finalize2, bn_relu_drop, bn_add_relu2 / bn_add_relu_head

tests/stage_check.py pins the train step from the tensors the step stores.
The eval forward stores next to nothing, so each block output is made
observable instead (rows are independent in eval, the kernels deterministic):

  prefix models  the model truncated to its first k blocks (same weights and
                 running statistics) computes the full model's h_k as its last
                 activation, k = 1 .. R.
  one-hot head   final_linear.weight[0, H:] = 0 and final_linear.bias = 0 make
                 zc exactly 0; final_linear.weight[0, :H] = e_c makes the
                 logit of row b exactly the bf16 h_k[b, c]: every path takes
                 the head dot over the bf16-rounded h_R with the fp32 w_f
                 (gemm_ws.hip HEAD epilogue, tower.hip head, row_dot), and
                 every other term of the dot is 0 * h.  H calls give h_k; the
                 weights are re-packed on every eval call, so the head weight
                 is overwritten in place between them.  The probe is validated
                 on the kept path, where the probed h_k must equal the stored
                 DCNR_WS_H[k] bit for bit.
  the tower's h0 has no ReLU, and the tower has no block-free form.  A
                 one-block model with bn2.weight = bn2.bias = 0 adds exactly 0
                 (tower_pack: sc = 0 * inv = 0, sh = fma(b, 0, 0 - rm * 0) = +0;
                 the epilogue's fma(acc, 0, +0) + h0 = h0), so h1 = relu(h0).
                 The negative half comes from a second one-block model with
                 the SAME initial layer: W1 = -I, W2 = I, b1 = b2 = 0, BN1 the
                 identity and BN2 a doubling (gamma = 1 / 2, beta = rm = 0,
                 rv = 1 - eps, so inv = fp32(1 / sqrt(1 +- 3e-8)) = 1 exactly in
                 every kernel's affine).  A dot product with one nonzero term
                 is exact, so a1 = relu(-h0) and h1 = relu(2 a1 + h0) = |h0|,
                 all exactly; h0 = relu(h0) where that is positive, else -|h0|.
                 Validated on the kept path: bit for bit the stored
                 DCNR_WS_H[0], the stored affines exactly (1, 0) and (2, 0).
                 (Negating W0 and b0 to read relu(-h0) is NOT exact: a GEMM's
                 fp32 sums are not symmetric in sign under cancellation.
                 Measured on the kept path at Dp = 584, the generic initial
                 GEMM: one element of 153600, a heavily cancelled sum, came out
                 3.9935e-06 with W0 and -4.0531e-06 with -W0.)

What a path stores itself is read, not probed (dcnr_workspace_offset with the
run's flags): x0 and zc everywhere; on P the prefix model's h_{k-1}; on K and
L its h_k and h_{k-1}, every BN scale and shift, and on L the last block's t2.

One block with a hidden a1 (a1 is never observable in eval).  X = the path's
own stored h_{k-1} in fp64, the weights rounded to bf16 (bf16 mode),
sc = gamma / sqrt(rv + eps), sh = beta - rm * sc in fp64, rnd = the storage
rounding:

  pre1 = (X W1^T + b1) sc1 + sh1      S1 = (|X| |W1|^T + |b1|) |sc1| + |sh1|
  a1 = rnd(relu(pre1)), a1_lo / a1_hi = rnd(relu(pre1 -/+ ACC_EPS S1))
  pre2 = (a1 W2^T + b2) sc2 + sh2 + X  S2 = the same with absolute values + |X|
  ext  = ((a1_hi - a1_lo) |W2|^T) |sc2|
  |got - relu(pre2)| <= BF16_ULPS ulp_bf16(relu(pre2)) + ACC_EPS S2 + ext
  fp32: one fp32 ulp in place of the bf16 one.

bf16: the share of elements with got != rnd(relu(pre2)) is capped by FLIP_FRAC.
(fp32 has no flip cap, as in stage_check: an fp32 sum of H terms equals the
rounded fp64 sum in a minority of elements whatever the kernel does; max
|diff| / bound is recorded instead.)

The L path rounds twice more: it stores t1 = rnd(X W1^T + b1) and
t2 = rnd(a1 W2^T + b2) in the t buffer before the row passes apply the affine
(the reference follows the path's stored points; the bound is the same).
There a1 = rnd(relu(rnd(lin1) sc1 + sh1)), with the interval from
rnd(lin1 -/+ ACC_EPS (|X| |W1|^T + |b1|)) pushed through the affine and widened
by ACC_EPS (|t1 sc1| + |sh1|); the stored t2 of the (prefix) model's last
block is checked against a1 W2^T + b2 with BF16_ULPS ulp + ACC_EPS x the summed
|terms| + (a1_hi - a1_lo) |W2|^T, and h_k from the stored t2, scale and shift
within one rounding (check_bf16 / check_fp32).

The other checks: x0 exact against the gathered rows (columns D..Dp-1 exactly
0); zc against the fp64 cross network at REL; stored BN scale within 2 fp32
ulp, shift within 2^-22 (|beta| + |rm sc|), padded entries 0; h0 from x0 by
check_bf16 / check_fp32; columns H..Hp-1 of every stored activation exactly 0;
the real head's logits per row within one fp32 ulp + ACC_EPS (sum |h_R w_f| +
|zc| + |b_f|) of h_R . w_f[:H] + zc + b_f from the path's own h_R and zc; a
second run bit-equal; the kernel classes the run launched (the library's launch
profiler).  The functions up to check_path take plain tensors
(tests/test_eval_check_cpu.py feeds them an emulated path and its faults).
"""
import torch

import golden_common as gc
from stage_check import (ACC_EPS, BF16_ULPS, FLIP_FRAC, REL, bf, check_bf16, check_fp32, check_rel,
                         ulp_bf16, ulp_fp32)

BN_EPS = 1e-5


# ---------------------------------------------------------------- references
def rnd(t, mode):
    """The storage rounding of ``mode``, result in fp64."""
    return (t.float().to(torch.bfloat16) if mode == "bf16" else t.float()).double()


def ulp(t, mode):
    return ulp_bf16(t.double()) if mode == "bf16" else ulp_fp32(t)


def packed(W, mode):
    """A deep-tower weight as the kernels read it (bf16 mode: rounded), fp64."""
    return bf(W.float()).double() if mode == "bf16" else W.double()


def affine_ref(g, be, rm, rv):
    sc = g.double() / torch.sqrt(rv.double() + BN_EPS)
    return sc, be.double() - rm.double() * sc


def block_ref(X, p, mode, t_stored=False):
    """References and bound terms of one residual block from its stored input
    X [B, H].  ``p``: W1 b1 g1 be1 rm1 rv1 W2 b2 g2 be2 rm2 rv2 (fp32, [H, H] /
    [H]).  ``t_stored``: the L path's two extra stored points.  Returns ref =
    relu(pre2) with S2 and ext, and lin2 = a1 W2^T + b2 with L2 and extl."""
    X = X.double()
    relu = lambda t: torch.clamp_min(t, 0)   # noqa: E731
    W1, W2 = packed(p["W1"], mode), packed(p["W2"], mode)
    b1, b2 = p["b1"].double(), p["b2"].double()
    sc1, sh1 = affine_ref(p["g1"], p["be1"], p["rm1"], p["rv1"])
    sc2, sh2 = affine_ref(p["g2"], p["be2"], p["rm2"], p["rv2"])
    lin1 = X @ W1.T + b1
    L1 = X.abs() @ W1.abs().T + b1.abs()
    if not t_stored:
        pre1 = lin1 * sc1 + sh1
        tol1 = ACC_EPS * (L1 * sc1.abs() + sh1.abs())
        lo, hi = pre1 - tol1, pre1 + tol1
    else:
        t1, ta, tb = rnd(lin1, mode), rnd(lin1 - ACC_EPS * L1, mode), rnd(lin1 + ACC_EPS * L1, mode)
        pre1 = t1 * sc1 + sh1
        ea, eb = ta * sc1 + sh1, tb * sc1 + sh1
        tol1 = ACC_EPS * (torch.maximum(ta.abs(), tb.abs()) * sc1.abs() + sh1.abs())
        lo, hi = torch.minimum(ea, eb) - tol1, torch.maximum(ea, eb) + tol1
    a1, a1_lo, a1_hi = rnd(relu(pre1), mode), rnd(relu(lo), mode), rnd(relu(hi), mode)
    lin2 = a1 @ W2.T + b2
    L2 = a1.abs() @ W2.abs().T + b2.abs()
    extl = (a1_hi - a1_lo) @ W2.abs().T
    pre2 = lin2 * sc2 + sh2 + X
    return dict(ref=relu(pre2), S2=L2 * sc2.abs() + sh2.abs() + X.abs(), ext=extl * sc2.abs(),
                lin2=lin2, L2=L2, extl=extl)


def check_bound(name, got, ref, scale, ext, mode, stats):
    """|got - ref| <= BF16_ULPS bf16 ulp (fp32: one fp32 ulp) of ref + ACC_EPS
    scale + ext; bf16: the flip cap.  Records (name, flip fraction or None,
    max |diff| / bound, max |diff|)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    d = (got - ref).abs()
    is_bf = mode == "bf16"
    tol = (BF16_ULPS if is_bf else 1) * ulp(ref, mode) + ACC_EPS * scale.double() + ext.double() + 1e-300
    bad = d > tol * (1.0001 if is_bf else 1.0)
    flips = float((got != rnd(ref, mode)).double().mean()) if is_bf else None
    stats.append((name, flips, float((d / tol).max()), float(d.max())))
    nb = int(bad.sum())
    assert nb == 0, (name, nb, float(d.max()), float((d / tol).max()), bad.nonzero()[:5].tolist(),
                     got[bad][:5].tolist(), ref[bad][:5].tolist())
    if is_bf:
        assert flips <= FLIP_FRAC, (name, flips)


def check_block(name, got, X, p, mode, stats):
    """h_k [B, H] of a path whose a1 is rounded once (T, P, K) from its h_{k-1}."""
    r = block_ref(X, p, mode)
    check_bound(name, got, r["ref"], r["S2"], r["ext"], mode, stats)


def check_block_t2(name, got, t2, sc2, sh2, X, p, mode, stats):
    """The L path: the stored t2 [B, H] from h_{k-1} across the hidden a1, then
    h_k from the stored t2 and the stored fp32 scale and shift, one rounding."""
    r = block_ref(X, p, mode, t_stored=True)
    check_bound(f"t2 of {name}", t2, r["lin2"], r["L2"], r["extl"], mode, stats)
    t2, X, sc2, sh2 = t2.double(), X.double(), sc2.double(), sh2.double()
    ref = torch.clamp_min(t2 * sc2 + sh2 + X, 0)
    check_bound(name, got, ref, (t2 * sc2).abs() + sh2.abs() + X.abs(), torch.zeros_like(ref), mode, stats)


def check_h0(name, got, x0, W0, b0, mode, stats):
    """check_bf16 / check_fp32 as they are; the record in check_bound's form."""
    x0 = x0.double()
    W = packed(W0, mode)
    ref = x0 @ W.T + b0.double()
    scale = x0.abs() @ W.abs().T + b0.double().abs()
    st = []
    if mode == "bf16":
        check_bf16(name, got, ref.float(), st, scale)
    else:
        check_fp32(name, got, ref, st, scale)
    d = (got.double() - ref).abs()
    tol = (BF16_ULPS * ulp_bf16(ref) if mode == "bf16" else ulp_fp32(ref)) + ACC_EPS * scale
    stats.append((name, st[0][1] if mode == "bf16" else None, float((d / tol).max()), float(d.max())))


def check_affine(name, sc, sh, p, which, H):
    """A stored running-stat affine [Hp] (fp32): scale within 2 fp32 ulp, shift
    within 2^-22 (|beta| + |rm sc|): three fp32 roundings; padded entries 0."""
    g, be, rm, rv = (p[k + which] for k in ("g", "be", "rm", "rv"))
    rsc, rsh = affine_ref(g, be, rm, rv)
    dsc = (sc[:H].double() - rsc).abs()
    assert (dsc <= 2 * ulp_fp32(rsc)).all(), (name, "scale", float((dsc / ulp_fp32(rsc)).max()))
    dsh = (sh[:H].double() - rsh).abs()
    tol = 2.0 ** -22 * (be.double().abs() + (rm.double() * rsc).abs())
    assert (dsh <= tol).all(), (name, "shift", float((dsh / tol.clamp_min(1e-300)).max()))
    assert not sc[H:].any() and not sh[H:].any(), (name, "padded entries")


def check_logits(name, z, hR, wf, zc, b_f, H, stats):
    """The real head per row, from the path's own h_R [B, H] and stored zc."""
    terms = hR.double() * wf[:H].double()
    ref = terms.sum(1) + zc.double() + b_f.double()
    tol = ulp_fp32(ref) + ACC_EPS * (terms.abs().sum(1) + zc.double().abs() + b_f.double().abs())
    d = (z.double() - ref).abs()
    assert torch.isfinite(z).all(), name
    stats.append((name, None, float((d / tol).max()), float(d.max())))
    bad = d > tol
    assert not bad.any(), (name, int(bad.sum()), float((d / tol).max()), bad.nonzero()[:5].tolist())


def check_x0(x0p, x0f, D, mode):
    """The stored x0 [B, Dp] against the gathered fp32 rows [B, D]: exact."""
    want = bf(x0f) if mode == "bf16" else x0f
    assert torch.equal(x0p[:, :D].float(), want), "x0 gather"
    assert not x0p[:, D:].any(), "x0 padded columns"


def zc_ref(x0f, cross_w, cross_b, wf_tail):
    """x_L . w_f[H:] of the cross network, fp64 from the fp32 gathered rows."""
    x = x0f.double()
    for w, b in zip(cross_w, cross_b):
        x = x + x * (x @ w.double())[:, None] + b.double()
    return x @ wf_tail.double()


def check_pad(name, t, H):
    tp = t[:, H:]
    assert not tp.any(), (name, "padded columns", int((tp != 0).sum()))


def check_path(obs, P, mode, stats=None):
    """Every check of one path's observables (plain tensors).

    P: H, D, W0, b0, blocks (block_ref's dicts), wf [H + D], bf [1], cross_w,
    cross_b.  obs: x0 [B, Dp] and x0f [B, D]; zc [B]; h0; blocks, per block a
    dict X (h_{k-1}), got (h_k) and, on the L path, t2, sc2, sh2; affine, the
    stored (scale, shift) pairs of the 2R layers or None; logits and hR.  A
    stored activation comes [B, Hp] (its padded columns are checked), a probed
    one [B, H]."""
    stats = [] if stats is None else stats
    H, D = P["H"], P["D"]
    cut = lambda t: t[:, :H]   # noqa: E731
    check_x0(obs["x0"], obs["x0f"], D, mode)
    check_rel("zc", obs["zc"], zc_ref(obs["x0f"], P["cross_w"], P["cross_b"], P["wf"][H:]), REL)
    if obs.get("affine") is not None:
        for i, (sc, sh) in enumerate(obs["affine"]):
            check_affine(f"bn{i % 2 + 1}[{i // 2}]", sc, sh, P["blocks"][i // 2], str(i % 2 + 1), H)
    check_pad("h0", obs["h0"], H)
    check_h0("h0", cut(obs["h0"]), obs["x0"][:, :D], P["W0"], P["b0"], mode, stats)
    for k, (o, p) in enumerate(zip(obs["blocks"], P["blocks"]), 1):
        for key in ("X", "got", "t2"):
            if o.get(key) is not None:
                check_pad(f"{key} of h[{k}]", o[key], H)
        if o.get("t2") is not None:
            check_block_t2(f"h[{k}]", cut(o["got"]), cut(o["t2"]), o["sc2"][:H], o["sh2"][:H], cut(o["X"]),
                           p, mode, stats)
        else:
            check_block(f"h[{k}]", cut(o["got"]), cut(o["X"]), p, mode, stats)
    check_logits("logits", obs["logits"], cut(obs["hR"]), P["wf"], obs["zc"], P["bf"], H, stats)
    return stats


# ------------------------------------------------------------ on the device
PATH_FLAGS = {"T": dict(keep=False, tower=True), "P": dict(keep=False, tower=False),
              "K": dict(keep=True, tower=False), "L": dict(keep=False, tower=False)}


def block_params(sd, j):
    pre = f"res_blocks.{j}"
    p = {}
    for l in ("1", "2"):
        p["W" + l], p["b" + l] = sd[f"{pre}.layer{l}.weight"], sd[f"{pre}.layer{l}.bias"]
        p["g" + l], p["be" + l] = sd[f"{pre}.bn{l}.weight"], sd[f"{pre}.bn{l}.bias"]
        p["rm" + l], p["rv" + l] = sd[f"{pre}.bn{l}.running_mean"], sd[f"{pre}.bn{l}.running_var"]
    return p


class EvalCase:
    """A model, its prefix models and one batch of inputs on the device."""

    def __init__(self, dev, cfg, B, seed, precision):
        import dcnr
        self.dev, self.cfg, self.B, self.mode = dev, cfg, B, precision
        self.R, self.H = cfg["params"]["n_res_blocks"], cfg["params"]["hidden_dim"]
        self.Hp = (self.H + 7) // 8 * 8
        torch.manual_seed(seed)
        full = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                               dict(cfg["params"]), precision=precision)
        gc.perturb_state(full, seed + 1)
        self.full = full.to(dev).eval()
        self.sd = {k: v.detach().clone() for k, v in self.full.state_dict().items()}
        self.D = self.full._dims["input_dim"]
        self.Dp = (self.D + 7) // 8 * 8
        self.st = torch.bfloat16 if precision == "bf16" else torch.float32
        g = torch.Generator(device=dev).manual_seed(seed - 2)
        cards = list(cfg["cat_dims"].values())
        self.u = torch.randint(0, cfg["n_users"], (B,), device=dev, generator=g)
        self.i = torch.randint(0, cfg["n_items"], (B,), device=dev, generator=g)
        self.c = torch.stack([torch.randint(0, n, (B,), device=dev, generator=g) for n in cards], 1)
        self.n = torch.rand((B, cfg["n_num"]), device=dev, generator=g)
        sd = self.sd
        parts = [sd["user_embedding.weight"][self.u], sd["item_embedding.weight"][self.i]]
        parts += [sd[f"cat_embeddings.{k}.weight"][self.c[:, k]] for k in range(len(cards))]
        self.x0f = torch.cat(parts + [self.n], 1)
        Lc = cfg["params"]["n_cross_layers"]
        self.P = dict(H=self.H, D=self.D, W0=sd["initial_deep_layer.weight"], b0=sd["initial_deep_layer.bias"],
                      blocks=[block_params(sd, j) for j in range(self.R)],
                      wf=sd["final_linear.weight"][0], bf=sd["final_linear.bias"],
                      cross_w=[sd[f"cross_network.{q}.w.weight"][0] for q in range(Lc)],
                      cross_b=[sd[f"cross_network.{q}.b"] for q in range(Lc)])
        self._prefix = {self.R: self.full}

    def prefix(self, k):
        """The model truncated to its first k blocks."""
        import dcnr
        if k not in self._prefix:
            cfg = self.cfg
            m = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                                dict(cfg["params"], n_res_blocks=k), precision=self.mode)
            m.load_state_dict({key: self.sd[key] for key in m.state_dict()})
            self._prefix[k] = m.to(self.dev).eval()
        return self._prefix[k]

    def run(self, m, path):
        """One eval forward of ``m`` on ``path``: (logits, workspace)."""
        from dcnr.model import run_forward
        m.keep_intermediates, m.fused_tower = PATH_FLAGS[path]["keep"], PATH_FLAGS[path]["tower"]
        z, ws = run_forward(m, False, 0, self.u, self.i, self.c, self.n)
        return z, ws

    def offset(self, m, kind, idx=0):
        from dcnr import _lib
        return m.workspace_offset(self.B, _lib.EVAL, kind, idx)

    def stored(self, m, ws, kind, idx=0, cols=None, dtype=None, rows=None):
        """A copy of a tensor the last run of ``m`` stored (the run's flags are the model's)."""
        cols = self.Hp if cols is None else cols
        dtype = self.st if dtype is None else dtype
        rows = self.B if rows is None else rows
        off = self.offset(m, kind, idx)
        assert off >= 0, (kind, idx)
        nb = rows * cols * torch.tensor([], dtype=dtype).element_size()
        return ws[off:off + nb].view(dtype).view(rows, cols).clone()

    def vec(self, m, ws, kind, idx):
        return self.stored(m, ws, kind, idx, dtype=torch.float32, rows=1)[0]

    def probe(self, m, path):
        """The last activation of ``m`` on ``path`` through H one-hot heads: [B, H]."""
        from dcnr.model import run_forward
        H, B = self.H, self.B
        wf, b_f = m.final_linear.weight, m.final_linear.bias
        saved = wf.detach().clone(), b_f.detach().clone()
        eye = torch.eye(H, device=self.dev)
        out = torch.empty(H, B, device=self.dev)
        m.keep_intermediates, m.fused_tower = PATH_FLAGS[path]["keep"], PATH_FLAGS[path]["tower"]
        ws = None
        with torch.no_grad():
            wf.zero_()
            b_f.zero_()
            for col in range(H):
                wf[0, :H].copy_(eye[col])
                z, ws = run_forward(m, False, 0, self.u, self.i, self.c, self.n, ws)
                out[col].copy_(z)
            wf.copy_(saved[0])
            b_f.copy_(saved[1])
        m.check_index_errors()
        h = out.T.contiguous()
        if self.mode == "bf16":
            assert torch.equal(h, bf(h)), "a probed value is not a bf16 number"
        return h

    def h0_models(self):
        """The two one-block models of the h0 device (module docstring): the
        block of the first adds exactly 0 (h1 = relu(h0)), the block of the
        second computes a1 = relu(-h0) and h1 = relu(2 a1 + h0) = |h0|."""
        import dcnr
        cfg, H = self.cfg, self.H
        out = []
        for second in (False, True):
            m = dcnr.DCN_RecSys(cfg["n_users"], cfg["n_items"], cfg["cat_dims"], cfg["n_num"],
                                dict(cfg["params"], n_res_blocks=1), precision=self.mode)
            sd = {key: self.sd[key].clone() for key in m.state_dict()}
            pre = "res_blocks.0."
            sd[pre + "bn2.weight"].zero_()
            sd[pre + "bn2.bias"].zero_()
            if second:
                eye = torch.eye(H, device=self.dev)
                sd[pre + "layer1.weight"].copy_(-eye)
                sd[pre + "layer2.weight"].copy_(eye)
                for l, gamma in (("1", 1.0), ("2", 2.0)):
                    sd[f"{pre}layer{l}.bias"].zero_()
                    sd[f"{pre}bn{l}.weight"].fill_(gamma)
                    sd[f"{pre}bn{l}.bias"].zero_()
                    sd[f"{pre}bn{l}.running_mean"].zero_()
                    sd[f"{pre}bn{l}.running_var"].fill_(1.0 - BN_EPS)   # inv = fp32(1 / sqrt(1 +- 3e-8)) = 1
            m.load_state_dict(sd)
            out.append(m.to(self.dev).eval())
        return out

    def probe_h0(self, path):
        """h0 of ``path``, exactly, from relu(h0) and |h0| (h0_models)."""
        ma, mb = self.h0_models()
        pos, mag = self.probe(ma, path), self.probe(mb, path)
        assert ((pos == 0) | (pos == mag)).all(), "relu(h0) is neither 0 nor |h0|"
        return torch.where(pos > 0, pos, -mag)

    def launches(self, m, path):
        """One run under the launch profiler: (logits, {class: launches})."""
        from dcnr import _lib
        _lib.profile_enable(True)
        _lib.profile_collect()
        try:
            z, _ = self.run(m, path)
            cnt = {k: v[1] for k, v in _lib.profile_collect().items()}
        finally:
            _lib.profile_enable(False)
        return z, cnt


def check_launches(path, cnt):
    """The kernel classes each plan launches (step.hip Fwd::tower, eval_epi,
    unfused_head, layers): the tower or not; head_parts is one head-class
    launch, row_dot + head_logits are two; only `layers` runs row passes."""
    assert cnt["tower"] == (1 if path == "T" else 0), (path, cnt)
    if path == "T":
        assert cnt["gemm_fwd"] == 0 and cnt["head"] == 0 and cnt["rowwise"] == 0, (path, cnt)
    elif path == "P":
        assert cnt["head"] == 1 and cnt["rowwise"] == 0 and cnt["reduce"] == 0, (path, cnt)
    elif path == "K":
        assert cnt["head"] == 2 and cnt["rowwise"] == 0 and cnt["reduce"] == 1, (path, cnt)
    else:
        assert cnt["rowwise"] > 0 and cnt["gemm_fwd"] > 0, (path, cnt)


def eval_check(dev, cfg, B, seed, precision, path):
    """Every eval check of one case on one path.  Returns a dict: ``stats``
    ((stage, flip fraction or None, max |diff| / bound, max |diff|) per checked
    stage), ``cross`` (max |h_R - the kept path's h_R| and the share of differing
    elements, T and P only) and ``second`` (second run bit-equal)."""
    ec = EvalCase(dev, cfg, B, seed, precision)
    R, H, Hp, D, Dp, m = ec.R, ec.H, ec.Hp, ec.D, ec.Dp, ec.full
    f32 = torch.float32

    # ---- the full model with its real head: logits twice, what the plan stores
    z, ws = ec.run(m, path)
    x0 = ec.stored(m, ws, "x0", cols=Dp)
    zc = ec.stored(m, ws, "zc", cols=1, dtype=f32)[:, 0]
    if path == "T":
        for j in range(R + 1):
            assert ec.offset(m, "h", j) == -1, ("h", j, "under the tower plan")
        for kind in ("t1", "t2", "bn_scale", "bn_shift"):
            assert ec.offset(m, kind, 0) == -1, (kind, "under the tower plan")
    z2, cnt = ec.launches(m, path)
    check_launches(path, cnt)
    second = torch.equal(z, z2)
    assert second, "second run differs"

    # ---- h0 and h_k, k = 1..R: stored where the path stores them, else probed
    obs = dict(x0=x0, x0f=ec.x0f, zc=zc, logits=z, affine=None, blocks=[])
    if path in ("K", "L"):
        obs["affine"] = [(ec.vec(m, ws, "bn_scale", i), ec.vec(m, ws, "bn_shift", i)) for i in range(2 * R)]
    if path == "T":
        obs["h0"] = ec.probe_h0("T")
    prev = obs.get("h0")
    for k in range(1, R + 1):
        mk = ec.prefix(k)
        _, wk = ec.run(mk, path)
        o = {}
        if path == "T":
            o["X"], o["got"] = prev, ec.probe(mk, "T")
        else:
            o["X"] = ec.stored(mk, wk, "h", k - 1)
            if k == 1:
                obs["h0"] = o["X"]
            if path == "P":
                o["got"] = ec.probe(mk, "P")
            else:
                o["got"] = ec.stored(mk, wk, "h", k)
            if path == "K":   # the probe's validation: bit for bit the stored h_k
                assert torch.equal(ec.probe(mk, "K"), o["got"][:, :H].float()), ("one-hot probe", k)
            if path == "L":
                o["t2"] = ec.stored(mk, wk, "t2", k - 1)
                o["sc2"], o["sh2"] = ec.vec(mk, wk, "bn_scale", 2 * k - 1), ec.vec(mk, wk, "bn_shift", 2 * k - 1)
        prev = o["got"]
        obs["blocks"].append(o)
    obs["hR"] = prev
    if path == "K":   # ... and the h0 device's: bit for bit the stored h0, its affines exactly (1, 0), (2, 0)
        assert torch.equal(ec.probe_h0("K"), obs["h0"][:, :H].float()), "h0 probe"
        mb = ec.h0_models()[1]
        _, wb = ec.run(mb, "K")
        for i, gamma in ((0, 1.0), (1, 2.0)):
            assert (ec.vec(mb, wb, "bn_scale", i)[:H] == gamma).all(), ("h0 probe: scale", i)
            assert not ec.vec(mb, wb, "bn_shift", i).any(), ("h0 probe: shift", i)
    stats = check_path(obs, ec.P, precision)

    # ---- against the kept path's h_R (recorded, not asserted)
    cross = None
    if path in ("T", "P"):
        _, wK = ec.run(m, "K")
        hK = ec.stored(m, wK, "h", R)[:, :H].float()
        dd = (prev[:, :H].float() - hK).abs()
        cross = (float(dd.max()), float((dd != 0).float().mean()))
    m.check_index_errors()
    return dict(stats=stats, cross=cross, second=second, input_dim=D)
