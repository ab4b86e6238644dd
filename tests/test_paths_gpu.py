"""One bf16 train step on each kernel path the train step can take, against
the fp64 oracle, at B = 300 (a ragged tile in every kernel).

The other bf16 train tests use hidden 96, 128, 384 and 512; which kernels a
step runs also changes at the shapes below:

  hidden  blocks  path
    40      1     no masks, plain GEMMs + row passes; one block, so the
                  weight-gradient pipe waits on its previous call
    64      1     BN statistics in the GEMM epilogues, no operand fold, the
                  single shared dt set
   384      2     the BN-backward row passes folded into the dX GEMMs; no
                  fused head pass; blocks 0 and 1 on the shared and second dt set
   512      3     fold, fused head pass (h_R rebuilt), rank-1 BN2 apply, a
                  fresh dt set for block 2
  1024      2     masks allocated, epilogues not applicable (K > 512)

Bounds are test_parity_gpu.py::test_bf16_mode_close's: logits relative norm
<= 1e-2, loss difference <= 1e-2, gradient norms within 5e-2 where the fp64
norm exceeds 1e-3.

Measured errors; these were measured on the commit before the host code's
path choices moved into one plan, not on the refactored code (which is
required to compute the same bits).  Every figure is under half its bound;
with the seed 300 the 512 case's logits were at 6.6e-3 and with 700 the 64
case's worst gradient norm at 3.9e-2, hence a seed per case.

  hidden  logits rel. norm  loss diff  worst gradient-norm rel. diff
    40       3.81e-4         3.1e-6     2.74e-3  (res_blocks.0.bn1.bias)
    64       4.79e-4         3.4e-5     1.21e-2  (res_blocks.0.bn1.bias)
   384       2.36e-3         2.2e-4     7.75e-3  (res_blocks.0.bn1.bias)
   512       3.54e-3         2.5e-4     1.39e-2  (res_blocks.1.bn1.bias)
  1024       2.76e-3         4.6e-5     5.95e-3  (res_blocks.0.bn2.weight)
"""
import numpy as np
import pytest
import torch

import dcnr_oracle as orc
import golden_common as gc
from helpers import np_state, our_model, spec_of, to_dev

pytestmark = pytest.mark.gpu

B = 300
# (hidden, n_res_blocks, seed of the weights and inputs)
PATHS = [(40, 1, 300), (64, 1, 300), (384, 2, 700), (512, 3, 700), (1024, 2, 700)]
# golden_common.CFG3R's tables and cross network (D = 456) around the tower under test
CFG = dict(n_users=4096, n_items=1024, cat_dims={f"c{i}": 1000 for i in range(12)}, n_num=8,
           params=dict(emb_dim=32, hidden_dim=0, n_cross_layers=3, n_res_blocks=0, dropout=0.0))


def cfg_of(hidden, n_res):
    return dict(CFG, params=dict(CFG["params"], hidden_dim=hidden, n_res_blocks=n_res))


def errors_vs_oracle(dev, cfg, seed):
    """(logits relative norm, loss difference, per-tensor gradient-norm
    relative differences where the fp64 norm exceeds 1e-3, their names) of one
    bf16 train step at B samples."""
    import dcnr
    m = our_model(cfg, precision="bf16", seed=seed)
    sd = np_state(m)
    u, i, c, n, y = gc.make_inputs(cfg, B, seed + 1)
    spec = spec_of(cfg)
    zr, cache = orc.forward(sd, spec, u, i, c, n, train=True)
    lr, dz = orc.bce_with_logits(zr, y)
    gr = orc.backward(sd, spec, cache, dz, u, i, c)

    m = m.to(dev).train()
    z = m(*to_dev(dev, u, i, c, n))
    loss = dcnr.BCEWithLogitsLoss()(z, to_dev(dev, y)[0])
    loss.backward()
    torch.cuda.synchronize()
    z = z.detach().cpu().double().numpy()
    names = [k for k, _ in m.named_parameters()]
    gn = np.array([np.linalg.norm(p.grad.detach().cpu().double().numpy()) for _, p in m.named_parameters()])
    gn64 = np.array([np.linalg.norm(gr[k]) for k in names])
    big = gn64 > 1e-3
    return (float(np.linalg.norm(z - zr) / np.linalg.norm(zr)), abs(float(loss.detach()) - lr),
            np.abs(gn[big] - gn64[big]) / gn64[big], [k for k, b in zip(names, big) if b])


@pytest.mark.parametrize("hidden,n_res,seed", PATHS)
def test_bf16_train_path_vs_oracle(dev, hidden, n_res, seed):
    e_z, e_l, e_g, names = errors_vs_oracle(dev, cfg_of(hidden, n_res), seed + hidden)
    print(f"hidden={hidden} n_res={n_res}: logits {e_z:.3e} loss {e_l:.3e} "
          f"gnorm max {e_g.max():.3e} ({names[int(e_g.argmax())]}, {len(names)} tensors)")
    assert e_z <= 1e-2
    assert e_l <= 1e-2
    assert len(names) > 0 and e_g.max() <= 5e-2
