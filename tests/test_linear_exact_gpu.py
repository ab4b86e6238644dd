"""dcnr_linear_bf16 (the deep tower's forward GEMM entry point), bit for bit.

Operands.  X and W are integers in [-3, 3] stored as bf16, the bias integers
in [-64, 64] as fp32.  Then |X . W^T + b| <= 9 K + 64 < 2^24 for K <= 1024:
every partial sum is an integer below 2^24, so the fp32 accumulator is exact
in any order and ref = X.double() @ W.double().T + b is what every kernel
must produce: ref.float() under torch.equal with out_f32 = 1, and
ref.float().to(bfloat16), ONE round-to-nearest-even of an exact value, with
out_f32 = 0.  _expected asserts both claims (|ref| < 2^24, ref.float() == ref).

Buffers.  Padded leading dimensions (ldx = K + 8, ldw = K + 16, ldc = N + 8
unless a chunk case says otherwise).  The operands' padding columns and 8
guard rows after X and after W hold 4096.0 (exact in bf16): an element
wrongly accumulated with a non-zero partner moves the result by >= 4096, one
multiplied by a zeroed fragment does no harm.  C lies in a NaN-filled buffer,
64 guard elements before and after it; after the call everything outside the
M x N interior (guards and pad columns alike) must still be NaN and nothing
inside may be.  (NaN in operand padding is out of scope.)

(a) Tile edges: M = 1, 31, 32, 33, 63, 64, 65, 300 for every (K, N, out_f32) of

  K              N                   out_f32  kernel
  8, 72, 128     8, 264              0        gemm_ws, 4 K-tiles, BIAS epilogue
  136, 256       248, 256            0, 1     gemm_ws, 8 K-tiles, BIAS / F32
  264, 456, 512  256, 264, 512, 520  1        gemm_ws, 16 K-tiles, F32 epilogue
  264, 456, 512  256, 264, 512, 520  0        gemm_wsp
  520, 1024      128, 136            0, 1     generic tiled kernel (K > 512)
  64             20, 132             0, 1     generic tiled kernel (N % 8 != 0)

  Why: gemm_nn (csrc/step.hip) sends a bf16 call to gemm_ws when
  gemm_ws_supported(K, N) (csrc/gemm_ws.hip: K <= 512, K % 8 == 0, N % 8 == 0),
  with the epilogue NT_EPI_F32 for out_f32 and NT_EPI_BIAS otherwise; every
  other call goes to gemm (csrc/gemm.hip, gemm_kernel: 128 x 128 tiles).
  gemm_ws() hands the call to gemm_wsp when gemm_wsp_supported(epi, K, N)
  (csrc/gemm_wsp.hip: epi BIAS or BIAS_STATS, 256 < K <= 512), so a bf16 output
  at K > 256 takes gemm_wsp (32-row tiles, 256-column slices) and an fp32 one
  stays on gemm_ws; dispatch_ws picks the K-tile count: K <= 128 -> 4,
  K <= 256 -> 8, else 16.  gemm_ws tiles are 64 rows (BIAS, F32) x 256 columns,
  so N = 264 / 520 add a slice of 8 columns and N = 248 leaves one ragged.

(b) Launch chunks.  Both kernels address their operands with 32-bit buffer
offsets and cut a call into M-chunks of < 2^29 bytes per operand:

  launch_ws (csrc/gemm_ws.hip)
    maxld  = max(ldx, 2 * ldc, R ? ldr : 0, Hb ? 2 * ldhb : 0, T ? ldt : 0)
    mchunk = max(WS_TM, ((1 << 29) / (maxld * 2)) / WS_TM * WS_TM)
    (WS_TM = 64 for BIAS / F32 / BIAS_STATS, 32 otherwise; this entry point has
    no R, Hb or T)
  launch_wsp (csrc/gemm_wsp.hip)
    maxld  = max(ldx, ldc)
    mchunk = max(WP_TM, ((1 << 29) / (maxld * 2)) / WP_TM * WP_TM),  WP_TM = 32

  One huge leading dimension brings the cut down to 2048 rows:

  case     K, N, out       leading dimension             M
  ws_x     256, 264, bf16  ldx = 2^17                    2 * 2048 + 65: three chunks, the
                                                         last one 64-row tile + 1 row
  ws_c     512, 512, fp32  ldc = 2^16 (2 * ldc binds)    2048 + 65
  wsp_x    512, 512, bf16  ldx = 2^17                    2048 + 33 (a 32-row tile + 1 row)
  wsp_c    456, 512, bf16  ldc = 2^17                    2048 + 33

  The test computes the cut from the formulas above, asserts that M exceeds it
  and reports the first wrong row beside the cut.  The big buffer of a case
  is 0.55 - 1.1 GB; it is filled once and freed before the next case
  (measured on an MI355X: under 10 ms per case, printed; all 80 tests 3 s).
  Checked once by hand: with the second chunk's C pointer one row low in
  launch_ws and launch_wsp (a scratch build) all four cases fail from row
  cut - 1 = 2047 on, and every small case still passes.

(c) Rejected shapes: ldx % 8, ldw % 8 and K % 8 return a non-zero status and
leave C untouched, on the gemm_ws side (K <= 512) and on the generic side.
ldc % 8 != 0 with N % 8 == 0: gemm_ws / gemm_wsp store 16-byte row pieces and
reject it; the generic kernel stores element by element and takes it
(include/dcnr.h says so).  Either way: nothing written on a non-zero status,
the exact result on zero.
"""
import itertools
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 4096.0          # operand padding and guard rows: exact in bf16
GUARD_ROWS = 8
C_GUARD = 64          # NaN elements before and after C
MS = (1, 31, 32, 33, 63, 64, 65, 300)


def _operands(dev, M, K, N, ldx, ldw, seed):
    """X [M][ldx] and W [N][ldw] inside PAD-filled buffers with GUARD_ROWS
    rows after each, the bias, and the compact integer operands."""
    g = torch.Generator(device=dev).manual_seed(seed)
    Xi = torch.randint(-3, 4, (M, K), device=dev, generator=g).to(torch.bfloat16)
    Wi = torch.randint(-3, 4, (N, K), device=dev, generator=g).to(torch.bfloat16)
    b = torch.randint(-64, 65, (N,), device=dev, generator=g).float()
    Xb = torch.full((M + GUARD_ROWS, ldx), PAD, device=dev, dtype=torch.bfloat16)
    Xb[:M, :K] = Xi
    Wb = torch.full((N + GUARD_ROWS, ldw), PAD, device=dev, dtype=torch.bfloat16)
    Wb[:N, :K] = Wi
    return Xb, Wb, b, Xi, Wi


def _expected(Xi, Wi, b, out_f32):
    ref = Xi.double() @ Wi.double().T + b.double()
    assert float(ref.abs().max()) < 2 ** 24
    assert float(ref.abs().max()) <= 9 * Xi.shape[1] + 64
    assert torch.equal(ref.float().double(), ref)
    return ref.float() if out_f32 else ref.float().to(torch.bfloat16)


def _c_buffer(dev, M, ldc, out_f32):
    """A NaN-filled buffer of C_GUARD + M * ldc + C_GUARD elements and its
    [M][ldc] view, 16-byte aligned."""
    dt = torch.float32 if out_f32 else torch.bfloat16
    buf = torch.full((C_GUARD + M * ldc + C_GUARD,), float("nan"), device=dev, dtype=dt)
    rows = buf[C_GUARD:C_GUARD + M * ldc].view(M, ldc)
    assert rows.data_ptr() % 16 == 0
    return buf, rows


def _call(dev, Xb, ldx, M, K, Wb, ldw, N, b, rows, ldc, out_f32):
    from dcnr import _lib
    lib = _lib.load()
    st = lib.dcnr_linear_bf16(Xb.data_ptr(), ldx, M, K, Wb.data_ptr(), ldw, N, b.data_ptr(),
                              rows.data_ptr(), ldc, out_f32, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    return st


def _assert_exact(buf, rows, M, N, exp, what, cut=None):
    out = rows[:, :N]
    bad = (out != exp) | out.isnan()
    if bool(bad.any()):
        wrong = bad.any(1).nonzero()[:, 0]
        r = int(wrong[0])
        c = int(bad[r].nonzero()[0, 0])
        at = "" if cut is None else f" (launch cut at row {cut}; rows per chunk {cut})"
        raise AssertionError(f"{what}: {int(bad.sum())} wrong elements in {wrong.numel()} rows, first wrong row "
                             f"{r}{at}, column {c}: got {float(out[r, c])}, want {float(exp[r, c])}")
    assert torch.equal(out, exp), what
    # everything but the interior is still NaN: the guards and the pad columns
    n_nan = int(buf.isnan().sum())
    assert n_nan == buf.numel() - M * N, (what, "written outside C", buf.numel() - M * N - n_nan)


def _run_small(dev, K, N, out_f32):
    ldx, ldw, ldc = K + 8, K + 16, N + 8
    for M in MS:
        Xb, Wb, b, Xi, Wi = _operands(dev, M, K, N, ldx, ldw, 1000 * K + 10 * N + M)
        exp = _expected(Xi, Wi, b, out_f32)
        buf, rows = _c_buffer(dev, M, ldc, out_f32)
        st = _call(dev, Xb, ldx, M, K, Wb, ldw, N, b, rows, ldc, out_f32)
        assert st == 0, (M, K, N, st)
        _assert_exact(buf, rows, M, N, exp, f"M={M} K={K} N={N} out_f32={out_f32}")


def _cases(Ks, Ns, outs):
    return list(itertools.product(Ks, Ns, outs))


@pytest.mark.parametrize("K,N,out_f32", _cases((8, 72, 128), (8, 264), (0,)))
def test_ws_4_ktiles(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


@pytest.mark.parametrize("K,N,out_f32", _cases((136, 256), (248, 256), (0, 1)))
def test_ws_8_ktiles(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


@pytest.mark.parametrize("K,N,out_f32", _cases((264, 456, 512), (256, 264, 512, 520), (1,)))
def test_ws_16_ktiles_f32(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


@pytest.mark.parametrize("K,N,out_f32", _cases((264, 456, 512), (256, 264, 512, 520), (0,)))
def test_wsp(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


@pytest.mark.parametrize("K,N,out_f32", _cases((520, 1024), (128, 136), (0, 1)))
def test_generic_k_past_512(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


@pytest.mark.parametrize("K,N,out_f32", _cases((64,), (20, 132), (0, 1)))
def test_generic_n_not_multiple_of_8(dev, K, N, out_f32):
    _run_small(dev, K, N, out_f32)


# ---------------------------------------------------------------- launch chunks
def _cut_ws(ldx, ldc, tile_rows=64):
    maxld = max(ldx, 2 * ldc)   # no R, Hb, T on this entry point
    return max(tile_rows, ((1 << 29) // (maxld * 2)) // tile_rows * tile_rows)


def _cut_wsp(ldx, ldc):
    maxld = max(ldx, ldc)
    return max(32, ((1 << 29) // (maxld * 2)) // 32 * 32)


# id: (kernel, K, N, out_f32, ldx or None, ldc or None, M, chunks)
CHUNK_CASES = {
    "ws_x": ("ws", 256, 264, 0, 1 << 17, None, 2 * 2048 + 65, 3),
    "ws_c": ("ws", 512, 512, 1, None, 1 << 16, 2048 + 65, 2),
    "wsp_x": ("wsp", 512, 512, 0, 1 << 17, None, 2048 + 33, 2),
    "wsp_c": ("wsp", 456, 512, 0, None, 1 << 17, 2048 + 33, 2),
}


@pytest.mark.parametrize("case", list(CHUNK_CASES))
def test_launch_chunks(dev, case):
    kernel, K, N, out_f32, ldx, ldc, M, chunks = CHUNK_CASES[case]
    ldx = ldx or K + 8
    ldc = ldc or N + 8
    ldw = K + 16
    # the path the case is about (gemm_nn / gemm_ws dispatch, module docstring)
    assert K <= 512 and K % 8 == 0 and N % 8 == 0
    assert (kernel == "wsp") == (not out_f32 and K > 256)
    cut = _cut_wsp(ldx, ldc) if kernel == "wsp" else _cut_ws(ldx, ldc)
    assert cut == 2048 and M > cut and -(-M // cut) == chunks, (cut, M)
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    Xb, Wb, b, Xi, Wi = _operands(dev, M, K, N, ldx, ldw, 77 + K + N + M)
    exp = _expected(Xi, Wi, b, out_f32)
    buf, rows = _c_buffer(dev, M, ldc, out_f32)
    big = max(Xb.numel() * 2, buf.numel() * buf.element_size())
    assert 0.5e9 < big < 1.15e9, big
    st = _call(dev, Xb, ldx, M, K, Wb, ldw, N, b, rows, ldc, out_f32)
    assert st == 0, st
    try:
        _assert_exact(buf, rows, M, N, exp, case, cut)
    finally:
        del Xb, buf, rows
        torch.cuda.empty_cache()
    print(f"  {case}: {big / 1e9:.2f} GB, wall {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------- rejected shapes
def _run_status(dev, M, K, N, ldx, ldw, ldc, out_f32):
    """Calls with operands that are valid for the rounded-up shape, so that a
    call the library wrongly accepted would still stay inside its buffers."""
    Kb = (K + 7) // 8 * 8
    Xb, Wb, b, Xi, Wi = _operands(dev, M, Kb, N, max(ldx, Kb) + 8, max(ldw, Kb) + 8, 5 + K + N)
    buf, rows = _c_buffer(dev, M, max(ldc, N) + 8, out_f32)
    st = _call(dev, Xb, ldx, M, K, Wb, ldw, N, b, rows, ldc, out_f32)
    return st, buf, Xb, Wb, b


# (K, N): the gemm_ws side and the generic side (K > 512)
@pytest.mark.parametrize("K,N", [(64, 16), (264, 16), (520, 16)])
@pytest.mark.parametrize("what", ["ldx", "ldw", "K"])
@pytest.mark.parametrize("out_f32", [0, 1])
def test_rejected_shapes(dev, K, N, what, out_f32):
    M = 33
    ldx, ldw, ldc = K + 8, K + 16, N + 8
    if what == "ldx":
        ldx += 4
    elif what == "ldw":
        ldw += 4
    else:
        K += 4
    st, buf, *_ = _run_status(dev, M, K, N, ldx, ldw, ldc, out_f32)
    assert st != 0, (what, K, N)
    assert bool(buf.isnan().all()), (what, "C written by a rejected call")


@pytest.mark.parametrize("K,N", [(64, 16), (264, 16), (512, 264), (520, 16)])
@pytest.mark.parametrize("out_f32", [0, 1])
def test_ldc_not_multiple_of_8(dev, K, N, out_f32):
    M = 33
    ldx, ldw, ldc = K + 8, K + 16, N + 4
    Xb, Wb, b, Xi, Wi = _operands(dev, M, K, N, ldx, ldw, 9 + K + N)
    exp = _expected(Xi, Wi, b, out_f32)
    buf, rows = _c_buffer(dev, M, ldc, out_f32)
    st = _call(dev, Xb, ldx, M, K, Wb, ldw, N, b, rows, ldc, out_f32)
    # include/dcnr.h: rejected where the weight-stationary kernels would take the call
    assert (st != 0) == (K <= 512), (K, N, st)
    if st != 0:
        assert bool(buf.isnan().all()), "C written by a rejected call"
    else:
        _assert_exact(buf, rows, M, N, exp, f"ldc={ldc} K={K} N={N}")
