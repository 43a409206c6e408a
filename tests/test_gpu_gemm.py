"""GPU parity of the bf16 MFMA GEMM family vs a plain fp32 torch reference on the same bf16-rounded inputs."""
import math

import pytest
import torch

from helpers import assert_close, gelu8_decode, gelu8_encode

pytestmark = pytest.mark.gpu


def _mk(shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).cuda()


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (394, 1152, 384), (1000, 200, 192), (128, 384, 1536), (77, 64, 72)])
def test_gemm_nt_bf16_and_f32(M, N, K):
    from protopformer_amd import ops
    a = _mk((M, K), 1.0, 1).bfloat16()
    b = _mk((N, K), 0.1, 2).bfloat16()
    bias = _mk((N,), 0.5, 3)
    ref = a.float() @ b.float().t() + bias
    out = ops.gemm(a, b, epi=ops.EPI_F32, bias=bias)
    assert_close(out, ref, rtol=1e-3, atol=1e-3, what="gemm f32")      # 1e-3 rel (north_star), K-term fp32 accumulation
    out16 = ops.gemm(a, b, epi=ops.EPI_BF16, bias=bias)
    assert_close(out16.float(), ref.bfloat16().float(), rtol=8e-3, atol=1e-3, what="gemm bf16 out")


@pytest.mark.parametrize("M,N,K,epi", [(24576, 512, 1024, "bf16"), (24600, 520, 768, "resid"), (24576, 512, 768, "gelu"), (25000, 512, 896, "dgelu")])
def test_gemm_long_contraction_forward_shapes(M, N, K, epi):
    """K >= 768 forward products (deit_base; no BASELINE configuration) through the dispatcher: edge tiles in m and n, odd K-tile counts, every
    fused epilogue, 10 bit-identical repeats.  Until round 6 these went to the 256x256 kernel (now scripts/gpu/experiments/gemm_nt256); the
    128x128 / 224x128 kernels serve them since."""
    from protopformer_amd import ops
    a = _mk((M, K), 0.5, 1).bfloat16(); b = _mk((N, K), 0.05, 2).bfloat16(); bias = _mk((N,), 0.1, 3)
    pre = a.float() @ b.float().t()
    if epi == "bf16":
        run = lambda: ops.gemm(a, b, epi=ops.EPI_BF16, bias=bias); ref = (pre + bias); tol = dict(rtol=8e-3, atol=2e-3)
    elif epi == "resid":
        res = _mk((M, N), 1.0, 4)
        run = lambda: ops.gemm(a, b, epi=ops.EPI_RESID, bias=bias, res=res); ref = res + pre + bias; tol = dict(rtol=1e-3, atol=2e-3)
    elif epi == "gelu":
        aux = torch.empty(M, N, dtype=torch.uint8, device="cuda")
        run = lambda: ops.gemm(a, b, epi=ops.EPI_GELU, bias=bias, aux_out=aux); ref = torch.nn.functional.gelu(pre + bias); tol = dict(rtol=8e-3, atol=2e-3)
    else:
        gp = gelu8_encode(0.5 + _mk((M, N), 0.3, 5))
        run = lambda: ops.gemm(a, b, epi=ops.EPI_DGELU, aux_in=gp); ref = pre * gelu8_decode(gp); tol = dict(rtol=1e-2, atol=3e-3)
    out = run()
    assert_close(out.float(), ref, what=f"long-K {epi}", **tol)
    for _ in range(10):
        assert torch.equal(out, run())


def test_gemm_transpose_detecting():
    """Asymmetric operands: an (m,n)-swapped write or a k-permutation mismatch between A and B cannot pass."""
    from protopformer_amd import ops
    M, N, K = 128, 128, 64
    a = torch.zeros(M, K); b = torch.zeros(N, K)
    for m in range(M):
        a[m, m % K] = 1.0 + (m % 7)
    for n in range(N):
        b[n, (3 * n + 1) % K] = 2.0 + (n % 5)
    ref = a @ b.t()
    out = ops.gemm(a.cuda().bfloat16(), b.cuda().bfloat16(), epi=ops.EPI_F32)
    assert torch.equal(out.cpu(), ref)


def test_gemm_gelu_sigmoid_resid():
    from protopformer_amd import ops
    M, N, K = 394, 768, 192
    a = _mk((M, K), 1.0, 1).bfloat16(); b = _mk((N, K), 0.1, 2).bfloat16(); bias = _mk((N,), 0.5, 3)
    pre = a.float() @ b.float().t() + bias
    h = torch.empty(M, N, dtype=torch.uint8, device="cuda")
    g = ops.gemm(a, b, epi=ops.EPI_GELU, bias=bias, aux_out=h)
    gp = 0.5 * (1 + torch.erf(pre / math.sqrt(2))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2 * math.pi)
    # 8-bit linear code of gelu' in [-0.13, 1.13]: half a step = 2.5e-3 (+ the polynomial erf of the kernel, 1e-6)
    assert_close(gelu8_decode(h), gp, rtol=0.0, atol=2.6e-3, what="gelu' saved for backward")
    assert_close(g.float(), torch.nn.functional.gelu(pre).bfloat16().float(), rtol=8e-3, atol=2e-3, what="gelu")
    s = ops.gemm(a, b, epi=ops.EPI_SIGMOID_F32, bias=bias)
    assert_close(s, torch.sigmoid(pre), rtol=1e-3, atol=1e-4, what="sigmoid")
    # residual epilogue with per-sample DropPath scale and LayerScale
    rows_per = 197
    res = _mk((M, N), 1.0, 4); rs = torch.tensor([0.0, 1.0 / 0.9], device="cuda"); cs = _mk((N,), 0.3, 5)
    raw = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    out = ops.gemm(a, b, epi=ops.EPI_RESID, bias=bias, res=res, rowscale=rs, rows_per_group=rows_per, colscale=cs, aux_out=raw)
    ridx = torch.arange(M, device="cuda") // rows_per
    ref = res + pre * cs * rs[ridx][:, None]
    assert_close(out, ref, rtol=1e-3, atol=2e-3, what="residual epilogue")
    assert_close(raw.float(), pre.bfloat16().float(), rtol=8e-3, atol=1e-3, what="raw branch output")


@pytest.mark.parametrize("M,N,K", [(394, 384, 1152), (300, 192, 576), (128, 1536, 384)])
def test_gemm_dgrad_nn(M, N, K):
    """dx[M,N] = dy[M,K] @ W[K,N]  (B stored [kc][n] -> trans_b)."""
    from protopformer_amd import ops
    dy = _mk((M, K), 1.0, 1).bfloat16(); w = _mk((K, N), 0.1, 2).bfloat16()
    ref = dy.float() @ w.float()
    out = ops.gemm(dy, w, trans_b=True, epi=ops.EPI_F32)
    assert_close(out, ref, rtol=1e-3, atol=2e-3, what="dgrad")
    gp = gelu8_encode(0.5 + _mk((M, N), 0.3, 3))            # gelu'(pre) as the EPI_GELU forward epilogue saves it: 8-bit codes
    out2 = ops.gemm(dy, w, trans_b=True, epi=ops.EPI_DGELU, aux_in=gp)
    assert_close(out2.float(), (ref * gelu8_decode(gp)).bfloat16().float(), rtol=1e-2, atol=3e-3, what="dgelu")


@pytest.mark.parametrize("R,N,K", [(1000, 384, 384), (50432 // 8, 1152, 384), (777 * 8, 192, 768)])
def test_gemm_wgrad_tn_atomic(R, N, K):
    """dW[N,K] += dy[R,N]^T @ x[R,K] with split contraction + fp32 atomics, fused bias grad (column sum of dy)."""
    from protopformer_amd import ops
    dy = _mk((R, N), 1.0, 1).bfloat16(); x = _mk((R, K), 1.0, 2).bfloat16()
    ref = dy.float().t() @ x.float()
    dw = torch.zeros(N, K, device="cuda"); db = torch.zeros(N, device="cuda")
    ops.gemm(dy, x, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=dw, colsum=db)
    scale = float(ref.abs().max())
    assert_close(dw, ref, rtol=1e-3, atol=1e-3 * scale, what="wgrad")
    assert_close(db, dy.float().sum(0), rtol=1e-3, atol=1e-3 * float(dy.float().sum(0).abs().max()), what="bias grad")
    # accumulates (+=) into existing contents
    ops.gemm(dy, x, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=dw)
    assert_close(dw, 2 * ref, rtol=1e-3, atol=2e-3 * scale, what="wgrad accumulate")


def test_gemm_wgrad_train_step_shapes():
    """The weight-gradient path at the train step's shapes (scripts/gpu/wgrad_check.py): fp32 reference agreement, bias-gradient column
    sums, bit-identical repeats."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "scripts", "gpu", "wgrad_check.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert all("repeatable True" in l for l in lines if l.startswith("dW")), r.stdout
    assert float(lines[-1].split()[-1]) < 1e-4, r.stdout


_G224_CHILD = r"""# (run in-process by test_gemm_224_row_tiles_nt with the library's test hook set)
import torch
from helpers import assert_close
from protopformer_amd import ops
def mk(shape, scale, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g) * scale
for (M, N, K) in [(50432, 384, 1536), (50432, 384, 384), (20992, 384, 1152), (5000, 256, 128), (2120, 392, 192), (229, 8, 64)]:
    a = mk((M, K), 0.5, 1).bfloat16(); b = mk((N, K), 0.1, 2).bfloat16()
    out = ops.gemm(a, b, epi=ops.EPI_BF16)
    ref = a.float() @ b.float().t()
    assert_close(out.float(), ref, rtol=8e-3, atol=2e-3 * float(ref.abs().max()), what=f"nt 224 {M}x{N}x{K}")
    for _ in range(3):
        assert torch.equal(out, ops.gemm(a, b, epi=ops.EPI_BF16))
# transpose-detecting: an asymmetric pattern, two row tiles, ragged n
for (M, N) in [(448, 128), (300, 136)]:
    a2 = torch.zeros(M, 64, device="cuda"); a2[:, 0] = torch.arange(M, device="cuda") % 17 - 8.0
    b2 = torch.zeros(N, 64, device="cuda"); b2[:, 0] = torch.arange(N, device="cuda") % 5 - 2.0
    o2 = ops.gemm(a2.bfloat16(), b2.bfloat16(), epi=ops.EPI_BF16).float()
    assert torch.equal(o2, (a2[:, :1] @ b2[:, :1].t())), (M, N)
print("G224 OK")
"""


def test_gemm_224_row_tiles_nt():
    """gemm224g_kernel (224 x 128 direct-to-LDS tiles: the input gradients with the transposed weight shadow), forced for EVERY legal shape
    through the library's test hook (ppf_gemm_test_force_g224): bf16 output vs an fp32 reference at the train step's shapes, edge tiles in
    m, ragged n (N = 392 / 136 / 8: the clamped B rows and the n < N store mask), a transpose-detecting pattern, bit-identical repeats.  The
    default cost model's choice for the step's shapes is covered below."""
    import os
    from protopformer_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _lib.call("ppf_gemm_test_force_g224", 1)
    try:
        import io, contextlib
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            exec(compile(_G224_CHILD, "<g224>", "exec"), {"__name__": "__g224__", "_ROOT": root})
        assert "G224 OK" in buf.getvalue(), buf.getvalue()[-1500:]
    finally:
        _lib.call("ppf_gemm_test_force_g224", 0)


@pytest.mark.parametrize("M,N,K", [(50432, 384, 1536), (50432, 384, 384)])
def test_gemm_224_default_dispatch(M, N, K):
    """Two N = 384 input-gradient shapes in-process under the default cost model (K = 1536 takes gemm224g_kernel, K = 384 the 128 x 128 tiles since round 5)."""
    from protopformer_amd import ops
    a = _mk((M, K), 0.5, 1).bfloat16(); b = _mk((N, K), 0.1, 2).bfloat16()
    out = ops.gemm(a, b, epi=ops.EPI_BF16)
    ref = a.float() @ b.float().t()
    assert_close(out.float(), ref, rtol=8e-3, atol=2e-3 * float(ref.abs().max()), what="nt 224")
    assert torch.equal(out, ops.gemm(a, b, epi=ops.EPI_BF16))


@pytest.mark.parametrize("n_out,n_in,rows", [(1536, 384, 8192), (1152, 384, 4160), (384, 1536, 8192), (1032, 392, 2120), (400, 1288, 1992), (768, 384, 4096)])
def test_gemm_wgrad_eight_wave_tiles(n_out, n_in, rows):
    """wgrad8_kernel (256 x 128 / 128 x 256 tiles, eight waves): dW += dy^T x with the ordered split-K reduce against an fp32 reference, ragged
    edge tiles on either side and in the contraction, bias-gradient column sums, accumulation into a non-zero C, bit-identical repeats."""
    from protopformer_amd import ops
    dy = _mk((rows, n_out), 0.5, 3).bfloat16(); x = _mk((rows, n_in), 0.5, 4).bfloat16()
    base = _mk((n_out, n_in), 1.0, 5)
    ref = base.double() + dy.double().t() @ x.double()
    ref_cs = dy.double().sum(0)

    def run():
        gw = base.clone(); gb = torch.zeros(n_out, device="cuda")
        ops.gemm(dy, x, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=gw, colsum=gb)
        return gw, gb

    gw, gb = run()
    assert_close(gw, ref, rtol=2e-3, atol=2e-4 * float(ref.abs().max()), what="dW (eight-wave tiles)")
    assert_close(gb, ref_cs, rtol=2e-3, atol=2e-4 * float(ref_cs.abs().max()), what="column sums of dy")
    for _ in range(3):
        g2, b2 = run()
        assert torch.equal(g2, gw) and torch.equal(b2, gb)
    # transpose-detecting pattern: dW[i][j] = i-pattern * j-pattern from a single contraction row
    d2 = torch.zeros(rows, n_out, device="cuda"); d2[7] = torch.arange(n_out, device="cuda") % 13 - 6.0
    x2 = torch.zeros(rows, n_in, device="cuda"); x2[7] = torch.arange(n_in, device="cuda") % 7 - 3.0
    o2 = torch.zeros(n_out, n_in, device="cuda")
    ops.gemm(d2.bfloat16(), x2.bfloat16(), trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=o2)
    assert torch.equal(o2, d2[7][:, None] * x2[7][None, :])


def test_gemm_wgrad_atomic_without_workspace():
    """EPI_ATOMIC with workspace=False: dW[192, 192] += dy[520, 192]^T x with x read at ldb = 5 * 192 (every fifth row of a [2600, 192] matrix)
    and the column sums of dy.  pick_splitk gives three K slices of 192 / 192 / 136 rows: real fp32 atomics from several slices, a ragged
    last slice, the strided operand.  (fp32 atomics are not ordered: no bit-identity here.)"""
    from protopformer_amd import ops
    R, N, K = 520, 192, 192
    dy = _mk((R, N), 1.0, 1).bfloat16(); xf = _mk((5 * R, K), 1.0, 2).bfloat16()
    ref = dy.float().t() @ xf[::5].float()
    ref_cs = dy.float().sum(0)
    dw = torch.zeros(N, K, device="cuda"); db = torch.zeros(N, device="cuda")
    ops.gemm(dy, xf, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=dw, colsum=db, ldb=5 * K, workspace=False)
    scale = float(ref.abs().max())
    assert_close(dw, ref, rtol=1e-3, atol=1e-3 * scale, what="wgrad (atomics)")
    assert_close(db, ref_cs, rtol=1e-3, atol=1e-3 * float(ref_cs.abs().max()), what="bias grad (atomics)")
    ops.gemm(dy, xf, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=dw, ldb=5 * K, workspace=False)
    assert_close(dw, 2 * ref, rtol=1e-3, atol=1e-3 * 2 * scale, what="wgrad accumulate (atomics)")
