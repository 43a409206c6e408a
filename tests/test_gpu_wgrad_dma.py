"""The LDS-DMA data path of wgrad8_kernel against its register-staged path (test hook ppf_gemm_test_wgrad_path) and an fp64 reference, at the
smallest shapes where the path can go wrong: exact tiles, a ragged row tile (clamped source rows) with a K slice shorter than the ring is deep,
the 128 x 256 form, ragged on both sides, and a contraction that is no multiple of 64, which must fall back.  Only the way a K tile reaches
LDS differs between the paths, so their results are equal bit for bit."""
import pytest
import torch

from helpers import assert_close

pytestmark = pytest.mark.gpu

CASES = [(512, 384, 1024),       # <4,2>: exact tiles, 4 slices of 4 K tiles
         (1152, 384, 832),       # <4,2>: ragged fifth row tile; 13 K tiles in slices of 4/4/4/1
         (384, 1536, 1024),      # <2,4>
         (400, 1288, 960),       # <2,4>: ragged on both sides
         (1152, 384, 840)]       # K % 64 != 0: falls back to the register-staged kernel


def _mk(shape, scale, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).cuda()


@pytest.mark.parametrize("n_out,n_in,rows", CASES)
def test_wgrad_dma_matches_register_staged(n_out, n_in, rows):
    from protopformer_amd import _lib, ops
    dy = _mk((rows, n_out), 0.5, 3).bfloat16(); x = _mk((rows, n_in), 0.5, 4).bfloat16()
    base = _mk((n_out, n_in), 1.0, 5)                                  # a non-zero C
    ref = base.double() + dy.double().t() @ x.double()
    ref_cs = dy.double().sum(0)
    d2 = torch.zeros(rows, n_out, device="cuda"); d2[7] = torch.arange(n_out, device="cuda") % 13 - 6.0
    x2 = torch.zeros(rows, n_in, device="cuda"); x2[7] = torch.arange(n_in, device="cuda") % 7 - 3.0
    d2b, x2b = d2.bfloat16(), x2.bfloat16()

    def run():
        gw = base.clone(); gb = torch.zeros(n_out, device="cuda")
        ops.gemm(dy, x, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=gw, colsum=gb)
        return gw, gb

    try:
        _lib.call("ppf_gemm_test_wgrad_path", 1)
        gw1, gb1 = run()
        _lib.call("ppf_gemm_test_wgrad_path", 2)
        gw2, gb2 = run()
        assert torch.equal(gw2, gw1), f"dW differs between the paths: max |diff| {float((gw2 - gw1).abs().max()):.3e}"
        assert torch.equal(gb2, gb1), f"column sums differ between the paths: max |diff| {float((gb2 - gb1).abs().max()):.3e}"
        assert_close(gw2, ref, rtol=2e-3, atol=2e-4 * float(ref.abs().max()), what="dW (LDS-DMA path)")
        assert_close(gb2, ref_cs, rtol=2e-3, atol=2e-4 * float(ref_cs.abs().max()), what="column sums of dy (LDS-DMA path)")
        for _ in range(3):
            g3, b3 = run()
            assert torch.equal(g3, gw2) and torch.equal(b3, gb2)
        # transpose-detecting pattern: dW[i][j] = i-pattern * j-pattern from a single contraction row
        o2 = torch.zeros(n_out, n_in, device="cuda")
        ops.gemm(d2b, x2b, trans_a=True, trans_b=True, epi=ops.EPI_ATOMIC, out=o2)
        assert torch.equal(o2, d2[7][:, None] * x2[7][None, :])
    finally:
        _lib.call("ppf_gemm_test_wgrad_path", 0)


def test_wgrad_path_hook_rejects_other_values():
    from protopformer_amd import _lib
    with pytest.raises(RuntimeError, match="ppf_gemm_test_wgrad_path"):
        _lib.call("ppf_gemm_test_wgrad_path", 3)
    _lib.call("ppf_gemm_test_wgrad_path", 0)
