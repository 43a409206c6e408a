"""Every kernel instantiation behind the six CaiT entry points of csrc/cait.hip against an fp64 reference, at the smallest shapes that
reach it, called through the C ABI (paddings, null pointers and refusals cannot be expressed through ops).  B = 2 unless stated (the sample
offset and the per-sample partial row are exercised), D = H hd.

Routes, how they are reached, and what is gated there:
  ppf_th_fwd          th_fwd_kernel<hd, H>, (hd, H) in {32, 48, 64} x {2, 4}: N = 1, 15, 16, 17, 32, 33 (one wave edge, one and two 32-key trips),
                      112, 113 (one and two workgroups per sample), 196, 208, 224, clipped to the pair's cover, plus the cover's largest N
                      (158 at (64, 4), 211 at (48, 4)); with out (NP = N up to 4, NPK = N up to 8, the product's paddings) and without (K image
                      only; the widest paddings the entry accepts, NP = NPK = 32 ceil(N / 32)): rowmax, zinv, a16 and hm over columns < N, every
                      pad column of a16 and hm exactly 0, out
  ppf_th_bwd          th_bwd_kernel<hd, H> at the same shapes on rowmax = fp32(m), zinv = fp32(1 / Z) of the REFERENCE: ds16 (NPK = N up to 8,
                      and once more at NPK = 16 ceil(N / 16): same columns < N bit for bit, pad columns exactly 0), every partial row
  ppf_th_param_reduce on that partial into prefilled dww, dbw, dbl, dwl: prefill + total; B = 3 at N = 113 (six partial rows) and N = 100 (three)
  ppf_th_grads        th_grads_kernel<hd> alone on random bf16 ds16 / a16 / qkv / dout: hd in {32, 48, 64} x H in {2, 4}, (hd, H) = (48, 1) and
                      (32, 3), N = 1, 16, 17, 31, 32, 33, 128, 129 (the second key block of a wave), 196, 208; pad columns of ds16 / a16 zero and
                      0.75: the two dqkv bit-identical; every column of the B N rows written
  the chain           th_fwd -> th_bwd -> th_grads -> th_param_reduce on the kernels' own statistics, a16 and ds16, per (hd, H) at N = 17 and at the
                      largest N <= 208 of the cover: dqkv and the four parameter gradients against fp64 autograd
  class attention     ppf_class_attn_fwd / _bwd: H in 1..4 x hd in {2, 32, 48, 64} x N1 in {1, 63, 64, 65, 197, 256}, with a policy that differs between
                      the samples and with none: attn, zinv, rowmean, out; dq, dk, dv on fp32(attn), fp32(zinv) of the reference and once more on
                      the forward kernel's own
  input families      (hd, H, N) = (48, 4, 196) (64, 2, 45) (32, 4, 100) through th_fwd, th_bwd and th_param_reduce: bw = 0.5 (A at a padded key must
                      be 0, not bw); Wl with dominant negative off-diagonals (the mixed maximum on a key that is no head's maximum, asserted on
                      the reference); bl = +-80 (loads the u (|S'| + max|S'|) term); peaked rows (one key >= 30 above the rest in every mixed head,
                      zinv ~ 1, asserted); Ww negative (A and the head mean negative, asserted).  Class attention at (hd, H, N1) = (48, 4, 197)
                      (64, 2, 45) (32, 3, 100): policy all zero (attn = 1 / N1 in closed form on the reference), the maximum on a masked key >= 30
                      above the kept ones, all scores negative
  refusals            test_cait_refusals: every case is stopped by a PPF_CHECK_ARG read in the source; code, error string naming the entry point,
                      all outputs still all-sentinel; the host predicates at 158 / 159, 211 / 212, 224 / 225, 208 / 209

Poison and sentinels, every call: bf16 inputs carry 32 rows of NaN behind the last sample, fp32 inputs (weights, statistics, partial) 16 NaN;
every output carries 16 more rows / elements of a sentinel bit pattern that must survive bit for bit; outputs are prefilled with the sentinel
and none may be left inside; everything inside is finite.  Every call runs twice: bit-identical (ppf_th_param_reduce included).

Reference: fp64 torch on the device from the exactly representable bf16 q / k / v / dout and the fp32 weights: S_h = scale q_h k_h^T,
S'_g = sum_h Wl[g,h] S_h + bl[g], m = max_j S', e = exp(S' - m), Z = sum_j e, P = e / Z, A_g = sum_h Ww[g,h] P_h + bw[g] (not rounded),
hm = mean_g A, O = A V, rowmax = m, zinv = 1 / Z.  Checked once per problem against the inner formula of
oracle.ppf_oracle.cait_talking_heads_attention (its einsum / softmax lines in fp64).  Backward: fp64 autograd of that formula; the explicit
chain dA = dO V^T, dP_h = sum_g Ww[g,h] dA_g, dot_h = sum_j dP_h P_h, dS'_h = P_h (dP_h - dot_h), dS_h = sum_g Wl[g,h] dS'_g that the bounds are
made of is asserted equal to it.  Class attention: S = scale q k^T, m = max_j S over all keys, e = exp(S - m) keep, Z = sum_j e,
attn = (e + eps / N1) / (Z + eps), checked against oracle.policy_softmax(..., self_keep=False) in fp64; backward: fp64 autograd, the maximum
included.

Gates, u = 2**-24, every scale from the fp64 reference:
  S_h        bf16 x bf16 products are exact in fp32, the additions round: a_s = scale (hd + 8) u |q| |k|^T (any order)
  S'_g       H products Wl[g,h] S_h -- scale = 1 / sqrtf(hd) (2 u), wl * scale rounded once in the forward, wl * (s * scale) in the backward (2 u
             either way) -- summed with bl in H + 1 additions (fused or not): a_sp = |Wl| a_s + (H + 6) u (|Wl| |S| + |bl|)
  rowmax     the largest computed logit lies between m - a_sp (at the arg max) and max_j (S' + a_sp): a_m = max_j (S' + a_sp) - m
  e          pass 2 forms exp2(a log2e - m log2e), pass 1 exp2((a - mt) log2e) against the lane's running maximum mt, |mt| <= R = max_j |S'|:
             relative r_e = a_sp + a_m + 6 u (|S'| + R) + r_exp (three roundings of the evaluation and the constant's, each <= u (|S'| + R)).
             The project has no figure for v_exp_f32, __expf or the reciprocal: r_exp, r_rcp = 4 x the worst error of a plain fp32 torch
             evaluation of the same expression (exp2(S'32 log2e - m32 log2e) where e > 2**-100, exp(S32 - m32) for class attention; 1 / Z32)
             against fp64 on the same inputs -- reference against reference, reported as exp_ref_u, rcp_ref_u
  zinv       Z is summed in-lane over the lane's keys with a rescale by exp2((m_old - m_new) log2e) per 32-key trip, then two shuffle levels
             with one more rescale each: (NT2 + 2) rescales of relative error r_exp + 3 u spread, spread = max_j S' - min_j S'.  The sum
             itself in the n_big form of the attention file (terms below u Z / N**2 are small; n_big the others, counted on the reference
             at half the threshold): a_Z = sum_j e r_e + (n_big + 1) u Z + (NT2 + 2) (r_exp + 3 u spread) Z; r_z = a_Z / Z + 2 u + r_rcp
  P          e zinv: a_P = P (r_e + r_z + u) + 2**-126 zinv (an fp32 exp2 returns nothing below the smallest normal number); in the backward
             on the reference's statistics r_z is replaced by the u of fp32(zinv)
  A          H products and H additions on P plus bw: a_A = |Ww| a_P + (H + 2) u (|Ww| P + |bw|); a16 is the exact bf16 interval
             bf16_rne(A - a_A) <= a16 <= bf16_rne(A + a_A); hm = mean_g A in fp32: a_hm = mean_g a_A + (H + 4) u mean_g |A|
  out        A enters the product rounded to bf16 (half a bf16 ulp of the term, h(x) = half_ulp_bf16(|A| + a_A)), accumulates over N keys in
             fp32 and is stored as bf16: a_O = (a_A + h + (N + 8) u |A|) |V|, the exact interval, no rtol
  ds16       dA: exact products accumulated in fp32 over hd, a_dA = (hd + 8) u |dO| |V|^T; dP: a_dP = |Ww|^T a_dA + (H + 2) u |Ww|^T |dA|;
             dot_h is summed in-lane over 4 ceil(N / 16) terms and two shuffles: a_dot = sum_j (a_dP P + (|dP| + a_dP) a_P) + (4 NT + 4) u
             sum_j |dP| P; dS' = P (dP - dot): a_dS' = a_P (|dP - dot| + a_dP + a_dot) + P (a_dP + a_dot) + 3 u |dS'|;
             a_dS = |Wl|^T a_dS' + (H + 2) u |Wl|^T |dS'|; the bf16 store is the exact interval, pad columns exactly 0
  partial    one row per workgroup: the terms dA_g P_h (dWw), dA_g (dbw), dS'_h (dbl), dS'_g S_h (dWl; S_h = s scale: a_S = a_s + 3 u |S|)
             of the workgroup's 112 queries x N keys, summed in the tree the kernel has: in-lane over 4 NT terms, a 6-level wave reduction,
             7 waves in order: depth = 4 NT + 13; a_partial = sum a_term + (depth + 4) u sum |term| (4: the products inside a term).  dbl is
             zero in exact arithmetic and is gated absolutely by this bound on sum |dS'|.  (The any-order bound N**2 u would pass a
             missing tile: at N = 196 the depth is 65, not 21 952.)
  reduce     th_param_reduce: at most 256 partial rows, one per thread (asserted), an 8-level tree, one accumulate into the prefill:
             against the fp64 sum of the kernel's own partial rows 10 u (sum |partial| + |prefill|); against the reference that plus the
             partial rows' bounds
  th_grads   operands exact bf16, fp32 accumulation over n = N: a_dV = (N + 8) u |a|^T |dO|; dQ, dK one multiplication by scale more:
             scale (N + 8) u |ds| |K| + 3 u |dQ|; bf16 stores: the exact interval.  In the chain the operands are the kernels' ds16 / a16:
             a_dQ = scale (a_dS + h(dS) + (N + 8) u |dS|) |K| + 3 u |dQ|, dK the same with dS^T and |Q|, a_dV = (a_A + h(A) + (N + 8) u |A|)^T |dO|
             with a_dS, a_A on the forward kernel's statistics (r_z kept in a_P) -- widened by the forward's own bound and nothing else
  class attn scores (hd + 8) u scale |q| |k| + 3 u |S|; e, Z, zinv as above without rescales (a wave sum of four in-lane terms), eps in Z + eps
             and c = eps / N1 two roundings each: a_attn = attn (r_z + 2 u) + zinv (e r_e + 3 u c + 2**-126); rowmean: mean_g a_attn + (H + 2) u
             mean_g attn; out accumulates fp32 probabilities over N1 keys: a_O = (a_attn + (N1 + 8) u attn) |V|, bf16 interval.  Backward on
             attn / zinv with input error a_in (u attn, u zinv for the reference's; a_attn, r_z zinv for the kernel's): g = dO V^T (hd + 8) u;
             dot = sum_j g attn: a_dot = sum_j (a_g attn + |g| a_in) + 12 u sum_j |g| attn; pt = attn - c zinv: a_pt = a_in + c zinv (4 u + r_zin)
             + u attn; dS = pt (g - dot): a_dS = a_pt (|g - dot| + a_g + a_dot) + pt (a_g + a_dot) + 3 u |dS| + |dL/dm| on the keys that tie for the
             maximum (the kernel holds m constant; autograd sends dL/dm = zinv sum_j g (attn Z - e) = zinv**2 sum_j g (c Z - eps e) there, evaluated in
             the second form, which has no cancellation, + 2**-40 zinv sum_j |g - dot| e for autograd's own fp64 rounding); ds = scale dS (+ 3 u);
             dk = ds q and dv = attn dO are single products (+ u), dq = sum_j ds k accumulates N1 fp32 terms; bf16 intervals
  zero bounds where a bound is exactly zero the error must be zero (frac()).
No gate is set from the output of a kernel under test.

Measured maxima on an MI355X (helpers.report: *_frac = the worst error as a fraction of its gate -- for bf16 outputs the part beyond half a
bf16 ulp as a fraction of the allowance):
  ppf_th_fwd          rowmax 0.055   zinv 0.012   a16 0.050   hm 0.078   out 0.949 (N = 1: the single term A = Ww row sum + bw IS the operand's bf16
                      rounding; 0.44 at N = 196)
  ppf_th_bwd          ds16 0.0053   partial 0.0090 (N = 1; 0.00024 at N = 196)   reduce against its input 0.142, against the reference 0.0063
  ppf_th_grads alone  dq 0.013   dk 0.0060   dv 0.0063 (the any-order (N + 8) u bound against an MFMA accumulation: every error is the bf16 store's)
  the chain           out 0.636   ds16 0.0014   partial 0.0012   dq 0.649   dk 0.691   dv 0.667 (all at N = 17: one bf16 operand rounding per few terms)
  families            bw = 0.5: hm 0.14, a16 0.018, out 0.40; Wl negative: rowmax 0.035, out 0.49, ds16 0.0020; bl = +-80: rowmax 0.24, zinv 0.025,
                      ds16 0.021; peaked: zinv exact, out 0.34, ds16 0.99 (keys whose e lies just under 2**-126: the kernel's exp2 returns 0 there
                      and the bound is that flush, nothing to spare and nothing missing; 0.0029 on the partial rows); Ww negative: as random
  class attention     attn 0.039   zinv 0.055   rowmean 0.039   out 0.0026   dq 0.994 (hd = 2, N1 = 64)   dk 0.998   dv 0.72; families: attn 0.058,
                      zero policy dq 3e-6.  dk 0.998 is the masked key that holds the maximum: the kernel's dk there is 0, autograd's is dL/dm q,
                      the allowance is |dL/dm| |q| and the fraction 1 - 2**-9 is the half ulp that `beyond` takes off
  reference against reference: exp2 <= 14 u on the random family, 213 u at bl = +-80 and 160 u on peaked rows (the argument's own rounding, |x| u);
  exp (class attention) <= 26 u, 81 u where all scores are near -64 scale; reciprocal <= 2.2 u
The whole file runs in 9.0 s (442 tests; the slowest two are the first, 1.2 s and 1.7 s with the library load and the first fp64 launches; every
other test <= 0.06 s).  (The dbl gate follows from the worst-case r_e and is 0.04 .. 0.13 per partial row at (48, 4, 196) on sum |dS'| of 400 .. 850:
test_gpu_cait.py's 1e-3 max |dWl| on the total stays the tighter check of dbl alone.)

The gates bite: value-only edits of cait.hip (a scratch build, nothing committed; no address, bound or launch geometry changes), each run
against this file and against test_gpu_cait.py as it stands (6 tests).
fail here, pass there:
   7. class-attention backward with pt = a instead of a - c zinv        -> 165 tests: 156 of test_class_attn (all but N1 = 1), all 9 families
   9. a16 stored with bw in its pad columns (the A.V operand untouched) -> 79 tests: test_th_kernels fwd at every N but 32 and 224 (54: the call without
                                                                          out pads to 32), all 18 families, the chains at N = 17 and (64, 4) N = 158
  10. zinv multiplied by 1 + 2**-10 in th_fwd                           -> 93 tests: every fwd and chain, 17 families (peaked (48, 4, 196) passes: r_z
                                                                          is 1e-3 there, nine rescales x 4 x the 160 u of exp2 at arguments near -100)
  14. the head mean multiplied by 1 + 2**-12                            -> 94 tests: every fwd (64), every family (18), every chain (12)
  15. m2 of head 1 shifted by 1e-3 (P_1 scaled by 2**-0.001)            -> 88 tests: 63 fwd, 12 chains, 13 families (not the peaked ones, where P is
                                                                          0 or 1, and bl = +-80 at N = 196 / 100, where r_e carries 4 x 213 u)
fail in both files, so they do not count as evidence for this one (failures here / there):
   1. bw added at padded keys (`a = valid ? a : 0` removed)             84 / 5      2. m2 of head 1 taken from m without * LOG2E           94 / 4
   3. dot[h] without its second shuffle                                 90 / 4      4. dbl accumulating pr instead of dsp                  96 / 1
   5. th_grads scaling dV by scale                                      92 / 3      6. th_grads image rows past N filled with 1.0, not 0   76 / 4
   8. the head mean divided by H + 1                                    94 / 2     11. dot[h] multiplied by 1 + 2**-9                       96 / 1
  13. th_grads dV multiplied by 1 + 2**-8                               86 / 1
      (6: the finite-pad comparison of test_th_grads_alone fails at the 64 cases with N % 16 != 0, and the chain; the tile rows past N repeat
      the last row and meet the filled Q / dO rows, which the old file sees too.  4 and 11 fail there through its dbl check alone.)
passes both: 12. dbl accumulating dsp + 1e-7 pr (1.1e-5 per partial row: a tenth of a percent of the dbl gate above)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import SENT, U, bf16_rne, bits, half_ulp_bf16, report

pytestmark = pytest.mark.gpu

ERR_SHAPE, ERR_ARG = -1, -3
PAD, POISON = 16, 32                     # sentinel rows / elements behind every output, NaN rows behind every bf16 input
EPS = 1e-6                               # SOFTMAX_EPS
FLUSH = 2.0 ** -126
LOG2E32 = float(np.float32(1.44269504088896340736))
TH_WAVES, LDS_BYTES = 7, 160 * 1024
PAIRS = [(hd, H) for hd in (32, 48, 64) for H in (2, 4)]
FAMILY_SHAPES = [(48, 4, 196), (64, 2, 45), (32, 4, 100)]


def pw_of(H):
    return 2 * H * H + 2 * H


def cover(hd, H):
    """Largest N ppf_th_fused_supported documents for the pair (K and V images of all heads + the reduction rows in 160 KiB, N <= 224);
    test_cait_refusals holds the library's predicate to it."""
    return min(224, (LDS_BYTES - TH_WAVES * pw_of(H) * 4) // (2 * H * hd * 2))


def groups(N):
    return ((N + 15) // 16 + TH_WAVES - 1) // TH_WAVES


def ceil_to(n, m):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ plumbing
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def frac(err, bound):
    """max err / bound where the bound is positive; where it is zero the error must be zero too."""
    z = bound <= 0
    assert not bool((err[z] != 0).any()), "non-zero error where the bound is exactly zero"
    return float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0


class Maxima(dict):
    def up(self, **kv):
        for k, v in kv.items():
            self[k] = max(self.get(k, 0.0), float(v))


def check_f32(tag, name, got, ref, bound, mx):
    ref, bound = ref.expand(got.shape), bound.expand(got.shape)
    err = (got.double() - ref).abs().nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(err, bound)})
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{tag}: {name} over its bound at {int(bad.sum())} places (worst {mx[name + '_frac']:.3g} of the bound)"


def check_bf16(tag, name, got, ref, a, mx):
    got, a = got.double(), a.expand(ref.shape)
    ok = (got >= bf16_rne(ref - a)) & (got <= bf16_rne(ref + a))
    beyond = ((got - ref).abs() - half_ulp_bf16(ref)).clamp_min(0).nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(beyond, a.contiguous())})         # the part of the error beyond half a bf16 ulp as a fraction of the allowance
    assert bool(ok.all()), f"{tag}: {name} outside [bf16(v - a), bf16(v + a)] at {int((~ok).sum())} places (worst {mx[name + '_frac']:.3g} of a beyond half an ulp)"


def poisoned(t):
    """A bf16 input with 32 rows of NaN behind it."""
    t = t.reshape(-1, t.shape[-1])
    return torch.cat([t, torch.full((POISON, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)])


def nan_tail(t):
    """An fp32 input (weights, statistics, partial rows) with 16 NaN behind it."""
    return torch.cat([t.detach().float().reshape(-1), torch.full((PAD,), float("nan"), device="cuda")])


def sentinel(n, cols=None, dtype=torch.float32):
    return torch.full((n + PAD,) if cols is None else (n + PAD, cols), SENT, dtype=dtype, device="cuda")


def sent_bits(t):
    return bits(torch.tensor([SENT], dtype=t.dtype)).item()


def all_sentinel(t):
    return torch.equal(bits(t), bits(torch.full(t.shape, SENT, dtype=t.dtype)))


def same_bits(a, b):
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def inner(tag, name, buf, n):
    """The first n rows / elements of an output: its tail still all-sentinel, everything inside written and finite."""
    assert all_sentinel(buf[n:]), f"{tag}: {name} written past its end"
    got = buf[:n]
    assert bool(torch.isfinite(got.float()).all()), f"{tag}: {name} is not finite"
    iv = {4: torch.int32, 2: torch.int16}[got.element_size()]
    assert not bool((got.contiguous().view(iv) == sent_bits(got)).any()), f"{tag}: an element of {name} was not written"
    return got


def call(name, *args):
    from protopformer_amd import _lib
    _lib.call(name, *args)


def twice(tag, fn):
    """fn() -> tuple of output buffers, run twice: bit-identical."""
    one, two = fn(), fn()
    torch.cuda.synchronize()
    for a, b in zip(one, two):
        assert a is None or same_bits(a, b), f"{tag}: two runs differ"
    return one


def split_heads(t, B, H, N, hd):
    """[B N][H hd] -> [B][H][N][hd]"""
    return t.reshape(B, N, H, hd).transpose(1, 2)


def merge_heads(t):
    B, H, N, hd = t.shape
    return t.transpose(1, 2).reshape(B * N, H * hd)


def mix(w, x):
    """y_g = sum_h w[g,h] x_h over dim 1 of [B][H][N][M]"""
    B, H, N, M = x.shape
    return (w @ x.reshape(B, H, N * M)).reshape(B, H, N, M)


def hb(x, a):
    """Half a bf16 ulp of an operand of magnitude |x| that carries the error a."""
    return half_ulp_bf16(x.abs() + a)


# ------------------------------------------------------------------------------------------------ talking heads: inputs and reference
def jstar_of(b, N):
    return (N // 2, N - 1)[b % 2]


def th_weights(family, H, seed):
    g = torch.Generator().manual_seed(seed)
    eye = torch.eye(H)
    wl, ww = eye + 0.3 * torch.randn(H, H, generator=g), eye + 0.3 * torch.randn(H, H, generator=g)
    bl, bw = 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    if family == "bw-large":
        bw = torch.full((H,), 0.5)
    elif family == "wl-negative":        # every mixed head subtracts 1.5 x its neighbour
        wl = wl - 1.5 * torch.roll(eye, 1, dims=1)
    elif family == "bl-80":
        bl = torch.tensor([80.0, -80.0, 79.5, -80.5])[:H]
    elif family == "peaked":             # row sums of Wl near 1: the peak survives the mix
        wl = eye + 0.05 * (wl - eye) / 0.3
    elif family == "ww-negative":        # bw negative too: the head mean is negative at every N (P is of the order of 1 / N, |bw| of 0.1)
        ww, bw = -ww, -bw.abs()
    elif family != "random":
        raise ValueError(family)
    return [t.float().cuda().contiguous() for t in (wl, bl, ww, bw)]


def th_qkv(family, B, H, N, hd, seed):
    x = 0.8 * torch.randn(B, N, 3, H, hd, device="cuda", generator=_gen(seed))
    if family == "peaked":               # q0 in 4.5 .. 7.5, key j*: 14 sqrt(hd) e0: its score is 63 .. 105 in every head, the others' within +-8
        x[:, :, 0, :, 0] = 6.0 + 0.5 * (x[:, :, 0, :, 0] / 0.8).clamp(-3, 3)
        for b in range(B):
            x[b, jstar_of(b, N), 1] = 0.0
            x[b, jstar_of(b, N), 1, :, 0] = 14.0 * hd ** 0.5
    return x.reshape(B * N, 3 * H * hd).bfloat16()


@functools.lru_cache(maxsize=4)
def th_problem(family, B, H, N, hd):
    """Inputs, the fp64 reference of the forward pass and the quantities its gates are made of (module docstring)."""
    D, scale = H * hd, hd ** -0.5
    seed = 1000 * hd + 7 * N + 3 * B + H
    qkv = th_qkv(family, B, H, N, hd, seed)
    w32 = th_weights(family, H, seed + 1)
    wl, bl, ww, bw = (t.double() for t in w32)
    t = qkv.double().reshape(B, N, 3, H, hd)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    S = scale * (q @ k.transpose(-1, -2))
    Sp = mix(wl, S) + bl.reshape(1, H, 1, 1)
    m = Sp.max(-1, keepdim=True)[0]
    e = torch.exp(Sp - m)
    Z = e.sum(-1, keepdim=True)
    zinv = 1.0 / Z
    P = e * zinv
    A = mix(ww, P) + bw.reshape(1, H, 1, 1)
    hm, Oh = A.mean(1), A @ v
    # the reference and the oracle cannot drift: the einsum / softmax lines of oracle.ppf_oracle.cait_talking_heads_attention in fp64
    s_or = torch.einsum("bhnm,gh->bgnm", (q * scale) @ k.transpose(-1, -2), wl) + bl.reshape(1, -1, 1, 1)
    p_or = torch.einsum("bhnm,gh->bgnm", s_or.softmax(dim=-1), ww) + bw.reshape(1, -1, 1, 1)
    assert bool(((p_or - A).abs() <= 1e-12 * (mix(ww.abs(), P) + bw.abs().reshape(1, H, 1, 1))).all()), "the fp64 reference and the oracle's formula differ"
    # ---- intrinsics: 4 x a plain fp32 torch evaluation of the same expression against fp64 on the same inputs
    Sp32, m32 = Sp.float(), m.float()
    e32 = torch.exp2(Sp32 * LOG2E32 - m32 * LOG2E32).double()
    sel = e > 2.0 ** -100
    exp_ref = float(((e32 - e).abs() / e)[sel].max())
    rcp_ref = float((((1.0 / Z.float()).double() - zinv).abs() / zinv).max())
    # ---- bounds
    a_s = scale * (hd + 8) * U * (q.abs() @ k.abs().transpose(-1, -2))
    a_sp = mix(wl.abs(), a_s) + (H + 6) * U * (mix(wl.abs(), S.abs()) + bl.abs().reshape(1, H, 1, 1))
    a_m = (Sp + a_sp).max(-1, keepdim=True)[0] - m
    R = Sp.abs().max(-1, keepdim=True)[0]
    spread = m - Sp.min(-1, keepdim=True)[0]
    r_e = a_sp + a_m + 6 * U * (Sp.abs() + R) + 4 * exp_ref
    n_big = (e >= 0.5 * U * Z / N ** 2).sum(-1, keepdim=True)
    resc = ((N + 31) // 32 + 2) * (4 * exp_ref + 3 * U * spread)
    a_Z = (e * r_e).sum(-1, keepdim=True) + (n_big + 1) * U * Z + resc * Z
    r_z = a_Z / Z + 2 * U + 4 * rcp_ref
    pr = SimpleNamespace(family=family, B=B, H=H, N=N, hd=hd, D=D, scale=scale, qkv=qkv, w32=w32, w=(wl, bl, ww, bw), q=q, k=k, v=v, S=S, Sp=Sp, m=m,
                         e=e, Z=Z, zinv=zinv, P=P, A=A, hm=hm, O=Oh, a_s=a_s, a_m=a_m, r_e=r_e, r_z=r_z, cache={},
                         ref_u=dict(exp_ref_u=exp_ref / U, rcp_ref_u=rcp_ref / U))
    pr.fwd_own = th_forward_bounds(pr, r_z)
    return pr


def th_forward_bounds(pr, r_zin):
    """a_P, a_A, a_hm, a_O for probabilities recomputed from statistics whose zinv carries the relative error r_zin."""
    H, N = pr.H, pr.N
    wl, bl, ww, bw = pr.w
    a_P = pr.P * (pr.r_e + r_zin + U) + FLUSH * pr.zinv
    a_A = mix(ww.abs(), a_P) + (H + 2) * U * (mix(ww.abs(), pr.P) + bw.abs().reshape(1, H, 1, 1))
    a_hm = a_A.mean(1) + (H + 4) * U * pr.A.abs().mean(1)
    a_O = (a_A + hb(pr.A, a_A) + (N + 8) * U * pr.A.abs()) @ pr.v.abs()
    return SimpleNamespace(a_P=a_P, a_A=a_A, a_hm=a_hm, a_O=a_O)


def weights_in(pr):
    return [nan_tail(t) for t in pr.w32]


# ------------------------------------------------------------------------------------------------ talking heads: forward
def run_th_fwd(tag, pr, with_out, NP, NPK):
    B, H, N, D = pr.B, pr.H, pr.N, pr.D
    qkv, (wl, bl, ww, bw) = poisoned(pr.qkv), weights_in(pr)

    def one():
        a16, hm = sentinel(B * H * N, NPK, torch.bfloat16), sentinel(B * N, NP)
        rowmax, zinv = sentinel(B * H * N), sentinel(B * H * N)
        out = sentinel(B * N, D, torch.bfloat16) if with_out else None
        call("ppf_th_fwd", qkv, wl, bl, ww, bw, a16, hm, rowmax, zinv, out, B, H, N, D, NP, NPK)
        return a16, hm, rowmax, zinv, out
    a16, hm, rowmax, zinv, out = twice(tag, one)
    return SimpleNamespace(a16=inner(tag, "a16", a16, B * H * N).reshape(B, H, N, NPK), hm=inner(tag, "hm", hm, B * N).reshape(B, N, NP),
                           rowmax=inner(tag, "rowmax", rowmax, B * H * N).reshape(B, H, N, 1), zinv=inner(tag, "zinv", zinv, B * H * N).reshape(B, H, N, 1),
                           out=inner(tag, "out", out, B * N) if with_out else None)


def check_th_fwd(tag, pr, res, mx):
    N, fb = pr.N, pr.fwd_own
    check_f32(tag, "rowmax", res.rowmax, pr.m, pr.a_m, mx)
    check_f32(tag, "zinv", res.zinv, pr.zinv, pr.zinv * pr.r_z, mx)
    assert bool((res.a16[..., N:] == 0).all()), f"{tag}: pad columns of a16 are not 0"
    assert bool((res.hm[..., N:] == 0).all()), f"{tag}: pad columns of hm are not 0"
    check_bf16(tag, "a16", res.a16[..., :N], pr.A, fb.a_A, mx)
    check_f32(tag, "hm", res.hm[..., :N], pr.hm, fb.a_hm, mx)
    if res.out is not None:
        check_bf16(tag, "out", res.out, merge_heads(pr.O), merge_heads(fb.a_O), mx)


def th_forward_both(tag, pr, mx):
    """With out at the product's paddings, without at the widest the entry accepts."""
    N = pr.N
    res = run_th_fwd(tag + " out", pr, True, ceil_to(N, 4), ceil_to(N, 8))
    check_th_fwd(tag + " out", pr, res, mx)
    wide = run_th_fwd(tag + " no-out", pr, False, ceil_to(N, 32), ceil_to(N, 32))
    check_th_fwd(tag + " no-out", pr, wide, mx)
    return res


# ------------------------------------------------------------------------------------------------ talking heads: backward
def make_dout(pr):
    return torch.randn(pr.B * pr.N, pr.D, device="cuda", generator=_gen(77 + pr.N + pr.hd + pr.H)).bfloat16()


def group_rows(x, N):
    """[..., N] query sums -> [..., groups]: the 112 queries of each workgroup"""
    G = groups(N)
    x = torch.nn.functional.pad(x, (0, G * 16 * TH_WAVES - N))
    return x.reshape(*x.shape[:-1], G, 16 * TH_WAVES).sum(-1)


def th_backward(pr, own):
    """fp64 autograd of the forward formula for make_dout(pr), and the allowances of ds16, the partial rows, the parameter gradients and
    (the chain) dq | dk | dv; own: the statistics, a16 and ds16 are the kernels' (module docstring)."""
    if own in pr.cache:
        return pr.cache[own]
    B, H, N, hd, D, scale = pr.B, pr.H, pr.N, pr.hd, pr.D, pr.scale
    dout = make_dout(pr)
    x = pr.qkv.double().requires_grad_(True)
    wl_r, bl_r, ww_r, bw_r = (t.clone().requires_grad_(True) for t in pr.w)
    t = x.reshape(B, N, 3, H, hd)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    S_r = scale * (q @ k.transpose(-1, -2))
    S_r.retain_grad()
    A_r = mix(ww_r, torch.softmax(mix(wl_r, S_r) + bl_r.reshape(1, H, 1, 1), -1)) + bw_r.reshape(1, H, 1, 1)
    merge_heads(A_r @ v).backward(dout.double())
    # the explicit chain the bounds are made of
    wl, bl, ww, bw = pr.w
    q, k, v, P, S = pr.q, pr.k, pr.v, pr.P, pr.S
    dO = split_heads(dout.double(), B, H, N, hd)
    dA = dO @ v.transpose(-1, -2)
    dP = mix(ww.t(), dA)
    dot = (dP * P).sum(-1, keepdim=True)
    dSp = P * (dP - dot)
    dS = mix(wl.t(), dSp)
    mag = P * (dP.abs() + (dP.abs() * P).sum(-1, keepdim=True))       # the size of dS' before its cancellation
    assert bool(((dS - S_r.grad).abs() <= 1e-10 * mix(wl.t().abs(), mag)).all()), "the explicit backward chain and autograd differ"
    NT = (N + 15) // 16
    a_P = pr.fwd_own.a_P if own else pr.P * (pr.r_e + 2 * U) + FLUSH * pr.zinv
    a_dA = (hd + 8) * U * (dO.abs() @ v.abs().transpose(-1, -2))
    a_dP = mix(ww.t().abs(), a_dA) + (H + 2) * U * mix(ww.t().abs(), dA.abs())
    a_dot = (a_dP * P + (dP.abs() + a_dP) * a_P).sum(-1, keepdim=True) + (4 * NT + 4) * U * (dP.abs() * P).sum(-1, keepdim=True)
    a_dSp = a_P * ((dP - dot).abs() + a_dP + a_dot) + P * (a_dP + a_dot) + 3 * U * dSp.abs()
    a_dS = mix(wl.t().abs(), a_dSp) + (H + 2) * U * mix(wl.t().abs(), dSp.abs())
    # partial rows [B][groups][dWw | dbw | dbl | dWl]: value, sum of |terms|, sum of the terms' errors, per query first
    a_S = pr.a_s + 3 * U * S.abs()
    ein = lambda a, b: torch.einsum("bgqj,bhqj->bghq", a, b).reshape(B, H * H, N)
    rows = [(ein(dA, P), ein(dA.abs(), P), ein(a_dA, P) + ein(dA.abs() + a_dA, a_P)),
            (dA.sum(-1), dA.abs().sum(-1), a_dA.sum(-1)),
            (dSp.sum(-1), dSp.abs().sum(-1), a_dSp.sum(-1)),
            (ein(dSp, S), ein(dSp.abs(), S.abs()), ein(a_dSp, S.abs() + a_S) + ein(dSp.abs(), a_S))]
    val, sab, ser = (group_rows(torch.cat([r[i] for r in rows], dim=1), N).transpose(1, 2) for i in range(3))      # [B][G][PW]
    a_part = ser + (4 * NT + 13 + 4) * U * sab
    total = torch.cat([t.grad.reshape(-1) for t in (ww_r, bw_r, bl_r, wl_r)])
    floor = float(mag.sum() * S.abs().max().clamp_min(1.0))
    assert bool(((val.sum((0, 1)) - total).abs() <= 1e-9 * (sab.sum((0, 1)) + floor)).all()), "the partial-row sums and autograd differ"
    # the chain's products on the kernels' ds16 / a16
    fb = pr.fwd_own
    tds = a_dS + hb(dS, a_dS) + (N + 8) * U * dS.abs()
    ref = x.grad
    a_dQ = scale * (tds @ k.abs()) + 3 * U * split_heads(ref[:, :D], B, H, N, hd).abs()
    a_dK = scale * (tds.transpose(-1, -2) @ q.abs()) + 3 * U * split_heads(ref[:, D:2 * D], B, H, N, hd).abs()
    a_dV = (fb.a_A + hb(pr.A, fb.a_A) + (N + 8) * U * pr.A.abs()).transpose(-1, -2) @ dO.abs()
    out = SimpleNamespace(dout=dout, dS=S_r.grad.detach(), a_dS=a_dS, part=val, part_abs=sab, a_part=a_part, total=total, dqkv=ref,
                          a_dqkv=torch.cat([merge_heads(a_dQ), merge_heads(a_dK), merge_heads(a_dV)], dim=1))
    pr.cache[own] = out
    return out


def run_th_bwd(tag, pr, dout, rowmax, zinv, NPK):
    B, H, N, D = pr.B, pr.H, pr.N, pr.D
    from protopformer_amd import _lib
    nfl = B * groups(N) * pw_of(H)
    assert int(_lib.lib().ppf_th_bwd_partial_floats(B, H, N)) == nfl
    qkv, dout, (wl, bl, ww, bw) = poisoned(pr.qkv), poisoned(dout), weights_in(pr)
    rowmax, zinv = nan_tail(rowmax), nan_tail(zinv)

    def one():
        ds16, partial = sentinel(B * H * N, NPK, torch.bfloat16), sentinel(nfl)
        call("ppf_th_bwd", qkv, dout, wl, bl, ww, rowmax, zinv, ds16, partial, B, H, N, D, NPK)
        return ds16, partial
    ds16, partial = twice(tag, one)
    return inner(tag, "ds16", ds16, B * H * N).reshape(B, H, N, NPK), inner(tag, "partial", partial, nfl).reshape(B, groups(N), pw_of(H))


def check_th_bwd(tag, pr, own, rowmax, zinv, mx):
    N, bw_ = pr.N, th_backward(pr, own)
    ds16, partial = run_th_bwd(tag, pr, bw_.dout, rowmax, zinv, ceil_to(N, 8))
    assert bool((ds16[..., N:] == 0).all()), f"{tag}: pad columns of ds16 are not 0"
    check_bf16(tag, "ds16", ds16[..., :N], bw_.dS, bw_.a_dS, mx)
    check_f32(tag, "partial", partial, bw_.part, bw_.a_part, mx)
    return ds16, partial


PREFILL = 0.25


def run_param_reduce(tag, pr, B, partial, mx, a_part=None, part_ref=None):
    """ppf_th_param_reduce on `partial` [B][groups][PW] (the kernel's) into prefilled gradients: prefill + total."""
    H, N, PW = pr.H, pr.N, pw_of(pr.H)
    nparts = B * groups(N)
    assert nparts <= 256, "more than one partial row per thread: the bound in the module docstring assumes one"
    sizes = [H * H, H, H, H * H]                                     # dww | dbw | dbl | dwl in the partial rows' order
    pre = [PREFILL * (1.0 + torch.arange(n, device="cuda", dtype=torch.float32)) * (-1.0) ** i for i, n in enumerate(sizes)]
    pin = nan_tail(partial)

    def one():
        bufs = [sentinel(n) for n in sizes]
        for b, p0 in zip(bufs, pre):
            b[:p0.numel()] = p0
        call("ppf_th_param_reduce", pin, B, H, N, *bufs)
        return tuple(bufs)
    bufs = twice(tag, one)
    got = torch.cat([inner(tag, name, b, n) for name, b, n in zip(("dww", "dbw", "dbl", "dwl"), bufs, sizes)])
    pre64, p64 = torch.cat(pre).double(), partial.double().reshape(nparts, PW)
    tree = 10 * U * (p64.abs().sum(0) + pre64.abs())
    check_f32(tag, "reduce_vs_input", got, pre64 + p64.sum(0), tree, mx)
    if a_part is not None:
        ref = part_ref.reshape(nparts, PW)
        check_f32(tag, "reduce_vs_ref", got, pre64 + ref.sum(0), a_part.reshape(nparts, PW).sum(0) + 10 * U * (ref.abs().sum(0) + pre64.abs()), mx)


def ref_stats(pr):
    return pr.m.float().reshape(-1), pr.zinv.float().reshape(-1)


def n_list(hd, H):
    c = cover(hd, H)
    return sorted({n for n in (1, 15, 16, 17, 32, 33, 112, 113, 196, 208, 224) if n <= c} | {c})


TH_SHAPES = [(hd, H, N) for hd, H in PAIRS for N in n_list(hd, H)]


@pytest.mark.parametrize("stage", ["fwd", "bwd"])
@pytest.mark.parametrize("hd,H,N", TH_SHAPES)
def test_th_kernels(hd, H, N, stage):
    pr = th_problem("random", 2, H, N, hd)
    tag = f"ppf_th_{stage}<{hd},{H}> N={N}"
    mx = Maxima(pr.ref_u)
    if stage == "fwd":
        th_forward_both(tag, pr, mx)
    else:
        ds16, partial = check_th_bwd(tag, pr, False, *ref_stats(pr), mx)
        b = th_backward(pr, False)
        wide, _ = run_th_bwd(tag + " wide", pr, b.dout, *ref_stats(pr), ceil_to(N, 16))
        assert bool((wide[..., N:] == 0).all()), f"{tag}: pad columns of the wide ds16 are not 0"
        assert same_bits(wide[..., :N], ds16[..., :N]), f"{tag}: ds16 depends on NPK"
        run_param_reduce(tag + " reduce", pr, 2, partial, mx, b.a_part, b.part)
    report(f"th_{stage}[{hd}-{H}-{N}]", **mx)


@pytest.mark.parametrize("N", [113, 100])
def test_th_param_reduce_three_samples(N):
    """B = 3: six partial rows at N = 113 (two workgroups per sample), three at N = 100."""
    pr = th_problem("random", 3, 4, N, 48)
    tag = f"ppf_th_param_reduce B=3 N={N}"
    mx = Maxima(pr.ref_u)
    _, partial = check_th_bwd(tag, pr, False, *ref_stats(pr), mx)
    b = th_backward(pr, False)
    run_param_reduce(tag, pr, 3, partial, mx, b.a_part, b.part)
    report(f"th_reduce_b3[{N}]", **mx)


# ------------------------------------------------------------------------------------------------ th_grads alone
def run_th_grads(tag, qkv, dout, ds16, a16, B, H, N, D):
    NPK = ds16.shape[-1]
    qkv, dout, ds16, a16 = (poisoned(t) for t in (qkv, dout, ds16, a16))

    def one():
        dqkv = sentinel(B * N, 3 * D, torch.bfloat16)
        call("ppf_th_grads", qkv, dout, ds16, a16, dqkv, B, H, N, D, NPK)
        return (dqkv,)
    return inner(tag, "dqkv", twice(tag, one)[0], B * N)


GRADS_CASES = [(hd, H) for hd in (32, 48, 64) for H in (2, 4)] + [(48, 1), (32, 3)]


@pytest.mark.parametrize("N", [1, 16, 17, 31, 32, 33, 128, 129, 196, 208])
@pytest.mark.parametrize("hd,H", GRADS_CASES)
def test_th_grads_alone(hd, H, N):
    from protopformer_amd import _lib
    B, D, NPK, scale = 2, H * hd, ceil_to(N, 8), hd ** -0.5
    assert _lib.lib().ppf_th_grads_supported(H, N, D) == 1
    g = _gen(31 * hd + 5 * N + H)
    qkv = (0.8 * torch.randn(B * N, 3 * D, device="cuda", generator=g)).bfloat16()
    dout = torch.randn(B * N, D, device="cuda", generator=g).bfloat16()
    ds16 = torch.zeros(B, H, N, NPK, dtype=torch.bfloat16, device="cuda")
    a16 = torch.zeros_like(ds16)
    ds16[..., :N] = (0.1 * torch.randn(B, H, N, N, device="cuda", generator=g)).bfloat16()
    a16[..., :N] = (torch.rand(B, H, N, N, device="cuda", generator=g) - 0.2).bfloat16()
    tag = f"ppf_th_grads<{hd}> H={H} N={N}"
    got = run_th_grads(tag, qkv, dout, ds16, a16, B, H, N, D)
    dsp, ap = ds16.clone(), a16.clone()
    dsp[..., N:], ap[..., N:] = 0.75, 0.75
    assert same_bits(got, run_th_grads(tag + " pads 0.75", qkv, dout, dsp, ap, B, H, N, D)), f"{tag}: dqkv depends on the pad columns of ds16 / a16"
    t = qkv.double().reshape(B, N, 3, H, hd)
    q, k = t[:, :, 0].transpose(1, 2), t[:, :, 1].transpose(1, 2)
    dO = split_heads(dout.double(), B, H, N, hd)
    ds, a = ds16[..., :N].double(), a16[..., :N].double()
    dQ, dK, dV = scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), a.transpose(-1, -2) @ dO
    a_dQ = scale * (N + 8) * U * (ds.abs() @ k.abs()) + 3 * U * dQ.abs()
    a_dK = scale * (N + 8) * U * (ds.abs().transpose(-1, -2) @ q.abs()) + 3 * U * dK.abs()
    a_dV = (N + 8) * U * (a.abs().transpose(-1, -2) @ dO.abs())
    mx = Maxima()
    for i, (name, ref, bound) in enumerate((("dq", dQ, a_dQ), ("dk", dK, a_dK), ("dv", dV, a_dV))):
        check_bf16(tag, name, got[:, i * D:(i + 1) * D], merge_heads(ref), merge_heads(bound), mx)
    report(f"th_grads[{hd}-{H}-{N}]", **mx)


# ------------------------------------------------------------------------------------------------ the chain
@pytest.mark.parametrize("which", ["N17", "largest"])
@pytest.mark.parametrize("hd,H", PAIRS)
def test_th_chain(hd, H, which):
    """th_fwd -> th_bwd -> th_grads -> th_param_reduce as the training step runs them, on the kernels' own statistics, a16 and ds16."""
    N = 17 if which == "N17" else min(208, cover(hd, H))
    pr = th_problem("random", 2, H, N, hd)
    tag = f"chain<{hd},{H}> N={N}"
    mx = Maxima(pr.ref_u)
    f = run_th_fwd(tag, pr, True, ceil_to(N, 4), ceil_to(N, 8))
    check_th_fwd(tag, pr, f, mx)
    b = th_backward(pr, True)
    ds16, partial = check_th_bwd(tag + " ppf_th_bwd", pr, True, f.rowmax.reshape(-1), f.zinv.reshape(-1), mx)
    got = run_th_grads(tag + " ppf_th_grads", pr.qkv, b.dout, ds16, f.a16, 2, H, N, pr.D)
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * pr.D, (i + 1) * pr.D)
        check_bf16(tag, name, got[:, sl], b.dqkv[:, sl], b.a_dqkv[:, sl], mx)
    run_param_reduce(tag + " ppf_th_param_reduce", pr, 2, partial, mx, b.a_part, b.part)     # b.part sums to autograd's gradients (asserted there)
    report(f"th_chain[{hd}-{H}-{N}]", **mx)


# ------------------------------------------------------------------------------------------------ talking heads: input families
@pytest.mark.parametrize("hd,H,N", FAMILY_SHAPES)
@pytest.mark.parametrize("family", ["random", "bw-large", "wl-negative", "bl-80", "peaked", "ww-negative"])
def test_th_input_families(family, hd, H, N):
    pr = th_problem(family, 2, H, N, hd)
    tag = f"{family} <{hd},{H}> N={N}"
    # the family is what it claims to be, on the reference
    if family == "bw-large":
        assert float(pr.w[3].min()) == 0.5
    elif family == "wl-negative":
        own_max = torch.zeros_like(pr.Sp, dtype=torch.bool).scatter_(-1, pr.S.argmax(-1, keepdim=True), True).any(1, keepdim=True)
        assert bool((~own_max.expand_as(pr.Sp))[pr.Sp == pr.m].any()), "no mixed maximum sits off every head's own maximum"
    elif family == "bl-80":
        assert float(pr.Sp.abs().min(-1)[0].max()) > 60.0 and bool(torch.isfinite(pr.e).all())
    elif family == "peaked":
        for b in range(pr.B):
            j = jstar_of(b, N)
            rest = torch.arange(N, device="cuda") != j
            assert float((pr.Sp[b][:, :, j:j + 1] - pr.Sp[b][:, :, rest]).min()) >= 30.0 and float((pr.zinv[b] - 1).abs().max()) < 1e-12
    elif family == "ww-negative":
        assert float(pr.A.max()) < 0.5 and float(pr.hm.min()) < 0.0 and float(pr.A.min()) < 0.0
    mx = Maxima(pr.ref_u)
    th_forward_both(tag + " ppf_th_fwd", pr, mx)
    _, partial = check_th_bwd(tag + " ppf_th_bwd", pr, False, *ref_stats(pr), mx)
    b = th_backward(pr, False)
    run_param_reduce(tag + " ppf_th_param_reduce", pr, 2, partial, mx, b.a_part, b.part)
    report(f"th_family[{family}-{hd}-{H}-{N}]", **mx)


# ------------------------------------------------------------------------------------------------ class attention
def ca_policy(kind, B, N1, seed):
    if kind == "none":
        return None
    pol = torch.zeros(B, N1, device="cuda")
    if kind == "zero":
        return pol
    g = _gen(seed)
    for b in range(B):
        if N1 == 1:
            pol[b, 0] = float(b % 2 == 0)
        else:
            pol[b, 0] = 1.0
            pol[b, torch.randperm(N1 - 1, device="cuda", generator=g)[:max(1, N1 // 3)] + 1] = 1.0
    return pol


@functools.lru_cache(maxsize=4)
def ca_problem(family, B, H, N1, hd, polkind):
    from oracle import ppf_oracle as O
    D, scale = H * hd, hd ** -0.5
    seed = 500 * hd + 11 * N1 + H
    g = _gen(seed)
    q = 1.5 * torch.randn(B, D, device="cuda", generator=g)
    k = 1.5 * torch.randn(B, N1, D, device="cuda", generator=g)
    v = torch.randn(B, N1, D, device="cuda", generator=g)
    pol = ca_policy(polkind, B, N1, seed + 1)
    qv, kv = q.reshape(B, H, hd), k.reshape(B, N1, H, hd)
    if family == "allneg":               # raw score -64 + noise
        qv *= 0.5; kv *= 0.5
        qv[:, :, 0] += 8.0; kv[:, :, :, 0] -= 8.0
    elif family == "maskedmax":          # q0 in 4.5 .. 7.5; the masked key j* scores 45 .. 75, the others within +-8
        qv[:, :, 0] = 6.0 + 0.5 * (qv[:, :, 0] / 1.5).clamp(-3, 3)
        kv *= 0.5
        for b in range(B):
            kv[b, jstar_of(b, N1)] = 0.0
            kv[b, jstar_of(b, N1), :, 0] = 10.0 * hd ** 0.5
            pol[b, jstar_of(b, N1)] = 0.0
    elif family != "random":
        raise ValueError(family)
    q, k, v = q.bfloat16(), k.reshape(B * N1, D).bfloat16(), v.reshape(B * N1, D).bfloat16()
    qh = q.double().reshape(B, 1, H, hd).transpose(1, 2)
    kh, vh = (t.double().reshape(B, N1, H, hd).transpose(1, 2) for t in (k, v))
    S = scale * (qh @ kh.transpose(-1, -2))                          # [B][H][1][N1]
    keep = torch.ones(B, 1, 1, N1, dtype=torch.float64, device="cuda") if pol is None else pol.double().reshape(B, 1, 1, N1)
    m = S.max(-1, keepdim=True)[0]
    e_all = torch.exp(S - m)
    e = e_all * keep
    Z = e.sum(-1, keepdim=True)
    c = EPS / N1
    zinv = 1.0 / (Z + EPS)
    attn = (e + c) * zinv
    p_or = O.policy_softmax(S.cpu(), torch.ones(B, N1) if pol is None else pol.cpu(), self_keep=False)
    assert p_or.dtype == torch.float64 and bool(((p_or - attn.cpu()).abs() <= 1e-12 * attn.cpu()).all()), "the fp64 reference and oracle.policy_softmax differ"
    sel = e_all > 2.0 ** -100
    exp_ref = float(((torch.exp(S.float() - m.float()).double() - e_all).abs() / e_all)[sel].max())
    rcp_ref = float((((1.0 / (Z.float() + float(np.float32(EPS)))).double() - zinv).abs() / zinv).max())
    a_s = scale * (hd + 8) * U * (qh.abs() @ kh.abs().transpose(-1, -2)) + 3 * U * S.abs()
    a_m = (S + a_s).max(-1, keepdim=True)[0] - m
    r_e = a_s + a_m + 6 * U * (S.abs() + m.abs()) + 4 * exp_ref
    n_big = (e >= 0.5 * U * Z / N1 ** 2).sum(-1, keepdim=True) * (Z > 0)
    a_Z = (e * r_e).sum(-1, keepdim=True) + (n_big + 1) * U * Z + N1 * FLUSH
    r_z = a_Z / (Z + EPS) + 2 * U + 4 * rcp_ref
    a_attn = attn * (r_z + 2 * U) + zinv * (e * r_e + 3 * U * c + FLUSH)
    a_mean = a_attn.mean(1) + (H + 2) * U * attn.mean(1)
    Oh = attn @ vh
    a_O = (a_attn + (N1 + 8) * U * attn) @ vh.abs()
    return SimpleNamespace(family=family, B=B, H=H, N1=N1, hd=hd, D=D, scale=scale, q=q, k=k, v=v, pol=pol, qh=qh, kh=kh, vh=vh, S=S, m=m, e=e, Z=Z, c=c,
                           keep=keep, zinv=zinv, attn=attn, O=Oh, r_z=r_z, a_attn=a_attn, a_mean=a_mean, a_O=a_O,
                           ref_u=dict(exp_ref_u=exp_ref / U, rcp_ref_u=rcp_ref / U))


def run_ca_fwd(tag, pr):
    B, H, N1, D = pr.B, pr.H, pr.N1, pr.D
    q, k, v = poisoned(pr.q), poisoned(pr.k), poisoned(pr.v)

    def one():
        attn, zinv, rowmean, out = sentinel(B * H * N1), sentinel(B * H), sentinel(B * N1), sentinel(B, D, torch.bfloat16)
        call("ppf_class_attn_fwd", q, k, v, pr.pol, attn, zinv, rowmean, out, B, H, N1, D)
        return attn, zinv, rowmean, out
    attn, zinv, rowmean, out = twice(tag, one)
    return SimpleNamespace(attn=inner(tag, "attn", attn, B * H * N1).reshape(B, H, 1, N1), zinv=inner(tag, "zinv", zinv, B * H).reshape(B, H, 1, 1),
                           rowmean=inner(tag, "rowmean", rowmean, B * N1).reshape(B, 1, N1), out=inner(tag, "out", out, B))


def check_ca_fwd(tag, pr, res, mx):
    check_f32(tag, "ca_attn", res.attn, pr.attn, pr.a_attn, mx)
    check_f32(tag, "ca_zinv", res.zinv, pr.zinv, pr.zinv * pr.r_z, mx)
    check_f32(tag, "ca_rowmean", res.rowmean, pr.attn.mean(1), pr.a_mean, mx)
    check_bf16(tag, "ca_out", res.out, pr.O.transpose(1, 2).reshape(pr.B, pr.D), pr.a_O.transpose(1, 2).reshape(pr.B, pr.D), mx)


def ca_backward(pr, dout, own):
    B, H, N1, hd, D, scale = pr.B, pr.H, pr.N1, pr.hd, pr.D, pr.scale
    qr, kr, vr = (t.double().requires_grad_(True) for t in (pr.q, pr.k, pr.v))
    qh = qr.reshape(B, 1, H, hd).transpose(1, 2)
    kh, vh = (t.reshape(B, N1, H, hd).transpose(1, 2) for t in (kr, vr))
    S = scale * (qh @ kh.transpose(-1, -2))
    e = torch.exp(S - S.max(-1, keepdim=True)[0]) * pr.keep
    ((e + pr.c) / (e.sum(-1, keepdim=True) + EPS) @ vh).transpose(1, 2).reshape(B, D).backward(dout.double())
    qh, kh, vh, attn, zinv = pr.qh, pr.kh, pr.vh, pr.attn, pr.zinv
    dO = dout.double().reshape(B, 1, H, hd).transpose(1, 2)          # [B][H][1][hd]
    a_in = pr.a_attn if own else U * attn
    r_zin = pr.r_z if own else U
    g = dO @ vh.transpose(-1, -2)
    a_g = (hd + 8) * U * (dO.abs() @ vh.abs().transpose(-1, -2))
    dot = (g * attn).sum(-1, keepdim=True)
    a_dot = (a_g * attn + g.abs() * a_in).sum(-1, keepdim=True) + 12 * U * (g.abs() * attn).sum(-1, keepdim=True)
    pt = pr.e * zinv
    a_pt = a_in + pr.c * zinv * (4 * U + r_zin) + U * attn
    dS = pt * (g - dot)
    # dL/dm = zinv sum_j g (attn Z - e), with attn Z - e = zinv (c Z - eps e) written without its cancellation, + 2**-40 of the sum of the
    # magnitudes for autograd's own fp64 evaluation of it
    gm = (zinv * zinv * (g * (pr.c * pr.Z - EPS * pr.e)).sum(-1, keepdim=True)).abs() + 2.0 ** -40 * (zinv * (g - dot).abs() * pr.e).sum(-1, keepdim=True)
    gm = gm * (pr.S == pr.m)
    a_dS = a_pt * ((g - dot).abs() + a_g + a_dot) + pt * (a_g + a_dot) + 3 * U * dS.abs() + gm
    ds, a_ds = scale * dS, scale * a_dS + 3 * U * scale * dS.abs()
    dk = ds.transpose(-1, -2) * qh                                   # [B][H][N1][hd]
    a_dk = a_ds.transpose(-1, -2) * qh.abs() + U * dk.abs()
    a_dv = a_in.transpose(-1, -2) * dO.abs() + U * (attn.transpose(-1, -2) * dO.abs())
    a_dq = (a_ds + (N1 + 8) * U * ds.abs()) @ kh.abs()               # [B][H][1][hd]
    flat = lambda t: t.transpose(1, 2).reshape(-1, D)
    return (qr.grad, kr.grad, vr.grad), (flat(a_dq), flat(a_dk), flat(a_dv))


def check_ca_bwd(tag, pr, own, attn_in, zinv_in, mx):
    B, H, N1, D = pr.B, pr.H, pr.N1, pr.D
    dout = torch.randn(B, D, device="cuda", generator=_gen(13 + N1 + pr.hd)).bfloat16()
    q, k, v, do = poisoned(pr.q), poisoned(pr.k), poisoned(pr.v), poisoned(dout)
    attn_in, zinv_in = nan_tail(attn_in), nan_tail(zinv_in)

    def one():
        dq, dk, dv = sentinel(B, D, torch.bfloat16), sentinel(B * N1, D, torch.bfloat16), sentinel(B * N1, D, torch.bfloat16)
        call("ppf_class_attn_bwd", q, k, v, attn_in, zinv_in, do, dq, dk, dv, B, H, N1, D)
        return dq, dk, dv
    dq, dk, dv = twice(tag, one)
    refs, bounds = ca_backward(pr, dout, own)
    for name, buf, n, ref, a in zip(("ca_dq", "ca_dk", "ca_dv"), (dq, dk, dv), (B, B * N1, B * N1), refs, bounds):
        check_bf16(tag, name, inner(tag, name, buf, n), ref, a, mx)


def ca_all(tag, pr, mx):
    res = run_ca_fwd(tag, pr)
    check_ca_fwd(tag + " ppf_class_attn_fwd", pr, res, mx)
    check_ca_bwd(tag + " ppf_class_attn_bwd", pr, False, pr.attn.float(), pr.zinv.float(), mx)
    check_ca_bwd(tag + " ppf_class_attn_bwd on the forward kernel's", pr, True, res.attn, res.zinv, mx)


@pytest.mark.parametrize("policy", [False, True], ids=["no-policy", "policy"])
@pytest.mark.parametrize("N1", [1, 63, 64, 65, 197, 256])
@pytest.mark.parametrize("hd", [2, 32, 48, 64])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_class_attn(H, hd, N1, policy):
    pr = ca_problem("random", 2, H, N1, hd, "rand" if policy else "none")
    mx = Maxima(pr.ref_u)
    ca_all(f"class attention H={H} hd={hd} N1={N1} policy={policy}", pr, mx)
    report(f"class_attn[{H}-{hd}-{N1}-{policy}]", **mx)


@pytest.mark.parametrize("hd,H,N1", [(48, 4, 197), (64, 2, 45), (32, 3, 100)])
@pytest.mark.parametrize("family", ["zero-policy", "maskedmax", "allneg"])
def test_class_attn_input_families(family, hd, H, N1):
    data, polkind = {"zero-policy": ("random", "zero"), "maskedmax": ("maskedmax", "rand"), "allneg": ("allneg", "rand")}[family]
    pr = ca_problem(data, 2, H, N1, hd, polkind)
    if family == "zero-policy":
        assert float(pr.Z.abs().max()) == 0.0 and bool(((pr.attn - 1.0 / N1).abs() <= 1e-12 / N1).all())
    elif family == "maskedmax":
        for b in range(pr.B):
            j = jstar_of(b, N1)
            kept = (pr.S[b] - 1e30 * (1.0 - pr.keep[b])).max(-1)[0]
            assert float((pr.S[b][..., j] - kept).min()) >= 30.0 and float(pr.Z[b].max()) < 1e-12
    else:
        assert float(pr.S.max()) < -1.0
    mx = Maxima(pr.ref_u)
    ca_all(f"class attention {family} H={H} hd={hd} N1={N1}", pr, mx)
    report(f"class_attn_family[{family}-{hd}-{H}-{N1}]", **mx)


# ------------------------------------------------------------------------------------------------ refusals
def test_cait_refusals():
    """Every documented refusal returns its code with an error string that names the entry point, and launches nothing.  Each case is stopped
    by a PPF_CHECK_ARG of the entry point (the shape checks come first, then the null checks), never by a launch."""
    from protopformer_amd import _lib
    lib = _lib.lib()
    # the two host predicates at their documented edges
    for hd, H in PAIRS:
        c = cover(hd, H)
        assert [lib.ppf_th_fused_supported(H, n, H * hd) for n in (1, c, c + 1)] == [1, 1, 0], (hd, H)
        assert max(n for n in range(1, 300) if lib.ppf_th_fused_supported(H, n, H * hd)) == c
    assert (cover(64, 4), cover(48, 4)) == (158, 211) and all(cover(hd, H) == 224 for hd, H in PAIRS if (hd, H) not in ((64, 4), (48, 4)))
    assert [lib.ppf_th_fused_supported(4, n, 256) for n in (158, 159)] == [1, 0] and [lib.ppf_th_fused_supported(4, n, 192) for n in (211, 212)] == [1, 0]
    assert [lib.ppf_th_fused_supported(2, n, 128) for n in (224, 225)] == [1, 0]
    for H in (1, 2, 3, 4):
        for hd in (32, 48, 64):
            assert [lib.ppf_th_grads_supported(H, n, H * hd) for n in (0, 1, 208, 209)] == [0, 1, 1, 0], (hd, H)
    assert lib.ppf_th_grads_supported(2, 64, 80) == 0 and lib.ppf_th_fused_supported(8, 64, 384) == 0 and lib.ppf_th_fused_supported(2, 64, 80) == 0

    B, NMAX, DMAX = 2, 256, 264
    qkv = poisoned(torch.zeros(B * NMAX, 3 * DMAX, dtype=torch.bfloat16, device="cuda"))
    act = poisoned(torch.zeros(B * NMAX, DMAX, dtype=torch.bfloat16, device="cuda"))
    sq_in = poisoned(torch.zeros(B * 4 * NMAX, NMAX, dtype=torch.bfloat16, device="cuda"))
    w = torch.ones(64, device="cuda")
    st_in = torch.ones(B * 4 * NMAX, device="cuda")
    pol = torch.ones(B, NMAX, device="cuda")
    outs = dict(a16=sentinel(B * 4 * NMAX, NMAX, torch.bfloat16), ds16=sentinel(B * 4 * NMAX, NMAX, torch.bfloat16), hm=sentinel(B * NMAX, NMAX),
                rowmax=sentinel(B * 4 * NMAX), zinv=sentinel(B * 4 * NMAX), out=sentinel(B * NMAX, DMAX, torch.bfloat16), partial=sentinel(4096),
                dqkv=sentinel(B * NMAX, 3 * DMAX, torch.bfloat16), dww=sentinel(16), dbw=sentinel(4), dbl=sentinel(4), dwl=sentinel(16),
                attn=sentinel(B * 4 * NMAX), czinv=sentinel(B * 4), rowmean=sentinel(B * NMAX), dq=sentinel(B, DMAX, torch.bfloat16),
                dk=sentinel(B * NMAX, DMAX, torch.bfloat16), dv=sentinel(B * NMAX, DMAX, torch.bfloat16))
    o = SimpleNamespace(**outs)
    X = object()                         # "the default"

    def pick(kw, name, default):
        return kw[name] if name in kw else default

    def fwd(N=64, H=2, hd=64, NP=None, NPK=None, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_th_fwd", p("qkv", qkv), p("wl", w), p("bl", w), p("ww", w), p("bw", w), p("a16", o.a16), p("hm", o.hm), p("rowmax", o.rowmax),
                p("zinv", o.zinv), o.out, B, H, N, H * hd, ceil_to(N, 4) if NP is None else NP, ceil_to(N, 8) if NPK is None else NPK)

    def bwd(N=64, H=2, hd=64, NPK=None, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_th_bwd", p("qkv", qkv), p("dout", act), p("wl", w), p("bl", w), p("ww", w), p("rowmax", st_in), p("zinv", st_in), p("ds16", o.ds16),
                p("partial", o.partial), B, H, N, H * hd, ceil_to(N, 8) if NPK is None else NPK)

    def grd(N=64, H=2, hd=64, NPK=None, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_th_grads", p("qkv", qkv), p("dout", act), p("ds16", sq_in), p("a16", sq_in), p("dqkv", o.dqkv), B, H, N, H * hd,
                ceil_to(N, 8) if NPK is None else NPK)

    def red(N=64, H=2, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_th_param_reduce", p("partial", st_in), B, H, N, p("dww", o.dww), p("dbw", o.dbw), p("dbl", o.dbl), p("dwl", o.dwl))

    def caf(N1=64, H=2, hd=64, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_class_attn_fwd", p("q", act), p("k", act), p("v", act), pol, p("attn", o.attn), p("zinv", o.czinv), p("rowmean", o.rowmean),
                p("out", o.out), B, H, N1, H * hd)

    def cab(N1=64, H=2, hd=64, **kw):
        p = lambda n, d: pick(kw, n, d)
        return ("ppf_class_attn_bwd", p("q", act), p("k", act), p("v", act), p("attn", st_in), p("zinv", st_in), p("dout", act), p("dq", o.dq), p("dk", o.dk),
                p("dv", o.dv), B, H, N1, H * hd)

    nulls = {fwd: ("qkv", "wl", "bl", "ww", "bw", "a16", "hm", "rowmax", "zinv"),
             bwd: ("qkv", "dout", "wl", "bl", "ww", "rowmax", "zinv", "ds16", "partial"),
             grd: ("qkv", "dout", "ds16", "a16", "dqkv"), red: ("partial", "dww", "dbw", "dbl", "dwl"),
             caf: ("q", "k", "v", "attn", "zinv", "rowmean", "out"), cab: ("q", "k", "v", "attn", "zinv", "dout", "dq", "dk", "dv")}
    cases = [("H = 8", ERR_SHAPE, [f(H=8, hd=32) for f in (fwd, bwd)] + [red(H=8)]),
             ("head_dim 40", ERR_SHAPE, [f(hd=40) for f in (fwd, bwd, grd)]),
             ("N = 0", ERR_SHAPE, [f(N=0, NPK=8) for f in (fwd, bwd, grd)] + [fwd(N=0, NP=4, NPK=8), red(N=0)]),
             ("N = 225", ERR_SHAPE, [f(N=225) for f in (fwd, bwd, grd)]),
             ("(4, 64) at N = 159", ERR_SHAPE, [f(N=159, H=4, hd=64) for f in (fwd, bwd)]),
             ("(4, 48) at N = 212", ERR_SHAPE, [f(N=212, H=4, hd=48) for f in (fwd, bwd)]),
             ("th_grads at N = 209", ERR_SHAPE, [grd(N=209)]),
             ("th_grads at NPK != ceil8(N)", ERR_SHAPE, [grd(N=61, NPK=72), grd(N=64, NPK=72), grd(N=61, NPK=56)]),
             ("NP % 4 != 0", ERR_SHAPE, [fwd(N=61, NP=62)]),
             ("NPK % 8 != 0", ERR_SHAPE, [fwd(N=61, NPK=68), bwd(N=61, NPK=68)]),
             ("NP < N", ERR_SHAPE, [fwd(N=61, NP=60), fwd(N=64, NP=60)]),
             ("NPK < NP", ERR_SHAPE, [fwd(N=61, NP=72, NPK=64)]),
             ("NPK < N", ERR_SHAPE, [bwd(N=61, NPK=56)]),
             ("NPK past the last key tile", ERR_SHAPE, [fwd(N=64, NPK=72), fwd(N=33, NPK=72), fwd(N=1, NPK=40), bwd(N=64, NPK=72), bwd(N=33, NPK=56),
                                                        bwd(N=1, NPK=24), fwd(N=224, NPK=232), bwd(N=224, NPK=232)]),
             ("class attention H = 5", ERR_SHAPE, [f(H=5, hd=32) for f in (caf, cab)]),
             ("class attention odd head_dim", ERR_SHAPE, [f(hd=33) for f in (caf, cab)]),
             ("class attention head_dim 66", ERR_SHAPE, [f(hd=66) for f in (caf, cab)]),
             ("class attention N1 = 257", ERR_SHAPE, [f(N1=257) for f in (caf, cab)]),
             ("class attention N1 = 0", ERR_SHAPE, [f(N1=0) for f in (caf, cab)]),
             ("every null", ERR_ARG, [f(**{name: None}) for f, names in nulls.items() for name in names])]
    for what, rc, calls in cases:
        for args in calls:
            with pytest.raises(RuntimeError, match=rf"rc={rc}\): {args[0]}\b"):
                call(*args)
    torch.cuda.synchronize()
    for name, buf in outs.items():
        assert all_sentinel(buf), f"a refused call wrote {name}"
    # the argument builders are sound: the unchanged calls are accepted (the widest accepted paddings among them)
    for args in (fwd(), fwd(NP=64, NPK=64), fwd(N=33, NP=64, NPK=64), bwd(), bwd(N=33, NPK=48), grd(), red(), caf(), cab()):
        call(*args)
    torch.cuda.synchronize()
    for name in ("a16", "ds16", "hm", "rowmax", "zinv", "out", "partial", "dqkv", "attn", "czinv", "rowmean", "dq", "dk", "dv"):
        assert not all_sentinel(outs[name]), f"an accepted call did not write {name}"
