"""Every instantiation behind the four attention entry points of csrc/attention.hip against an fp64 reference, at the smallest shapes that
reach it, called through the C ABI (refusals and NP cannot be expressed through ops).  B = 2, H = 2 (D = 2 hd) unless stated: the head
offset is exercised and the policy differs between the two samples.

Routes, how they are reached, and what is gated there:
  ppf_attn_fwd       attn_fwd_kernel<hd, NT>, hd in {32, 48, 64} x NT in {1, 2, 4, 7}: N = 1, 17, 32 (NT 1) / 33, 64 (NT 2) / 65, 128 (NT 4) /
                     129, 197, 224 (NT 7; 224: seven full key tiles, the largest N), each with and without a policy: out, rowmax, zinv
  ppf_attn_fwd_hm    attn_fwd16_kernel<64, NT16, POLICY, TAIL>: <6,P> N = 1, 16, 17, 80, 81, 96 with a policy; <6,F,F> 1, 16, 17, 80 and
                     <6,F,T> 81, 96 without; <13,P> 97, 112, 113, 192, 193, 208 with a policy; <13,F,F> 97, 112, 113, 192 and <13,F,T> 193, 208
                     without; each with headmean non-null and null: out, rowmax, zinv (against the reference and against ppf_attn_fwd's),
                     the head-mean map, its pad columns (NP = N rounded up to 4) exactly 0
  ppf_attn_headmean  attn_headmean_kernel<hd, 4>, hd in {32, 48, 64}: N = 1, 127, 128, 129, 130, 197, 224 (N mod 4 = 1, 3, 0, 1, 2, 1, 0; one and
                     two key blocks, one and two query blocks), with and without a policy, fed fp32(m) and fp32(zinv) of the reference
  ppf_attn_bwd       attn_bwd_stream_kernel<64, NT> and attn_bwd_onepass_kernel<48 | 32, NT>, NT in {1, 2, 4, 7}: N = 17, 33, 65, 129, 224 with and
                     without a policy on out = bf16_rne(O), rowmax = fp32(m), zinv = fp32(zinv) of the REFERENCE, and once per (hd, N) on the
                     outputs of the kernel forward, as the training step does: dq, dk, dv
  persistent walk    attn_bwd_stream_kernel<64, 7> at N = 129 with H = 1, D = 64, B = CUs + 1 (one slot per CU: an odd item count, the last
                     workgroup walks one item fewer) and <64, 4> at N = 97 with H = 8, B H = 2 CUs + 8 (three rounds): every item gated
  input families     (hd, N) = (64, 82) (64, 197) (48, 45) (32, 100) through every entry point that takes the shape: all-negative scores (q near
                     +8 e0, k near -8 e0: a zero-filled padded key would own the row maximum); the maximum on a masked key >= 30 above every
                     kept key (kept mass ~1e-13: the eps terms dominate); policy all zero with self_keep = 0 (Z = 0: P = (eps / N_ref) / eps =
                     1 / N_ref, out = sum_j v_j / N_ref, asserted on the reference in closed form) and with self_keep = 1 (mass on the
                     diagonal); eps_n = 197 at N < 197 with a policy; the known-answer construction of test_attn_eps_term_known_answer (score
                     0 on one key, -200 elsewhere) at eps_n = 197, N = 82 / 45: c = eps / 197 in the map, asserted on the reference in closed form
  refusals           N = 225, N = 0, hd = 40, D % H != 0, D % 8 != 0, ppf_attn_fwd_hm at hd 48 and N = 209, NP = N + 4 when N % 4 == 0, NP % 4 != 0,
                     NP < N, null qkv / rowmax / zinv, null out / dout / dqkv / delta of the backward: the documented code, an error string naming
                     the entry point, and every output still all-sentinel.  (ppf_attn_headmean tiles queries and keys by its grid and has no
                     upper limit on N: N = 225 is refused by the other three.)

Poison and sentinels, every call: qkv, out (the backward's input) and dout carry 32 rows of bf16 NaN behind the last sample; out, rowmax, zinv,
headmean, dqkv and delta carry 16 more rows / elements of a sentinel bit pattern that must survive bit for bit; everything inside is finite;
dqkv is prefilled with the sentinel and none may be left in its B N rows.  Every call runs twice: bit-identical.

Reference: fp64 torch on the device from the exactly representable bf16 q / k / v / dout and the 0 / 1 policy: S = scale q k^T, keep = policy
(+ (1 - policy) I with self_keep), m = max_j S over all keys, e = exp(S - m) keep, Z = sum_j e, P = (e + eps / N_ref) / (Z + eps), N_ref =
eps_n or N, O = P V, head mean = mean_h P, rowmax = m, zinv = 1 / (Z + eps).  Every problem is checked once against
oracle.ppf_oracle.policy_softmax in fp64 (at N_ref = N, the oracle's only form).  Backward: fp64 autograd of that formula, the maximum included.

Gates, u = 2**-24, every scale from the fp64 reference, A = |q| |k|^T:
  scores     bf16 x bf16 products are exact in fp32, the additions round: a_s = scale (hd + 8) u A (any order, the convention of the GEMM file)
  rowmax     the largest computed score lies between m - a_s (at a key that attains m) and max_j (S + a_s): a_m = max_j (S + a_s) - m covers
             both sides; |rowmax - m| <= a_m + 2 u |m| (scale = 1 / sqrtf(hd) and the multiplication)
  e          exp2(s c1 - m1), c1 = scale log2(e): relative r_e = a_s + a_m + 6 u (|S| + |m|) + r_exp: three roundings of the evaluation (s c1, m1,
             the difference) and three inside c1, each <= u (|S| + |m|) log2(e), times ln 2.  The project gives no figure for v_exp_f32, the
             reciprocal or v_log_f32: r_exp, r_rcp, r_log = 4 x the worst error of a plain fp32 torch evaluation of the same expression
             (exp2(s32 c1 - m32 c1) where e > 2**-100; 1 / (Z32 + eps32); log2(zinv32) as an absolute error times ln 2) against fp64 on the
             same inputs -- reference against reference, reported as exp_ref_u, rcp_ref_u, log_ref_u
  zinv       Z is a sum of N non-negative terms in some tree order.  An addition errs by at most u Z and by at most its smaller operand; call
             a term small when it is below u Z / N**2: the additions whose smaller side holds only small terms err by at most those terms,
             each counted at most N times (N terms x N counts x u Z / N**2 = u Z in all); the others are at most n_big - 1, n_big the number of terms that
             are not small (counted on the reference at half the threshold).  a_Z = sum_j e r_e + (n_big + 1) u Z: (N + 1) u Z on an
             ordinary row, 2 u Z where one key holds the mass; relative r_z = a_Z / (Z + eps) + 2 u + r_rcp
  head mean  P = (e keep + c) zinv per head, c = eps_c (two roundings), summed over H heads and multiplied by 1 / H:
             a_hm = mean_h P (r_z + r_e + 6 u) + (H + 4) u hm.  The TAIL instantiations add c sum_h zinv / H at the store: the same bound.  No
             allowance for a dropped eps term: the map must carry it
  underflow  an fp32 exp2 returns nothing between 0 and the smallest normal number: absolute 2**-126 on e (on p = e zinv in the backward:
             2**-126 max(1, zinv), the streaming kernel's exp2 returns p itself).  The known-answer family has e = exp(-200)
  out        the unnormalised p = e keep + c has the fp32 error a_p = p (r_e + 3 u) + 2**-126 and is rounded to bf16 before the product: half a
             bf16 ulp of the term, h(p) = half_ulp_bf16(p + a_p), between 2**-9 p and 2**-8 p.  (A flat 2**-9 p per term would be half of
             round-to-nearest's worst case: an fp32 emulation of exactly these rounding points in plain torch misses a 2**-9 gate by up to
             1.6 x on rows that one term dominates -- a masked query's own key, a peaked row -- and stays within h(p) everywhere.)  fp32
             accumulation over N keys (N + 8) u sum_j |p| |v|; times zinv: |O| (r_z + u);
             a_O = zinv sum_j (a_p + h(p) + (N + 8) u p) |v| + |O| (r_z + u), and the bf16 store is the exact interval
             bf16_rne(O - a_O) <= out <= bf16_rne(O + a_O) (no rtol).  TAIL instantiations only: + 1e-6 max |v| of the (sample, head), the eps
             term of the output that the kernel comment bounds and drops.  (The 32-row kernel keeps e + c in every instantiation -- `s = e + c`
             -- so it gets no such allowance, with or without a policy.)
  backward   delta = sum_d dO out from the bf16 out: a_delta = sum_d |dO| a_in + (hd + 8) u sum_d |dO| |O|, a_in = half a bf16 ulp of O (the
             reference's bf16_rne(O)), or a_O + 2**-8 (|O| + a_O) when out is the forward kernel's; g = dO V^T: a_g = (hd + 8) u |dO| |V|^T;
             p = exp2(s c1 - m') zinv keep, relative r_p = r_e + 4 u + 4 u |ln zinv| + r_log (the streaming kernel folds zinv into the exponent:
             m' = m log2(e) - log2(zinv); the one-pass kernel multiplies: fewer roundings), + r_z on the forward kernel's statistics;
             dS = p (g - delta): a_dS = p (a_g + a_delta + 2 u (|g| + |delta|)) + |dS| (r_p + u) + 2**-126 max(1, zinv) |g - delta| + |dL/dm| on
             the keys that tie for the row maximum (the kernels hold m constant; autograd sends dL/dm = zinv sum_j g (P Z - e), of the order
             of eps, to the arg max); dS and P are rounded to bf16 (half an ulp of the term, h as above) before the products, which accumulate
             N terms in fp32: a_dQ = scale (a_dS + h(dS) + (N + 8) u |dS|) |K| + 2 u |dQ|, dK the same with dS^T and |Q|,
             a_dV = (a_P + h(P) + (N + 8) u P)^T |dO|, a_P = P (r_p + 3 u) + 2**-126 max(1, zinv); all three are bf16 stores: the exact interval
  statistics of ppf_attn_fwd_hm against ppf_attn_fwd's: both within their gate of the reference, so within twice the gate of each other.
No gate is set from the output of a kernel under test.

Measured maxima on an MI355X (helpers.report: *_frac = the worst error as a fraction of its gate -- for bf16 outputs the part beyond half a
bf16 ulp as a fraction of the allowance):
  ppf_attn_fwd        out 0.885   rowmax 0.046   zinv 0.019
  ppf_attn_fwd_hm     out 0.842   rowmax 0.022   zinv 0.012   head mean 0.0057   against ppf_attn_fwd's: rowmax bit-identical, zinv 0.0025
  ppf_attn_headmean   head mean 0.010
  ppf_attn_bwd        dq 0.506   dk 0.995   dv 0.966; the persistent walks dq 0.497   dk 0.996   dv 0.968
  families            all-negative: out 0.365, rowmax 0.061, dq / dk / dv 0.29 / 0.25 / 0.36; masked maximum: out 0.254, zinv 0.0064, head mean
                      0.0023, dq / dk / dv 0.996 / 0.79 / 0.096; zero policy, self_keep 0: out 0.29, head mean 0.0006, dq = dk = 0 exactly,
                      dv 0.12; self_keep 1: out 0.961, dq / dk / dv 0.995 / 0.996 / 0.949; eps_n: out 0.83, head mean 0.0093, dk 0.995;
                      known answer at eps_n = 197: zinv 0.109, head mean 0.036, dv 0.31, out exact
  reference against reference: exp2 <= 36 u on the random family, 122 u where the scores reach -74 (the argument's own rounding, |x| u);
  reciprocal <= 2.3 u; log2 <= 21 u ln 2
The fractions near 1 are rows that ONE term owns -- a masked key's dk is the single product bf16(dS_jj) q_j of "a masked query still attends
to itself", so the error IS that operand's bf16 rounding and the gate is its half-ulp: nothing to spare and nothing missing; the fp32 torch
emulation of the same rounding points gives the same 0.99.  The whole file runs in 5.4 s (220 tests; the slowest, the first, 1.3 s with the
library load; 0.2 s for CUs + 1 items at N = 129).

The gates bite: value-only edits of attention.hip (a scratch build, nothing committed; no address, bound or launch geometry changes), each
run against this file and against test_gpu_attention.py as it stands:
fail here, pass there:
  1. eps_c from N instead of eps_n (fill)                              -> the eps_n and known-answer families at all three head widths: 6 tests
  2. delta multiplied by (1 + 2**-7), both backward kernels            -> 42 tests: test_attn_bwd at every head width, both walks, five families
  3. K rows past N zero-filled instead of clamped (Stage::load<true>)  -> the all-negative family x 4, and N = 1 of test_attn_fwd /
                                                                          test_attn_fwd_hm (a single negative score against a padded 0): 14 tests
  4. st_cz = 0 in the streaming backward (P without its eps term)      -> 20 tests: dv of masked keys in every policy case at head_dim 64,
                                                                          both walks, five families
  5. po = pt without cz in the one-pass backward                       -> 30 tests: the same at head_dim 48 / 32
  6. attn_fwd_kernel multiplies bf16(e) instead of bf16(e + c)         -> 12 tests: masked maximum, zero policy with and without self_keep
  7. czsum += c instead of c zinv in the TAIL head mean                -> test_attn_fwd_hm N = 81, 96, 193, 208 without a policy, with the map
fail in both files, so they do not count: the head-mean kernel without + cc[i] (54 tests here, 1 there), zinv of the TAIL path without
SOFTMAX_EPS (1 / 2: only the known answer at Z = 1 sees 1e-6 of zinv, here after the n_big form of a_Z), rowmax + 1e-3 in attn_fwd_kernel
(145 / 15), zinv of attn_fwd_kernel without SOFTMAX_EPS (26 / 4), qself compared against q + 1 (162 / 26), the head mean over H + 1 in fwd16
(34 / 11), dK without scale (24 / 5), fwd16's per-element softmax without + c (25 / 3)."""
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
FLUSH = 2.0 ** -126                      # an fp32 exp2 returns nothing below the smallest normal number (module docstring)
LN2 = math.log(2.0)
FAMILY_SHAPES = [(64, 82), (64, 197), (48, 45), (32, 100)]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def make_policy(kind, B, N, seed):
    """[B][N] fp32 in {0, 1}, different in every sample; None: no policy."""
    if kind == "none":
        return None
    pol = torch.zeros(B, N, device="cuda")
    if kind == "zero":
        return pol
    g = _gen(seed)
    for b in range(B):
        if N == 1:
            pol[b, 0] = float(b % 2 == 0)
        else:
            pol[b, 0] = 1.0
            pol[b, torch.randperm(N - 1, device="cuda", generator=g)[:max(1, N // 3)] + 1] = 1.0
    return pol


def jstar_of(b, N):
    return (N // 2, N - 1)[b % 2]        # the masked maximum sits mid-row in even samples and on the last real key in odd ones


def make_qkv(family, B, H, N, hd, seed):
    g = _gen(seed)
    x = torch.randn(B, N, 3, H, hd, device="cuda", generator=g)
    if family == "random":
        x *= 1.5
    elif family == "allneg":             # raw score -64 + noise: every score negative
        x[:, :, :2] *= 0.5
        x[:, :, 0, :, 0] += 8.0
        x[:, :, 1, :, 0] -= 8.0
    elif family == "maskedmax":          # q0 in 6 +- 1.5; key j*: beta e0 with scale beta = 9: its score is 40 .. 68, the others' within +-6
        x[:, :, 0, :, 0] = 6.0 + 0.5 * x[:, :, 0, :, 0].clamp(-3, 3)
        for b in range(B):
            x[b, jstar_of(b, N), 1] = 0.0
            x[b, jstar_of(b, N), 1, :, 0] = 9.0 * hd ** 0.5
    elif family == "onehot":             # score 0 on key 5, -200 elsewhere (exp underflows to exactly 0 in fp32)
        x[:, :, :2] = 0.0
        a = 200.0 ** 0.5 * hd ** 0.25
        x[:, :, 0, :, 0] = a
        x[:, :, 1, :, 0] = -a
        x[:, 5, 1] = 0.0
    else:
        raise ValueError(family)
    return x.reshape(B * N, 3 * H * hd).bfloat16()


def split_heads(t, B, H, N, hd):
    """[B N][H hd] -> [B][H][N][hd]"""
    return t.reshape(B, N, H, hd).transpose(1, 2)


def merge_heads(t):
    B, H, N, hd = t.shape
    return t.transpose(1, 2).reshape(B * N, H * hd)


@functools.lru_cache(maxsize=4)
def problem(family, B, H, N, hd, polkind, self_keep, eps_n):
    """Inputs, the fp64 reference of the forward pass and the quantities its gates are made of (module docstring)."""
    from oracle import ppf_oracle as O
    D, scale = H * hd, hd ** -0.5
    seed = 1000 * hd + 7 * N + 3 * B + H + (eps_n > 0)
    qkv = make_qkv(family, B, H, N, hd, seed)
    pol = make_policy(polkind, B, N, seed + 1)
    if family == "maskedmax":
        for b in range(B):
            pol[b, jstar_of(b, N)] = 0.0
    t = qkv.double().reshape(B, N, 3, H, hd)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    raw = q @ k.transpose(-1, -2)
    S = scale * raw
    keep = torch.ones(B, 1, 1, N, dtype=torch.float64, device="cuda") if pol is None else pol.double().reshape(B, 1, 1, N)
    if self_keep:
        keep = keep + (1.0 - keep) * torch.eye(N, dtype=torch.float64, device="cuda")
    keep = keep.expand(B, H, N, N)
    m = S.max(-1, keepdim=True)[0]
    e_all = torch.exp(S - m)
    e = e_all * keep
    Z = e.sum(-1, keepdim=True)
    nref = eps_n if eps_n > 0 else N
    c = EPS / nref
    P = (e + c) / (Z + EPS)
    zinv = 1.0 / (Z + EPS)
    # the reference and the oracle cannot drift: the oracle's softmax (eps / N only) in fp64 on the same scores
    p_or = O.policy_softmax(S.cpu(), torch.ones(B, N) if pol is None else pol.cpu(), self_keep=bool(self_keep))
    p_n = ((e + EPS / N) / (Z + EPS)).cpu()
    assert p_or.dtype == torch.float64 and bool(((p_or - p_n).abs() <= 1e-12 * p_n).all()), "the fp64 reference and oracle.policy_softmax differ"
    Oh = P @ v
    # ---- intrinsics: 4 x a plain fp32 torch evaluation of the same expression against fp64 on the same inputs
    scale32 = np.float32(1.0) / np.sqrt(np.float32(hd))
    c1 = float(np.float32(scale32 * np.float32(1.44269504088896340736)))
    raw32 = raw.float()
    e32 = torch.exp2(raw32 * c1 - raw32.max(-1, keepdim=True)[0] * c1).double()
    sel = e_all > 2.0 ** -100
    exp_ref = float(((e32 - e_all).abs() / e_all)[sel].max())
    zinv32 = 1.0 / (Z.float() + float(np.float32(EPS)))
    rcp_ref = float(((zinv32.double() - zinv).abs() / zinv).max())
    log_ref = float((torch.log2(zinv.float()).double() - torch.log2(zinv)).abs().max()) * LN2
    A = q.abs() @ k.abs().transpose(-1, -2)
    a_s = scale * (hd + 8) * U * A
    a_m = (S + a_s).max(-1, keepdim=True)[0] - m
    r_e = a_s + a_m + 6 * U * (S.abs() + m.abs()) + 4 * exp_ref
    n_big = (e >= 0.5 * U * Z / N ** 2).sum(-1, keepdim=True) * (Z > 0)
    a_Z = (e * r_e).sum(-1, keepdim=True) + (n_big + 1) * U * Z
    r_z = a_Z / (Z + EPS) + 2 * U + 4 * rcp_ref
    pun = e + c                                                     # the unnormalised probability the P.V product sees
    a_pun = pun * (r_e + 3 * U) + FLUSH
    a_O = zinv * ((a_pun + half_ulp_bf16(pun + a_pun) + (N + 8) * U * pun) @ v.abs()) + Oh.abs() * (r_z + U)
    hm = P.mean(1)
    a_hm = (P * (r_z + r_e + 6 * U) + FLUSH * zinv).mean(1) + (H + 4) * U * hm
    return SimpleNamespace(family=family, B=B, H=H, N=N, hd=hd, D=D, scale=scale, self_keep=int(self_keep), eps_n=eps_n, nref=nref, qkv=qkv, pol=pol,
                           q=q, k=k, v=v, S=S, m=m, e=e, Z=Z, P=P, zinv=zinv, O=Oh, hm=hm, keep=keep, a_m=a_m + 2 * U * m.abs(), r_e=r_e, r_z=r_z,
                           a_O=a_O, a_tail=1e-6 * v.abs().amax((-1, -2), keepdim=True), a_hm=a_hm, r_log=4 * log_ref,
                           ref_u=dict(exp_ref_u=exp_ref / U, rcp_ref_u=rcp_ref / U, log_ref_u=log_ref / U))


# ------------------------------------------------------------------------------------------------ checks
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
    err = (got.double() - ref).abs().nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(err, bound)})
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{tag}: {name} over its bound at {int(bad.sum())} places (worst {mx[name + '_frac']:.3g} of the bound)"


def check_bf16(tag, name, got, ref, a, mx):
    got = got.double()
    ok = (got >= bf16_rne(ref - a)) & (got <= bf16_rne(ref + a))
    beyond = ((got - ref).abs() - half_ulp_bf16(ref)).clamp_min(0).nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(beyond, a)})         # the part of the error beyond half a bf16 ulp as a fraction of the allowance
    assert bool(ok.all()), f"{tag}: {name} outside [bf16(v - a), bf16(v + a)] at {int((~ok).sum())} places (worst {mx[name + '_frac']:.3g} of a beyond half an ulp)"


def poisoned(t):
    return torch.cat([t, torch.full((POISON, t.shape[1]), float("nan"), dtype=t.dtype, device=t.device)])


def sentinel(n, cols=None, dtype=torch.float32):
    return torch.full((n + PAD,) if cols is None else (n + PAD, cols), SENT, dtype=dtype, device="cuda")


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
    return got


def call(name, *args):
    from protopformer_amd import _lib
    _lib.call(name, *args)


def np_of(N):
    return (N + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ forward
def run_forward(tag, pr, entry, with_map=True):
    """ppf_attn_fwd or ppf_attn_fwd_hm, twice: sentinels, finiteness, two runs bit-identical."""
    B, H, N, D, NP = pr.B, pr.H, pr.N, pr.D, np_of(pr.N)
    qkv = poisoned(pr.qkv)
    runs = []
    for _ in range(2):
        out, rowmax, zinv = sentinel(B * N, D, torch.bfloat16), sentinel(B * H * N), sentinel(B * H * N)
        hm = sentinel(B * N * NP) if entry == "ppf_attn_fwd_hm" and with_map else None
        if entry == "ppf_attn_fwd":
            call(entry, qkv, out, pr.pol, rowmax, zinv, B, H, N, D, pr.self_keep, pr.eps_n)
        else:
            call(entry, qkv, out, pr.pol, rowmax, zinv, hm, NP, B, H, N, D, pr.self_keep, pr.eps_n)
        runs.append((out, rowmax, zinv, hm))
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert a is None or same_bits(a, b), f"{tag}: two runs differ"
    out, rowmax, zinv, hm = runs[0]
    return SimpleNamespace(out=inner(tag, "out", out, B * N), rowmax=inner(tag, "rowmax", rowmax, B * H * N).reshape(B, H, N, 1),
                           zinv=inner(tag, "zinv", zinv, B * H * N).reshape(B, H, N, 1),
                           hm=None if hm is None else inner(tag, "headmean", hm, B * N * NP).reshape(B, N, NP))


def check_map(tag, pr, hm, mx):
    N = pr.N
    if hm.shape[-1] > N:
        assert bool((hm[:, :, N:] == 0).all()), f"{tag}: pad columns of the head-mean map are not 0"
    check_f32(tag, "hm", hm[:, :, :N], pr.hm, pr.a_hm, mx)


def check_forward(tag, pr, res, tail, mx):
    check_f32(tag, "rowmax", res.rowmax, pr.m, pr.a_m, mx)
    check_f32(tag, "zinv", res.zinv, pr.zinv, pr.zinv * pr.r_z, mx)
    a = pr.a_O + (pr.a_tail if tail else 0.0)
    check_bf16(tag, "out", res.out, merge_heads(pr.O), merge_heads(a.expand_as(pr.O)), mx)
    if res.hm is not None:
        check_map(tag, pr, res.hm, mx)


def fwd16_route(N, policy):
    nt = 13 if N > 96 else 6
    tail = not policy and (N > 192 or 80 < N <= 96)
    return f"<{nt},{'P' if policy else 'F'},{'T' if tail else 'F'}>", tail


def run_headmean(tag, pr, rowmax, zinv):
    B, H, N, D, NP = pr.B, pr.H, pr.N, pr.D, np_of(pr.N)
    qkv = poisoned(pr.qkv)
    runs = []
    for _ in range(2):
        hm = sentinel(B * N * NP)
        call("ppf_attn_headmean", qkv, pr.pol, rowmax, zinv, hm, NP, B, H, N, D, pr.self_keep, pr.eps_n)
        runs.append(hm)
    torch.cuda.synchronize()
    assert same_bits(*runs), f"{tag}: two runs differ"
    return inner(tag, "headmean", runs[0], B * N * NP).reshape(B, N, NP)


def ref_stats(pr):
    """fp32(m), fp32(zinv) of the reference, with a sentinel tail (inputs of ppf_attn_headmean / ppf_attn_bwd)."""
    n = pr.B * pr.H * pr.N
    rowmax, zinv = sentinel(n), sentinel(n)
    rowmax[:n] = pr.m.float().reshape(-1)
    zinv[:n] = pr.zinv.float().reshape(-1)
    return rowmax, zinv


FWD_N = [1, 17, 32, 33, 64, 65, 128, 129, 197, 224]


@pytest.mark.parametrize("policy", [False, True], ids=["no-policy", "policy"])
@pytest.mark.parametrize("N", FWD_N)
@pytest.mark.parametrize("hd", [32, 48, 64])
def test_attn_fwd(hd, N, policy):
    pr = problem("random", 2, 2, N, hd, "rand" if policy else "none", 1, 0)
    tag = f"ppf_attn_fwd hd={hd} N={N} policy={policy}"
    mx = Maxima(pr.ref_u)
    check_forward(tag, pr, run_forward(tag, pr, "ppf_attn_fwd"), False, mx)
    report(f"attn_fwd[{hd}-{N}-{policy}]", **mx)


HM_N = [1, 16, 17, 80, 81, 96, 97, 112, 113, 192, 193, 208]


@pytest.mark.parametrize("with_map", [True, False], ids=["with-map", "no-map"])
@pytest.mark.parametrize("policy", [False, True], ids=["no-policy", "policy"])
@pytest.mark.parametrize("N", HM_N)
def test_attn_fwd_hm(N, policy, with_map):
    pr = problem("random", 2, 2, N, 64, "rand" if policy else "none", 1, 0)
    route, tail = fwd16_route(N, policy)
    tag = f"ppf_attn_fwd_hm {route} N={N} map={with_map}"
    mx = Maxima(pr.ref_u)
    res = run_forward(tag, pr, "ppf_attn_fwd_hm", with_map)
    assert (res.hm is not None) == with_map
    check_forward(tag, pr, res, tail, mx)
    two = run_forward(tag, pr, "ppf_attn_fwd")                      # the 32-row kernel's statistics: the same contract for the backward
    check_f32(tag, "rowmax_vs_fwd", res.rowmax, two.rowmax.double(), 2 * pr.a_m, mx)
    check_f32(tag, "zinv_vs_fwd", res.zinv, two.zinv.double(), 2 * pr.zinv * pr.r_z, mx)
    report(f"attn_fwd_hm[{route}-{N}-{with_map}]", **mx)


@pytest.mark.parametrize("policy", [False, True], ids=["no-policy", "policy"])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 130, 197, 224])
@pytest.mark.parametrize("hd", [32, 48, 64])
def test_attn_headmean(hd, N, policy):
    pr = problem("random", 2, 2, N, hd, "rand" if policy else "none", 1, 0)
    tag = f"ppf_attn_headmean hd={hd} N={N} policy={policy}"
    mx = Maxima(pr.ref_u)
    check_map(tag, pr, run_headmean(tag, pr, *ref_stats(pr)), mx)
    report(f"attn_headmean[{hd}-{N}-{policy}]", **mx)


# ------------------------------------------------------------------------------------------------ backward
def make_dout(pr):
    return torch.randn(pr.B * pr.N, pr.D, device="cuda", generator=_gen(77 + pr.N + pr.hd)).bfloat16()


def backward_reference(pr, dout, own):
    """fp64 autograd of the forward formula for dout, and the allowances of dq | dk | dv (module docstring)."""
    B, H, N, hd, D, scale = pr.B, pr.H, pr.N, pr.hd, pr.D, pr.scale
    x = pr.qkv.double().requires_grad_(True)
    t = x.reshape(B, N, 3, H, hd)
    q, k, v = (t[:, :, i].transpose(1, 2) for i in range(3))
    S = scale * (q @ k.transpose(-1, -2))
    e = torch.exp(S - S.max(-1, keepdim=True)[0]) * pr.keep
    P = (e + EPS / pr.nref) / (e.sum(-1, keepdim=True) + EPS)
    merge_heads(P @ v).backward(dout.double())
    ref = x.grad
    dO = split_heads(dout.double(), B, H, N, hd)
    q, k, v, P, zinv, Oh = pr.q, pr.k, pr.v, pr.P, pr.zinv, pr.O
    g = dO @ v.transpose(-1, -2)
    delta = (dO * Oh).sum(-1, keepdim=True)
    p = pr.e * zinv
    dS = p * (g - delta)
    gm = (zinv * (g * (P * pr.Z - pr.e)).sum(-1, keepdim=True)).abs() * (pr.S == pr.m)
    a_in = (pr.a_O + 2.0 ** -8 * (Oh.abs() + pr.a_O)) if own else half_ulp_bf16(Oh)
    a_delta = (dO.abs() * a_in).sum(-1, keepdim=True) + (hd + 8) * U * (dO.abs() * Oh.abs()).sum(-1, keepdim=True)
    a_g = (hd + 8) * U * (dO.abs() @ v.abs().transpose(-1, -2))
    r_p = pr.r_e + 4 * U + 4 * U * torch.log(zinv).abs() + pr.r_log + (pr.r_z if own else 0.0)
    flush = FLUSH * zinv.clamp_min(1.0)                             # on p: exp2 of the one-pass kernel is multiplied by zinv, the streaming one's is p
    a_dS = p * (a_g + a_delta + 2 * U * (g.abs() + delta.abs())) + dS.abs() * (r_p + U) + flush * (g - delta).abs() + gm
    tds = a_dS + half_ulp_bf16(dS.abs() + a_dS) + (N + 8) * U * dS.abs()
    dQ, dK = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q)
    a_dQ = scale * (tds @ k.abs()) + 2 * U * dQ.abs()
    a_dK = scale * (tds.transpose(-1, -2) @ q.abs()) + 2 * U * dK.abs()
    a_P = P * (r_p + 3 * U) + flush
    a_dV = (a_P + half_ulp_bf16(P + a_P) + (N + 8) * U * P).transpose(-1, -2) @ dO.abs()
    return ref, torch.cat([merge_heads(a_dQ), merge_heads(a_dK), merge_heads(a_dV)], dim=1)


def run_backward(tag, pr, dout, out_in, rowmax, zinv):
    B, H, N, D = pr.B, pr.H, pr.N, pr.D
    qkv, out_in, dout = poisoned(pr.qkv), poisoned(out_in), poisoned(dout)
    runs = []
    for _ in range(2):
        dqkv, delta = sentinel(B * N, 3 * D, torch.bfloat16), sentinel(B * H * N)
        call("ppf_attn_bwd", qkv, out_in, dout, dqkv, pr.pol, rowmax, zinv, delta, B, H, N, D, pr.self_keep, pr.eps_n)
        runs.append((dqkv, delta))
    torch.cuda.synchronize()
    assert same_bits(runs[0][0], runs[1][0]), f"{tag}: two runs differ"
    dqkv, delta = runs[0]
    assert all_sentinel(delta[B * H * N:]), f"{tag}: delta written past its end"
    got = inner(tag, "dqkv", dqkv, B * N)
    assert not bool((got.view(torch.int16) == bits(torch.tensor([SENT], dtype=torch.bfloat16)).item()).any()), f"{tag}: a column of dqkv was not written"
    return got


def check_backward(tag, pr, own, mx):
    D = pr.D
    dout = make_dout(pr)
    if own:
        f = run_forward(tag, pr, "ppf_attn_fwd")
        n = pr.B * pr.H * pr.N
        rowmax, zinv = sentinel(n), sentinel(n)
        rowmax[:n], zinv[:n] = f.rowmax.reshape(-1), f.zinv.reshape(-1)
        out_in = f.out.clone()
    else:
        rowmax, zinv = ref_stats(pr)
        out_in = bf16_rne(merge_heads(pr.O)).bfloat16()
        assert torch.equal(out_in.double(), bf16_rne(merge_heads(pr.O)))
    got = run_backward(tag, pr, dout, out_in, rowmax, zinv)
    ref, a = backward_reference(pr, dout, own)
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * D, (i + 1) * D)
        check_bf16(tag, name, got[:, sl], ref[:, sl], a[:, sl], mx)


def bwd_route(hd, N):
    nt = next(t for t in (1, 2, 4, 7) if (N + 31) // 32 <= t)
    return f"{'stream' if hd == 64 else 'onepass'}<{hd},{nt}>"


@pytest.mark.parametrize("mode", ["no-policy", "policy", "policy-own-forward"])
@pytest.mark.parametrize("N", [17, 33, 65, 129, 224])
@pytest.mark.parametrize("hd", [32, 48, 64])
def test_attn_bwd(hd, N, mode):
    pr = problem("random", 2, 2, N, hd, "none" if mode == "no-policy" else "rand", 1, 0)
    tag = f"ppf_attn_bwd {bwd_route(hd, N)} N={N} {mode}"
    mx = Maxima(pr.ref_u)
    check_backward(tag, pr, mode.endswith("own-forward"), mx)
    report(f"attn_bwd[{hd}-{N}-{mode}]", **mx)


@pytest.mark.parametrize("case", ["odd-items", "three-rounds"])
def test_attn_bwd_walks_several_items(case):
    """Workgroups of the persistent streaming kernel that walk more than one (sample, head) item, prefetching item i + 1 under the stores
    of item i: the slot count is CUs x min(160 KiB / lds, 8 / NT) as in the launch code -- one per CU at NT = 7 and NT = 4."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if case == "odd-items":              # CUs + 1 items on CUs slots: two rounds, (CUs + 1) / 2 rounded up workgroups, the last walks one item
        B, H, N = cus + 1, 1, 129
    else:                                # 2 CUs + 8 items: three rounds, the last workgroups walk two items
        B, H, N = (2 * cus + 8 + 7) // 8, 8, 97
    lds = {7: 2 * 28672 + 7 * 8192 + 7 * 4096 + 3 * 7 * 128, 4: 2 * 16384 + 4 * 8192 + 4 * 4096 + 3 * 4 * 128}[7 if N > 128 else 4]
    slots = cus * max(1, min(160 * 1024 // lds, 8 // (7 if N > 128 else 4)))
    assert B * H > slots, "this shape no longer makes a workgroup walk two items"
    pr = problem("random", B, H, N, 64, "rand", 1, 0)
    tag = f"ppf_attn_bwd {bwd_route(64, N)} B={B} H={H} N={N}"
    mx = Maxima(pr.ref_u)
    check_backward(tag, pr, False, mx)
    report(f"attn_bwd_walk[{case}]", **mx)


# ------------------------------------------------------------------------------------------------ input families
FAMILIES = {"allneg": ("allneg", "none", 1, 0), "maskedmax": ("maskedmax", "rand", 1, 0), "zero-nokeep": ("random", "zero", 0, 0),
            "zero-selfkeep": ("random", "zero", 1, 0), "eps_n": ("random", "rand", 1, 197), "onehot-eps_n": ("onehot", "none", 1, 197)}
FAMILY_CASES = [(f, hd, N) for f in FAMILIES for hd, N in FAMILY_SHAPES if not (FAMILIES[f][3] and N >= 197)]


@pytest.mark.parametrize("family,hd,N", FAMILY_CASES)
def test_attn_input_families(family, hd, N):
    data, polkind, self_keep, eps_n = FAMILIES[family]
    pr = problem(data, 2, 2, N, hd, polkind, self_keep, eps_n)
    tag = f"{family} hd={hd} N={N}"
    # the family is what it claims to be, and its known answers, on the reference
    if family == "allneg":
        assert float(pr.S.max()) < -1.0
    elif family == "maskedmax":
        for b in range(pr.B):
            j = jstar_of(b, N)
            rows = torch.arange(N, device="cuda") != j
            kept = (pr.S[b] - 1e30 * (1.0 - pr.keep[b]))[:, rows].max(-1)[0]
            assert float((pr.S[b][:, rows, j] - kept).min()) >= 30.0 and float(pr.Z[b][:, rows].max()) < 1e-12
    elif family == "zero-nokeep":
        assert float(pr.Z.abs().max()) == 0.0
        assert bool(((pr.P - 1.0 / pr.nref).abs() <= 1e-12 / pr.nref).all())
        want = pr.v.sum(-2, keepdim=True) / pr.nref
        assert bool(((pr.O - want).abs() <= 1e-12 * pr.v.abs().sum(-2, keepdim=True) / pr.nref).all())
    elif family == "zero-selfkeep":
        off = 1.0 - torch.eye(N, dtype=torch.float64, device="cuda")
        assert float((pr.e * off).abs().max()) == 0.0
    elif family == "onehot-eps_n":
        c = EPS / 197
        want = torch.full((pr.B, N, N), c / (1 + EPS), dtype=torch.float64, device="cuda")
        want[:, :, 5] = (1 + c) / (1 + EPS)
        assert bool(((pr.hm - want).abs() <= 1e-12 * want).all()) and bool(((pr.zinv - 1 / (1 + EPS)).abs() <= 1e-12).all())
    mx = Maxima(pr.ref_u)
    two = run_forward(tag, pr, "ppf_attn_fwd")
    check_forward(tag + " ppf_attn_fwd", pr, two, False, mx)
    if hd == 64 and N <= 208:
        route, tail = fwd16_route(N, pr.pol is not None)
        check_forward(f"{tag} ppf_attn_fwd_hm {route}", pr, run_forward(tag, pr, "ppf_attn_fwd_hm"), tail, mx)
    check_map(tag + " ppf_attn_headmean", pr, run_headmean(tag, pr, *ref_stats(pr)), mx)
    check_backward(f"{tag} ppf_attn_bwd {bwd_route(hd, N)}", pr, False, mx)
    report(f"attn_family[{family}-{hd}-{N}]", **mx)


# ------------------------------------------------------------------------------------------------ refusals
def test_attn_refusals():
    """Every documented refusal returns its code with an error string that names the entry point, and launches nothing."""
    from protopformer_amd import _lib
    B, NMAX, DMAX = 2, 232, 128
    rows, stats = B * NMAX, B * 4 * NMAX
    qkv = poisoned(torch.zeros(rows, 3 * DMAX, dtype=torch.bfloat16, device="cuda"))
    zeros = poisoned(torch.zeros(rows, DMAX, dtype=torch.bfloat16, device="cuda"))
    pol = torch.ones(B, NMAX, device="cuda")
    out, dqkv = sentinel(rows, DMAX, torch.bfloat16), sentinel(rows, 3 * DMAX, torch.bfloat16)
    rowmax, zinv, delta, hm = sentinel(stats), sentinel(stats), sentinel(stats), sentinel(rows * NMAX)
    st_in = torch.ones(stats, device="cuda")

    def fwd(N=64, H=2, D=128, qkv=qkv, rowmax=rowmax, zinv=zinv):
        return ("ppf_attn_fwd", qkv, out, pol, rowmax, zinv, B, H, N, D, 1, 0)

    def fhm(N=64, H=2, D=128, NP=None, hm=hm, qkv=qkv, rowmax=rowmax, zinv=zinv):
        return ("ppf_attn_fwd_hm", qkv, out, pol, rowmax, zinv, hm, np_of(N) if NP is None else NP, B, H, N, D, 1, 0)

    def hmn(N=64, H=2, D=128, NP=None, qkv=qkv, rowmax=st_in, zinv=st_in):
        return ("ppf_attn_headmean", qkv, pol, rowmax, zinv, hm, np_of(N) if NP is None else NP, B, H, N, D, 1, 0)

    def bwd(N=64, H=2, D=128, qkv=qkv, out_in=zeros, dout=zeros, dqkv=dqkv, rowmax=st_in, zinv=st_in, delta=delta):
        return ("ppf_attn_bwd", qkv, out_in, dout, dqkv, pol, rowmax, zinv, delta, B, H, N, D, 1, 0)

    every = (fwd, fhm, hmn, bwd)
    cases = [("N = 225", ERR_SHAPE, [f(N=225) for f in (fwd, fhm, bwd)]),
             ("N = 0", ERR_SHAPE, [f(N=0) for f in every]),
             ("head_dim 40", ERR_SHAPE, [f(D=80) for f in every]),
             ("D % H != 0", ERR_SHAPE, [f(H=3) for f in every]),
             ("D % 8 != 0", ERR_SHAPE, [f(H=1, D=60) for f in every]),
             ("fwd_hm at head_dim 48", ERR_SHAPE, [fhm(D=96)]),
             ("fwd_hm at N = 209", ERR_SHAPE, [fhm(N=209)]),
             ("NP = N + 4 with N % 4 == 0", ERR_SHAPE, [fhm(NP=68), hmn(NP=68)]),
             ("NP % 4 != 0", ERR_SHAPE, [fhm(N=61, NP=62), hmn(N=61, NP=62)]),
             ("NP < N", ERR_SHAPE, [fhm(NP=60), hmn(NP=60), fhm(N=61, NP=60), hmn(N=61, NP=60)]),
             ("null qkv", ERR_ARG, [f(qkv=None) for f in every]),
             ("null rowmax", ERR_ARG, [f(rowmax=None) for f in every]),
             ("null zinv", ERR_ARG, [f(zinv=None) for f in every]),
             ("null out / dout / dqkv / delta", ERR_ARG, [bwd(out_in=None), bwd(dout=None), bwd(dqkv=None), bwd(delta=None)])]
    for what, rc, calls in cases:
        for args in calls:
            with pytest.raises(RuntimeError, match=rf"rc={rc}\): {args[0]}\b"):
                call(*args)
    lib = _lib.lib()
    assert [lib.ppf_attn_fwd_hm_supported(2, N, D) for N, D in ((208, 128), (209, 128), (64, 96), (0, 128))] == [1, 0, 0, 0]
    torch.cuda.synchronize()
    for name, buf in (("out", out), ("dqkv", dqkv), ("rowmax", rowmax), ("zinv", zinv), ("delta", delta), ("headmean", hm)):
        assert all_sentinel(buf), f"a refused call wrote {name}"
    call(*fwd())                                                    # the argument builders are sound: the unchanged call is accepted
    torch.cuda.synchronize()
    assert not all_sentinel(out)
