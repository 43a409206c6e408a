"""Every instantiation behind the four entry points of csrc/proto.hip (ppf_proto_fwd, ppf_proto_bwd, ppf_proto_bwd_rows, ppf_proto_bwd_single)
against an fp64 reference, at the smallest shapes that reach it, called through the C ABI (refusals, strides with slack, null maps and short
workspaces cannot be expressed through ops).  B = 2 and P odd unless stated: the 16-byte / scalar store branch of the map epilogue and the
alignment branch of the mark kernel then differ between the two samples.

Routes, how they are reached, and what is gated there:
  ppf_proto_fwd       proto_fwd6_kernel<TT, true, PRE> (Dp % 16 == 0) and proto_fwd_kernel<TT, true> (else), TT = 1 .. 4: T = 2, 31, 32, 33, 64, 65, 96,
                      97, 127, 128 at Dp = 48 / 20, with the pre-split planes (PRE) and with a NULL workspace; contraction lengths Dp = 16, 48, 64, 80,
                      192, 384, 400 (split-bf16: one 16-step, a partial 64-chunk, whole chunks, 400 = six chunks and one 16-step) and 4, 20, 36, 100
                      (fp32 MFMA: a partial 32-chunk, one chunk and a part), each at T = 33, 128 and 1; P = 1, 15, 16, 17, 31, 33, 127, 128, 129, 145,
                      257 at T = 9 and T = 1 (np < 16, np <= 0, whole waves past P, a second workgroup column); <2, false, false> at B = 1, 63, 64, 65,
                      130 with the maps in their [B][P] layout; the four null combinations of dist_full / act_full; t0 = 0, 1, 3 with two slack rows
                      per sample; the workspace exact, one byte short and misaligned by 4 bytes; act_kind 1 and eps = 1e-3: dist_full, act_full,
                      act_max, argmax
  ppf_proto_bwd       dense g_full (+ g_max): proto_bwd_mark_kernel (both alignment branches, isolated entries, exact zeros inside dense rows),
                      proto_bwd_tokens_kernel<NJ, 1> and proto_bwd_protos_kernel<NJ>, NJ = 1, 2, 3, 4, 6, 8: Dp = 4, 64, 68, 128, 132, 192, 196, 256,
                      260, 320, 384, 388, 512 (and 6, reference-fed: the forward refuses it) at T = 5, P = 33; proto_bwd_tokens_kernel<1, 8> at P = 2048
                      (still NW = 1: W = 64), 2049, 4100, 8192 with gradients in the first and the last word of every wave's range at bits 0 and 31 and at
                      prototype P - 1; the block loop of proto_bwd_protos_kernel at (B, T) = (128, 128) (exactly one block) and (129, 128) (a second
                      block of 128 elements) with gradients in the first and the last element of each block: dtok, dprotos
  g_max only / rows   proto_bwd_mark_sparse_kernel, proto_bwd_protos_tiled_kernel<NJ, 16> and proto_bwd_protos_rows_kernel<NJ> at NJ = 1, 2, 3, 4, 6 (Dp = 4,
                      64, 68, 128, 132, 192, 196, 256, 260, 320, 384; 388 and 512: the gather kernel reads g_rows at NJ = 8); the tiled kernel
                      with and without the XCD remap ((B, P) = (8, 40), (16, 257),
                      (32, 4097) with; (5, 40), (40, 4097) without: pt = 17, three samples per group, the last group short), one, two and three LDS
                      images (T = 50, 51, 101, 128 at Dp = 384) and the 32-byte image (Dp = 4, T = 2), proto_bwd_protos_rows_kernel<NJ> (ppc = 1, 10, 16;
                      its three-per-lane window at r0 = 51), proto_bwd_protos_finish_kernel, ppc = 17 (the gather kernel), labels with two samples of
                      one class, a class without a sample and the last class, rows with and without g_max, dtok only / dprotos only / both, a
                      workspace that holds the bitmap only: dtok, dprotos
  ppf_proto_bwd_single  B = 1, 63, 65 x P = 1, 63, 64, 65, 257 x Dp = 4, 48, 100, both activation kinds, dtok only / dprotos only: dtok, dprotos
  refusals            T = 0, T = 129, Dp = 6, B = 0, P = 0, null tok / protos / act_max, null argmax at T > 1 (forward); Dp = 516, P = 8193, dtok with a
                      null or short workspace, ppc = 0, ppc > P, T = 1 for the rows form, null g_rows / labels, g_max without argmax at T > 1, a short
                      workspace of the single-token form: the documented code, an error string naming the entry point, outputs still all-sentinel
Unreachable through the C ABI: proto_bwd_protos_tiled_kernel / proto_bwd_protos_rows_kernel at NJ = 8 -- proto_tiled_geometry refuses Dp > 384
(`if (T < 2 || Dp % 4 || Dp > 384 || ...) return g;`), and `if constexpr (NJ <= 6)` in proto_bwd_launch compiles them out.

Poison and sentinels, every call: the token rows outside [t0, t0 + T) -- the class-token rows, the slack rows between samples -- hold NaN; every
output carries 16 elements of a sentinel bit pattern behind it that must survive bit for bit; the maps, act_max, argmax and dtok are prefilled
with the sentinel, none may be left inside and everything inside is finite; dtok rows outside [t0, t0 + T) keep the sentinel; dprotos is
prefilled with multiples of 2**-6 (it is accumulated).  Every call runs twice: bit-identical.

Reference: fp64 torch on the device from the fp32 inputs converted exactly: d = sum_k (x_k - p_k)**2, a = log((d + 1) / (d + eps)) or -d with eps
the fp64 value of the fp32 argument, max over tokens through an explicit index (the smallest index of the maximum).  Backward in closed form:
G = g da/dd (0 where d <= 0), dtok[b, t] = sum_p 2 G (x - p), dprotos[p] += sum_{b, t} 2 G (p - x), g = g_full + g_rows + g_max at the arg-max
index.  Every family is checked once against oracle.ppf_oracle.proto_activations and its autograd in fp64 (the maximum gathered at the reference
index, so exact ties do not depend on autograd's choice).

Input families (generated on the host: the same numbers on every machine):
  A  dyadic     multiples of 2**-6 in [0, 1): for Dp <= 512 every partial sum of |x|**2, |p|**2, x.p and lx2 + (-2 acc + p2) is a multiple of 2**-12
                below 2**10, exact in fp32 in any order, so dist_full must EQUAL the reference bit for bit in both kernels, with and without the
                planes.  Planted: a prototype equal to a token (d = 0), one coordinate off by 2**-6 (d = 2**-12 = 2.4 eps), by 2**-5 (d = 2**-10), two
                coordinates off by 2**-6 (d = 2**-11).  No distance is excluded anywhere in this file
  B  sparse     1 to 3 non-zero coordinates per row, full 24-bit significands, both signs, magnitudes 2**-6 .. 2**4, at the position classes of the
                contraction (first, last, both sides of every 16-step of the first 64-chunk, the 32-chunk boundary, the start of the partial last
                chunk); the first at a coordinate all rows of the case share, the others at most 2**-1 (sparse_rows: otherwise a prototype sees
                many tokens at nearly its own norm and a tenth of the pairs are near-ties of the maximum); the accumulation terms of the gate
                count the non-zeros of the pair, so the gate is a few u of |x| |p|
  C  dense      rand in (0, 1) (what the add-on sigmoid produces), randn, 8 randn: the worst-case gate with Dp + 8 terms (coverage, not sharpness)
  D  ties       bit-identical token rows (2, 6) (the lower index in half-wave 0), (6, 9) (in half-wave 1), (5, 37) (across tiles, one lane), (0, T - 1),
                one pair per sample, each with a prototype 2**-6 off the row: argmax is the smaller index exactly
In A and C with B >= 2 and Dp >= 16 prototype j takes coordinate k from one token of sample k mod B (a prototype bank after projection consists
of tokens): every (sample, prototype) pair then has a winner at about half the distance of the rest, which keeps near-ties of the maximum rare.

Gates, u = 2**-24, every scale from the fp64 reference; n = Dp (A, C) or the non-zeros of the row / pair (B):
  distance    |x|**2 and |p|**2 are fp32 sums of n terms: (n + 8) u of the sum each (any order, the convention of the GEMM file); the contraction
              (n + 8) u s, s = sum_k |x_k| |p_k|, + 3 u s for the piece products the split drops (kernel comment: below 3 * 2**-24 |x| |p|); times 2;
              lx2 + (-2 acc + p2) rounds twice: 2 u (|x|**2 + 2 s + |p|**2).  The relu keeps the bound (d >= 0).  Family A: equality
  activation  a is monotone in d: the kernel's value lies in [a(d + a_d) - w_a, a(max(d - a_d, 0)) + w_a], w_a = 3 u (d + 1, d + eps and the division
              are one rounding each, relative in the ratio = absolute in the log) + r_log max(|a|, 1); kind 1: [-(d + a_d), -max(d - a_d, 0)] exactly.
              r_log = 4 x the worst error of a plain fp32 torch log((d + 1) / (d + eps)) against fp64 on the same fp32 arguments, relative to
              max(|a|, 1), and at least 4 u (two ulp; where torch happens to be exact); reported as log_ref_u -- reference against reference
  derivative  map_is_act = 0: da/dd = 1 / (d + 1) - 1 / (d + eps) is increasing in d: the interval of the fed distance (fp32(d): u d; the forward's
              own map: a_d), the clipped 0 included when d - a_d <= 0, widened by w_D = 2 u / (d + 1) + 2 u / (d + eps) + u |da/dd| (an addition and
              a reciprocal each, the subtraction).  map_is_act = 1: da/dd = -(E - 1)**2 / ((1 - eps) E), E = e**a, is decreasing in a with relative
              slope (E + 1) / (E - 1) -- the term the comment of dact_from_act derives -- so it is evaluated over the interval of the fed
              activation (fp32(a): u |a|; the forward's own: the activation gate), the clipped 0 included when the interval reaches
              a(0) - w_a, widened by (3 r_exp + 6 u) |da/dd|; r_exp = 4 x fp32 torch expm1 against fp64 on the same arguments (at least 4 u),
              reported as exp_ref_u.  Reference-fed with map_is_act = 1 a planted d = 0 pair may take either branch (fp32(log(1 / eps)) against
              the kernel's own threshold): its entries get the wide interval [da/dd(a(0)), 0]; forward-fed the comment of dact_from_act promises
              bit-equality with the forward's value at d = 0, so on family A (where the distance is exactly 0) the coefficient must be exactly 0
  arg-max     the kernel's index i is accepted when a_i + r_i >= max_t (a_t - r_t), r the activation gate; act_max must be the map's value at i
              bit for bit and inside the activation interval at i; the reference backward is routed through i.  On A and D the index must also be
              the smallest of the tokens with exactly its distance (equal distances give bit-equal activations); that makes it the smallest index
              of the minimal d wherever the gate separates the two smallest distances, the planted pairs included.  Near-ties: a pair (b, p)
              counts when a token with ANOTHER distance than the best has a_t + r_t >= a_best - r_best; counted on the reference and asserted
              to be at most 1 % of the pairs of every case (NEAR_TIE_CAP)
  gradients   G = g da/dd: a_G from the interval above + 3 u |G| (the sum of up to three gradients, the product); every term 2 G (x - p) rounds
              three times; the accumulation (n_terms + 8) u sum |2 G (x - p)|, n_terms = the non-zero candidates of that output row on the
              reference (any tree of n non-zero leaves has at most n - 1 rounding additions): a = sum 2 a_G |x - p| + (n_terms + 11) u sum 2 |G|
              |x - p|.  The tiled / single-token forms 2 (sum G) p - 2 sum G x cancel: |x - p| becomes |x| + |p| in the rounding term, and the group
              partials are covered by the + 8.  dprotos: + u (|prefill| + |result|) for the accumulation into the prefill
  two routes  the bitmap-only workspace (gather) against the tiled result, the short / misaligned forward workspace against the planes: both
              within their gate of the reference, so within the sum of the gates of each other; bit-identical dist on family A
No gate is set from the output of a kernel under test.

Measured maxima on an MI355X (helpers.report: the worst error as a fraction of its gate, per route and family A / B / C; dist on A and D: equal):
  ppf_proto_fwd         tiles: act 0.27 / - / 0.19, dist - / - / 0.084;  contraction: act 0.27 / 0.83 / -, dist - / 0.24 / - (0.83: Dp = 64, T = 128 has
                        a pair at d = 3.6e-9 < a_d = 4.4e-7; its interval is cut off at d = 0 and the fraction is taken of the shorter side);  P edges: act 0.24;
                        T = 1: act 0.25 / - / 0.07, dist - / - / 0.074;  layout: act 0.19 / 0.19 / -, dist - / 0.18 / -;  workspace: dist - / 0.24 /
                        0.023, fallbacks against the planes 0 / 0.095 / 0.013;  families: dist - / 0.28 / 0.062, act - / 0.20 / 0.17;
                        kind 1, eps 1e-3: act 0.18 / - / 0.073;  ties: act 0.18;  null combinations: bit-identical
  ppf_proto_bwd dense   every NJ: dtok 0.19 / 0.41 / -, dprotos 0.49 / 0.48 / -;  token-kernel width: dtok 0.12 / 0.13 / -, dprotos 0.43 / 0.50 / -;
                        mark: dtok 0.22 / - / 0.37, dprotos 0.48 / - / 0.50;  block loop: dtok 0.15 / - / 0.17, dprotos 0.007 / - / 0.021
  g_max only / rows     every NJ: dtok 0.40 / 0.44 / -, dprotos 0.50 / 0.48 / -;  grid mapping: dtok 0.24 / - / 0.36, dprotos 0.37 / - / 0.48;
                        LDS chunks: dtok 0.34 / - / 0.38, dprotos 0.50 / - / 0.50;  classes: dtok 0.30 / - / 0.40, dprotos 0.38 / - / 0.34;
                        bitmap-only workspace: dprotos 0.45 / - / 0.46, against the tiled result 0.23 / - / 0.32;  separate calls: bit-identical
  ppf_proto_bwd_single  B = 1: dtok 0.026 / 0.066 / 0.17, dprotos 0.79 / 0.63 / 0.91;  B = 63: dtok 0.15 / 0.40 / 0.40, dprotos 0.049 / 0.52 / 0.15;
                        B = 65: dtok 0.12 / 0.40 / 0.41, dprotos 0.036 / 0.47 / 0.13
  (dprotos near 0.5: rows with one or no term, where the gate is the u (|prefill| + |result|) of the accumulation and round-to-nearest's
  worst case is half of it; 0.91: B = 1, one term per prototype through two products and the fix-up.)
  reference against reference: log <= 3.9 u max(|a|, 1), expm1 <= 1.8 u relative: r_log <= 15.5 u, r_exp <= 7.2 u
  near-ties on the reference: 0 in every case but the 8 x randn cases at P = 129 (1 of 258 pairs; cap 2); no pair left the reference arg-max
The whole file runs in 8.0 s (326 tests; the slowest, the first, 1.1 s with the library load; 0.23 s at P = 8192);
test_gpu_attention_paths.py on the same machine: 5.1 s (220 tests).

The gates bite: value-only edits of proto.hip (scratch builds, nothing committed; no address, bound or launch geometry changes), each run
against this file and against the prototype tests of test_gpu_head.py (-k proto: 37 tests) as they stand:
fail here, pass there:
  3. `a > best` -> `a >= best` (epilogue)                          -> 14 tests: test_fwd_argmax_ties x 8, and the backward cases whose own forward has
                                                                      tokens at exactly equal distances (block loop x 2, grid mapping x 3, P = 8192)
  4. `oi < besti` -> `oi > besti` (half-wave merge)                -> 9 tests: test_fwd_argmax_ties x 8, the block loop at B = 128
  5. `d <= 0.f` -> `d < 0.f` in dact_dd                            -> 35 tests: the forms that cancel (tiled, single-token: 2 G p - 2 G x with
                                                                      G = -g / eps at the planted d = 0) -- the direct forms multiply by x - p = 0
  6. `(1.0f - eps)` -> `1.0f` in dact_from_act                     -> 87 tests: every backward case fed activations
  7. the eight-wave reduction sums seven partials                   -> 5 tests: test_bwd_token_kernel_width P = 2049, 4100, 8192 and (32 | 40, 4097)
  8. gather gradient x (1 + 2**-10) where blk0 > 0                  -> 1 test: test_bwd_gather_block_loop[129]
fail in both files:
  1. the `xb * pb` piece product dropped                            -> 52 tests here (family B: contraction lengths, layout, workspace, and the
                                                                      backward cases fed by the own forward); there test_proto_fwd_golden_and_kat
  2. |x|**2 from the first bf16 piece only                          -> 115 tests here; 23 there
  9. finish kernel: sgv from the first sample group only            -> 39 tests here (every tiled case with more than one group); there
                                                                      test_proto_bwd_block_rows_vs_oracle x 5
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import SENT, U, bits, report

pytestmark = pytest.mark.gpu

DEV = "cuda" if torch.cuda.is_available() else "cpu"
ERR_SHAPE, ERR_ARG = -1, -3
PAD = 16                                 # sentinel elements behind every output
ISENT = 0x5A5A5A5A                       # sentinel of the int32 arg-max
NEAR_TIE_CAP = 0.01


# ------------------------------------------------------------------------------------------------ inputs
def position_classes(Dp):
    """Where the contraction can lose a term: first / last element, both sides of every 16-step of the first 64-chunk, the 32-chunk boundary of
    the fp32 kernel, the start and the end of the partial last chunk."""
    c = {0, 1, 3, 4, 15, 16, 31, 32, 33, 47, 48, 63, 64, 65, Dp - 1, Dp - 2, Dp - 4, Dp - 5, Dp - 16, Dp - 17, (Dp - 1) // 64 * 64, (Dp - 1) // 32 * 32,
         (Dp - 1) // 16 * 16}
    return sorted(k for k in c if 0 <= k < Dp)


def full_significand(n, g, top=4.0):
    """n fp32 values with both signs, magnitudes 2**-6 .. 2**top and (almost surely) all 24 bits of the significand in use."""
    mag = torch.exp2(torch.rand(n, generator=g, dtype=torch.float64) * (top + 6.0) - 6.0)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def sparse_rows(n, Dp, g, shift):
    """Row i: one non-zero of magnitude 2**-6 .. 2**4 at a coordinate every row of the case shares, and (i + shift) % 3 more of magnitude
    2**-6 .. 2**-1 walking the position classes.  (Disjoint supports, or a prototype with a large coordinate that no token has, put many
    tokens at nearly the prototype's own norm: distances of 100 that differ by 1e-3, activations that differ by 1e-7 -- near-ties of the
    maximum at a tenth of the pairs.  With the large values on the shared coordinate the nearest token is decided there.)"""
    cls = position_classes(Dp)
    common = cls[(Dp // 4) % len(cls)]
    out = torch.zeros(n, Dp)
    for i in range(n):
        out[i, common] = full_significand(1, g)[0]
        for j in range((i + shift) % 3):
            k = cls[(i // 3 + 5 * j + shift) % len(cls)]
            if k != common:
                out[i, k] = full_significand(1, g, -1.0)[0]
    return out


def make_inputs(family, B, T, P, Dp, seed):
    """x [B][T][Dp], protos [P][Dp] fp32 on the host, and the tie pairs that were planted (family D)."""
    g = torch.Generator().manual_seed(seed)
    ties = []
    if family in ("A", "D"):
        x = torch.randint(0, 64, (B, T, Dp), generator=g).float() / 64.0
        pro = torch.randint(0, 64, (P, Dp), generator=g).float() / 64.0
    elif family == "B":
        return sparse_rows(B * T, Dp, g, 0).reshape(B, T, Dp), sparse_rows(P, Dp, g, 1), ties
    elif family == "C-rand":
        x, pro = torch.rand(B, T, Dp, generator=g), torch.rand(P, Dp, generator=g)
        x, pro = x.clamp_min(2.0 ** -24), pro.clamp_min(2.0 ** -24)
    elif family in ("C-randn", "C-randn8"):
        s = 8.0 if family.endswith("8") else 1.0
        x, pro = torch.randn(B, T, Dp, generator=g) * s, torch.randn(P, Dp, generator=g) * s
    else:
        raise ValueError(family)
    if B >= 2 and Dp >= 16 and T > 1:                  # prototype j: coordinate k from token tsel[j][k % B] of sample k % B
        tsel = torch.randint(0, T, (P, B), generator=g)
        kb = torch.arange(Dp) % B
        pro = x[kb[None, :].expand(P, Dp), tsel[:, kb], torch.arange(Dp)[None, :].expand(P, Dp)].clone()
    if family == "D":
        pairs = [(2, 6), (6, 9), (5, 37), (0, T - 1)]
        for b in range(B):
            lo, hi = pairs[b % 4]
            assert hi < T
            x[b, hi] = x[b, lo]
            ties.append((b, lo, hi))
    if family in ("A", "D") and P >= 1:                # close pairs (grid-preserving: step towards the inside of [0, 1))
        def off(row, k, steps):
            row = row.clone()
            row[k] += (steps if row[k] < 0.5 else -steps) / 64.0
            return row
        plants = [x[0, min(1, T - 1)].clone(), off(x[B - 1, T - 1], 0, 1), off(x[0, 0], Dp - 1, 2), off(off(x[B - 1, T // 2], 1 % Dp, 1), Dp - 2, 1)]
        if family == "D":                              # one prototype 2**-6 off each tied row
            plants = [off(x[b, lo], (3 * b) % Dp, 1) for b, lo, _ in ties] + plants
        slots = [0, P - 1, P // 2, 1, 2, 3, 4, 5]
        for row, j in zip(plants, dict.fromkeys(s for s in slots if 0 <= s < P)):
            pro[j] = row
    return x, pro, ties


def first_max_index(a):
    """The smallest index of the maximum over the last axis."""
    T = a.shape[-1]
    ar = torch.arange(T, device=a.device).expand_as(a)
    return torch.where(a == a.max(-1, keepdim=True)[0], ar, T).min(-1)[0]


def act_of(d, kind, eps):
    return torch.log((d + 1.0) / (d + eps)) if kind == 0 else -d


def dact_dist(d, kind, eps):
    """da/dd at d > 0 (the limit at d = 0 where d is 0: the caller decides about the clip)."""
    return 1.0 / (d + 1.0) - 1.0 / (d + eps) if kind == 0 else -torch.ones_like(d)


def dact_act(a, eps):
    em1 = torch.expm1(a)
    return -(em1 * em1) / ((1.0 - eps) * (em1 + 1.0))


@functools.lru_cache(maxsize=6)
def problem(family, B, T, P, Dp, t0=0, slack=0, kind=0, eps=1e-4, seed=0):
    """Inputs, the fp64 reference of the forward pass and the quantities its gates are made of (module docstring)."""
    x32, pro32, ties = make_inputs(family, B, T, P, Dp, 7919 * seed + 31 * Dp + 7 * T + 3 * P + B)
    rows = t0 + T + slack
    tok = torch.full((B, rows, Dp), float("nan"))
    tok[:, t0:t0 + T] = x32
    tok, pro32 = tok.to(DEV), pro32.to(DEV).contiguous()
    x, p = tok[:, t0:t0 + T].double(), pro32.double()
    eps64 = float(np.float32(eps))
    d = torch.zeros(B, P, T, dtype=torch.float64, device=DEV)
    step = max(1, (1 << 22) // max(1, P * T * Dp))
    for b0 in range(0, B, step):
        d[b0:b0 + step] = ((x[b0:b0 + step, None] - p[None, :, None]) ** 2).sum(-1)
    a = act_of(d, kind, eps64)
    x2, p2 = (x * x).sum(-1), (p * p).sum(-1)                                   # [B][T], [P]
    s = torch.einsum("btk,pk->bpt", x.abs(), p.abs())
    exact = family in ("A", "D")
    if family == "B":
        nx, npp = (x != 0).sum(-1).double(), (p != 0).sum(-1).double()
        nxp = torch.einsum("btk,pk->bpt", (x != 0).double(), (p != 0).double())
    else:
        nx, npp, nxp = torch.full_like(x2, Dp), torch.full_like(p2, Dp), torch.full_like(s, Dp)
    a_d = ((nx + 8) * U * x2)[:, None, :] + ((npp + 8) * U * p2)[None, :, None] + 2 * (nxp + 8 + 3) * U * s + 2 * U * (x2[:, None, :] + 2 * s + p2[None, :, None])
    if exact:
        a_d = torch.zeros_like(a_d)
        assert bool((d.float().double() == d).all()) and Dp <= 512
    # ---- intrinsics: 4 x a plain fp32 torch evaluation of the same expression against fp64 on the same arguments
    d32 = d.float()
    eps32 = torch.tensor(eps, dtype=torch.float32, device=DEV)
    a64 = act_of(d32.double(), 0, eps64)
    log_ref = float(((torch.log((d32 + 1.0) / (d32 + eps32)).double() - a64).abs() / a64.abs().clamp_min(1.0)).max())
    a32 = a64.float()
    e64 = torch.expm1(a32.double())
    exp_ref = float(((torch.expm1(a32).double() - e64).abs() / e64.abs().clamp_min(1e-300)).max())
    r_log, r_exp = max(4 * log_ref, 4 * U), max(4 * exp_ref, 4 * U)
    w_of = (lambda v: 3 * U + r_log * v.abs().clamp_min(1.0)) if kind == 0 else (lambda v: torch.zeros_like(v))
    d_lo, d_hi = (d - a_d).clamp_min(0.0), d + a_d
    a_hi, a_lo = act_of(d_lo, kind, eps64), act_of(d_hi, kind, eps64)           # a is decreasing in d
    a_hi, a_lo = a_hi + w_of(a_hi), a_lo - w_of(a_lo)
    idx = first_max_index(a)
    # near-ties of the maximum, on the reference alone
    best_lo = a_lo.gather(-1, idx[..., None])
    other = d != d.gather(-1, idx[..., None])
    near = int(((a_hi >= best_lo) & other).any(-1).sum())
    return SimpleNamespace(family=family, exact=exact, B=B, T=T, P=P, Dp=Dp, t0=t0, rows=rows, stride_b=rows * Dp, kind=kind, eps=eps, eps64=eps64,
                           tok=tok, pro=pro32, x=x, p=p, d=d, a=a, a_d=a_d, d_lo=d_lo, d_hi=d_hi, a_lo=a_lo, a_hi=a_hi, idx=idx, ties=ties, near=near,
                           r_log=r_log, r_exp=r_exp, w_of=w_of, ref_u=dict(log_ref_u=log_ref / U, exp_ref_u=exp_ref / U))


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


def check_abs(tag, name, got, ref, bound, mx):
    err = (got.double() - ref).abs().nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(err, bound)})
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{tag}: {name} over its bound at {int(bad.sum())} places (worst {mx[name + '_frac']:.3g} of the bound)"


def check_interval(tag, name, got, lo, hi, mid, mx):
    got = got.double().nan_to_num(nan=math.inf)
    over = torch.where(got >= mid, (got - mid) / (hi - mid).clamp_min(1e-300), (mid - got) / (mid - lo).clamp_min(1e-300))
    over = torch.where(got == mid, torch.zeros_like(over), over)
    mx.up(**{name + "_frac": float(over.max())})
    bad = ~((got >= lo) & (got <= hi))
    assert not bool(bad.any()), f"{tag}: {name} outside its interval at {int(bad.sum())} places (worst {mx[name + '_frac']:.3g} of the half-width)"


def sentinel(n, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full((n + PAD,), ISENT, dtype=torch.int32, device=DEV)
    return torch.full((n + PAD,), SENT, dtype=dtype, device=DEV)


def all_sentinel(t):
    if t.dtype == torch.int32:
        return bool((t == ISENT).all())
    return torch.equal(bits(t), bits(torch.full(t.shape, SENT, dtype=t.dtype)))


def none_sentinel(t):
    if t.dtype == torch.int32:
        return not bool((t == ISENT).any())
    return not bool((bits(t) == bits(torch.tensor([SENT])).item()).any())


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def inner(tag, name, buf, n):
    """The first n elements of an output: its tail still all-sentinel, everything inside written and finite."""
    assert all_sentinel(buf[n:]), f"{tag}: {name} written past its end"
    got = buf[:n]
    assert none_sentinel(got), f"{tag}: an element of {name} was not written"
    assert got.dtype == torch.int32 or bool(torch.isfinite(got).all()), f"{tag}: {name} is not finite"
    return got


def call(name, *args):
    from protopformer_amd import _lib
    _lib.call(name, *args)


def lib():
    from protopformer_amd import _lib
    return _lib.lib()


def scratch(nbytes):
    return torch.zeros(max(int(nbytes), 1) + 16, dtype=torch.uint8, device=DEV)


# ------------------------------------------------------------------------------------------------ forward
def run_fwd(tag, pr, want_dist=True, want_act=True, ws="exact"):
    """ppf_proto_fwd twice: sentinels, finiteness, two runs bit-identical.  ws: 'exact' | 'short' | 'misaligned' | None."""
    B, T, P, Dp = pr.B, pr.T, pr.P, pr.Dp
    need = lib().ppf_proto_fwd_workspace(P, Dp)
    runs = []
    for _ in range(2):
        act_max, argmax = sentinel(B * P), sentinel(B * P, torch.int32)
        dist = sentinel(B * P * T) if want_dist else None
        act = sentinel(B * P * T) if want_act else None
        buf = scratch(need + 16)
        wptr, wbytes = {"exact": (buf.data_ptr(), need), "short": (buf.data_ptr(), need - 1), "misaligned": (buf.data_ptr() + 4, need), None: (None, 0)}[ws]
        call("ppf_proto_fwd", pr.tok, pr.stride_b, pr.t0, T, pr.pro, B, P, Dp, pr.kind, pr.eps, act_max, argmax if T > 1 else None, dist, act, wptr, wbytes)
        runs.append((act_max, argmax, dist, act))
    torch.cuda.synchronize()
    for u, v in zip(*runs):
        assert u is None or same_bits(u, v), f"{tag}: two runs differ"
    act_max, argmax, dist, act = runs[0]
    if T == 1:
        assert all_sentinel(argmax), f"{tag}: argmax written at T == 1"
    return SimpleNamespace(act_max=inner(tag, "act_max", act_max, B * P).reshape(B, P),
                           argmax=inner(tag, "argmax", argmax, B * P).reshape(B, P).long() if T > 1 else torch.zeros(B, P, dtype=torch.long, device=DEV),
                           dist=None if dist is None else inner(tag, "dist_full", dist, B * P * T).reshape(B, P, T),
                           act=None if act is None else inner(tag, "act_full", act, B * P * T).reshape(B, P, T),
                           raw=SimpleNamespace(act_max=act_max, argmax=argmax, dist=dist, act=act))


def check_argmax(tag, pr, idx):
    """The acceptance rule of the module docstring; returns how many pairs did not take the reference index."""
    assert int(idx.min()) >= 0 and int(idx.max()) < pr.T, f"{tag}: argmax outside [0, T)"
    top = (pr.a_lo).max(-1)[0]
    ok = pr.a_hi.gather(-1, idx[..., None])[..., 0] >= top
    assert bool(ok.all()), f"{tag}: argmax points at a token whose activation is below the maximum by more than the gate at {int((~ok).sum())} pairs"
    if pr.exact:
        same = pr.d == pr.d.gather(-1, idx[..., None])
        first = torch.where(same, torch.arange(pr.T, device=DEV).expand_as(same), pr.T).min(-1)[0]
        assert torch.equal(first, idx), f"{tag}: argmax is not the smallest index among tokens of equal distance at {int((first != idx).sum())} pairs"
        for b, lo, hi in pr.ties:                       # the planted prototype of this pair: the tied rows are the maximum
            j = [0, pr.P - 1, pr.P // 2, 1, 2, 3, 4, 5]
            j = list(dict.fromkeys(s for s in j if 0 <= s < pr.P))[pr.ties.index((b, lo, hi))]
            assert int(pr.idx[b, j]) == lo and float(pr.d[b, j, lo]) == float(pr.d[b, j, hi]) == 2.0 ** -12, "the tie is not what it claims to be"
            assert int(idx[b, j]) == lo, f"{tag}: tie ({lo}, {hi}) of sample {b} went to {int(idx[b, j])}"
    moved = int((idx != pr.idx).sum())
    assert pr.near <= NEAR_TIE_CAP * pr.B * pr.P, f"{tag}: {pr.near} near-ties among {pr.B * pr.P} pairs on the reference: choose another seed"
    assert moved <= pr.near, f"{tag}: {moved} pairs left the reference arg-max, the reference has {pr.near} near-ties"
    return moved


def check_fwd(tag, pr, res, mx):
    if res.dist is not None:
        if pr.exact:
            assert same_bits(res.dist, pr.d.float()), f"{tag}: dist_full differs from the exact distances at {int((res.dist.double() != pr.d).sum())} places"
        check_abs(tag, "dist", res.dist, pr.d, pr.a_d, mx)
    if res.act is not None:
        check_interval(tag, "act", res.act, pr.a_lo, pr.a_hi, pr.a, mx)
    if pr.T > 1:
        mx.up(near_ties=pr.near, moved=check_argmax(tag, pr, res.argmax))
    pick = lambda t: t.gather(-1, res.argmax[..., None])[..., 0]
    check_interval(tag, "act_max", res.act_max, pick(pr.a_lo), pick(pr.a_hi), pick(pr.a), mx)
    if res.act is not None:
        assert same_bits(res.act_max, pick(res.act)), f"{tag}: act_max is not the map's value at argmax"


def fwd_case(name, pr, mx=None, **kw):
    mx = Maxima(pr.ref_u) if mx is None else mx
    tag = f"ppf_proto_fwd {name}"
    res = run_fwd(tag, pr, **kw)
    check_fwd(tag, pr, res, mx)
    report(f"proto_fwd[{name}]", **mx)
    return res


@pytest.mark.parametrize("ws", ["planes", "null"])
@pytest.mark.parametrize("family", ["A", "C-randn"])
@pytest.mark.parametrize("Dp", [48, 20])
@pytest.mark.parametrize("T", [2, 31, 32, 33, 64, 65, 96, 97, 127, 128])
def test_fwd_token_tiles(T, Dp, family, ws):
    fwd_case(f"tiles-{T}-{Dp}-{family}-{ws}", problem(family, 2, T, 33, Dp), ws="exact" if ws == "planes" else None)


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("T", [33, 128, 1])
@pytest.mark.parametrize("Dp", [16, 48, 64, 80, 192, 384, 400, 4, 20, 36, 100])
def test_fwd_contraction_lengths(Dp, T, family):
    pr = problem(family, 2, T, 33, Dp, seed=int((family, Dp, T) == ("B", 400, 128)))         # (seed 0 has one near-tie among its 66 pairs)
    fwd_case(f"contraction-{Dp}-{T}-{family}", pr)
    if T == 33:
        fwd_case(f"contraction-{Dp}-{T}-{family}-null", pr, ws=None)


@pytest.mark.parametrize("T", [9, 1])
@pytest.mark.parametrize("P", [1, 15, 16, 17, 31, 33, 127, 128, 129, 145, 257])
def test_fwd_prototype_edges(P, T):
    fwd_case(f"P-{P}-{T}", problem("A", 2, T, P, 16))
    fwd_case(f"P-{P}-{T}-fp32", problem("A", 2, T, P, 20))


@pytest.mark.parametrize("Dp", [16, 20])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_fwd_single_token(B, Dp):
    for family in ("A", "C-rand"):
        pr = problem(family, B, 1, 33, Dp, 1, 1)
        res = fwd_case(f"single-{B}-{Dp}-{family}", pr)
        assert res.dist.shape == (B, 33, 1) and same_bits(res.act[..., 0], res.act_max)


@pytest.mark.parametrize("T,Dp", [(33, 48), (33, 20), (1, 48), (1, 20)])
def test_fwd_output_combinations(T, Dp):
    """A training forward writes act_full only: the four null combinations give the same act_max / argmax and the same maps."""
    pr = problem("C-rand", 2, T, 33, Dp, 1, 0)
    full = fwd_case(f"outputs-{T}-{Dp}-both", pr)
    for want_dist, want_act in ((True, False), (False, True), (False, False)):
        res = fwd_case(f"outputs-{T}-{Dp}-{int(want_dist)}{int(want_act)}", pr, want_dist=want_dist, want_act=want_act)
        assert (res.dist is None) == (not want_dist) and (res.act is None) == (not want_act)
        assert same_bits(res.act_max, full.act_max) and torch.equal(res.argmax, full.argmax)
        assert res.dist is None or same_bits(res.dist, full.dist)
        assert res.act is None or same_bits(res.act, full.act)


@pytest.mark.parametrize("Dp", [48, 20])
@pytest.mark.parametrize("t0", [0, 1, 3])
def test_fwd_layout(t0, Dp):
    """stride_b = (t0 + T + 2) Dp: NaN in the class-token rows and in the slack between samples."""
    for family in ("A", "B"):
        fwd_case(f"layout-{t0}-{Dp}-{family}", problem(family, 3, 40, 33, Dp, t0, 2))
    fwd_case(f"layout-{t0}-{Dp}-single", problem("A", 70, 1, 33, Dp, t0, 2))


@pytest.mark.parametrize("family", ["A", "B", "C-randn8"])
def test_fwd_workspace_fallbacks(family):
    """Too small by one byte and misaligned by four: every workgroup splits its own prototype rows -- the same pieces, |p|**2 in another order."""
    pr = problem(family, 2, 40, 129, 80)
    mx = Maxima(pr.ref_u)
    planes = fwd_case(f"workspace-{family}-exact", pr, mx)
    null = fwd_case(f"workspace-{family}-null", pr, mx, ws=None)
    for ws in ("short", "misaligned"):
        res = fwd_case(f"workspace-{family}-{ws}", pr, mx, ws=ws)
        for k in ("dist", "act", "act_max"):
            assert same_bits(getattr(res, k), getattr(null, k)), f"{ws} workspace: {k} differs from the NULL-workspace run"
        assert torch.equal(res.argmax, null.argmax)
        if pr.exact:
            assert same_bits(res.dist, planes.dist)
        check_abs(f"{ws} against the planes", "dist_vs_planes", res.dist, planes.dist.double(), 2 * pr.a_d, mx)
    report(f"proto_fwd[workspace-{family}]", **mx)


@pytest.mark.parametrize("Dp", [48, 20])
@pytest.mark.parametrize("kind,eps", [(1, 1e-4), (0, 1e-3)])
def test_fwd_activation_kinds(kind, eps, Dp):
    for family in ("A", "C-rand"):
        fwd_case(f"kind-{kind}-{eps}-{Dp}-{family}", problem(family, 2, 40, 33, Dp, 1, 0, kind, eps))
        fwd_case(f"kind-{kind}-{eps}-{Dp}-{family}-single", problem(family, 5, 1, 33, Dp, 0, 0, kind, eps))


@pytest.mark.parametrize("Dp", [64, 36])
@pytest.mark.parametrize("family", ["B", "C-rand", "C-randn", "C-randn8"])
def test_fwd_input_families(family, Dp):
    fwd_case(f"family-{family}-{Dp}", problem(family, 2, 40, 129, Dp, 1, 0))


@pytest.mark.parametrize("ws", ["planes", "null"])
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("Dp", [48, 20])
def test_fwd_argmax_ties(Dp, kind, ws):
    """Bit-identical token rows: each arm of the rule (`a > best` inside a lane, `ob == best && oi < besti` across the half-waves) decides."""
    pr = problem("D", 4, 40, 33, Dp, 1, 0, kind)
    assert [(lo, hi) for _, lo, hi in pr.ties] == [(2, 6), (6, 9), (5, 37), (0, 39)]
    for b, lo, hi in pr.ties:
        assert torch.equal(pr.x[b, lo], pr.x[b, hi])
    fwd_case(f"ties-{Dp}-{kind}-{ws}", pr, ws="exact" if ws == "planes" else None)


def test_fwd_refusals():
    """Every documented refusal returns its code with an error string that names the entry point, and launches nothing."""
    B, T, P, Dp = 2, 9, 33, 16
    tok, pro = torch.zeros(B, 130, 32, device=DEV), torch.zeros(P, 32, device=DEV)
    act_max, argmax, dist, act = sentinel(B * P), sentinel(B * P, torch.int32), sentinel(B * P * 129), sentinel(B * P * 129)

    def fwd(B=B, T=T, P=P, Dp=Dp, tok=tok, pro=pro, act_max=act_max, argmax=argmax):
        return ("ppf_proto_fwd", tok, 130 * 32, 0, T, pro, B, P, Dp, 0, 1e-4, act_max, argmax, dist, act, None, 0)

    cases = [(ERR_SHAPE, [fwd(T=0), fwd(T=129), fwd(Dp=6), fwd(B=0), fwd(P=0), fwd(Dp=0), fwd(T=-1)]),
             (ERR_ARG, [fwd(tok=None), fwd(pro=None), fwd(act_max=None), fwd(argmax=None)])]
    for rc, calls in cases:
        for args in calls:
            with pytest.raises(RuntimeError, match=rf"rc={rc}\): ppf_proto_fwd\b"):
                call(*args)
    torch.cuda.synchronize()
    for name, buf in (("act_max", act_max), ("argmax", argmax), ("dist_full", dist), ("act_full", act)):
        assert all_sentinel(buf), f"a refused call wrote {name}"
    call(*fwd(T=1, argmax=None))                                    # a null argmax is accepted at T == 1
    call(*fwd())                                                    # the argument builder is sound: the unchanged call is accepted
    torch.cuda.synchronize()
    assert none_sentinel(act_max[:B * P]) and none_sentinel(argmax[:B * P])


# ------------------------------------------------------------------------------------------------ backward: reference
def coefficient(pr, is_act, own):
    """The interval [lo, hi] of da/dd the kernel may compute from the map it is fed, its centre (the reference) and the evaluation's own error
    (module docstring: derivative).  own: the forward kernel's maps are fed, else fp32 of the reference."""
    d, eps, kind = pr.d, pr.eps64, pr.kind
    centre = torch.where(d > 0, dact_dist(d, kind, eps), torch.zeros_like(d))
    delta = pr.a_d if own else U * d
    d_lo, d_hi = (d - delta).clamp_min(0.0), d + delta
    clip = d_lo <= 0                                                 # the clipped branch is within reach
    if kind == 1:
        lo, hi, w = torch.where(d_hi > 0, -1.0, 0.0).to(d), torch.where(clip, 0.0, -1.0).to(d), torch.zeros_like(d)
    elif not is_act:
        lo = torch.where(d_hi > 0, dact_dist(d_lo, 0, eps), torch.zeros_like(d))
        hi = torch.where(clip, torch.zeros_like(d), dact_dist(d_hi, 0, eps))
        w = 2 * U / (d_lo + 1) + 2 * U / (d_lo + eps) + U * lo.abs()
    else:
        if own:
            a_lo, a_hi = pr.a_lo, pr.a_hi
        else:
            a_lo, a_hi = pr.a - U * pr.a.abs(), pr.a + U * pr.a.abs()
        a0 = math.log(1.0 / eps)
        reach = a_hi >= a0 - (3 * U + pr.r_log * a0 + U * a0)
        lo = dact_act(a_hi.clamp_max(a0), eps)
        hi = torch.where(reach, torch.zeros_like(d), dact_act(a_lo.clamp_min(0.0), eps))
        w = (3 * pr.r_exp + 6 * U) * lo.abs()
        if own and pr.exact:                                         # bit-equal to the forward's value at d = 0 (comment of dact_from_act)
            z = d == 0
            lo, hi, w = torch.where(z, 0.0, lo), torch.where(z, 0.0, hi), torch.where(z, 0.0, w)
    z = (d == 0) & (delta == 0) & (not is_act or kind == 1)
    lo, hi, w = torch.where(z, torch.zeros_like(lo), lo), torch.where(z, torch.zeros_like(hi), hi), torch.where(z, torch.zeros_like(w), w)
    assert bool((lo <= centre).all()) and bool((centre <= hi).all())
    return centre, lo, hi, w


def pair_sums(pr, G, aG):
    """sum_p and sum_{b, t} of 2 G (x - p), of 2 a_G |x - p|, of 2 (|G| + a_G) |x - p| and of 2 (|G| + a_G) (|x| + |p|) in fp64."""
    B, T, P, Dp = pr.B, pr.T, pr.P, pr.Dp
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=DEV)
    tokq, proq = [z(B, T, Dp) for _ in range(4)], [z(P, Dp) for _ in range(4)]
    Gm = G.abs() + aG
    step = max(1, (1 << 22) // max(1, P * T * Dp))
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        diff = pr.x[sl, None] - pr.p[None, :, None]                # [b][P][T][Dp]
        mag = pr.x[sl, None].abs() + pr.p[None, :, None].abs()
        for q, (coef, v) in enumerate(((G[sl], diff), (aG[sl], diff.abs()), (Gm[sl], diff.abs()), (Gm[sl], mag))):
            term = 2.0 * coef[..., None] * v
            tokq[q][sl] = term.sum(1)
            proq[q] += (-term if q == 0 else term).sum((0, 2))
    return tokq, proq


def backward_reference(pr, g_full, rows, g_max, idx, is_act, own, tiled, tok_cancels=False):
    """(dtok, its gate, dprotos without the prefill, its gate without the prefill's rounding).  tiled / tok_cancels: the prototype / token
    gradients are formed as 2 (sum G) v - 2 sum G w (the tiled kernels; both products of the single-token form)."""
    B, T, P = pr.B, pr.T, pr.P
    g = torch.zeros(B, P, T, dtype=torch.float64, device=DEV)
    if g_full is not None:
        g += g_full.double()
    if rows is not None:
        g_rows, label, ppc = rows
        for b in range(B):
            p0 = int(label[b]) * ppc
            g[b, p0:p0 + ppc] += g_rows[b].double()
    if g_max is not None:
        g.scatter_add_(-1, idx[..., None], g_max.double()[..., None])
    cand = g != 0                                                    # the kernels' candidates: any non-zero upstream entry
    if g_full is not None:
        cand |= g_full != 0
    if g_max is not None:
        cand |= torch.zeros_like(cand).scatter_(-1, idx[..., None], (g_max != 0)[..., None])
    centre, lo, hi, w = coefficient(pr, is_act, own)
    G = g * centre
    aG = torch.maximum((g * lo - G).abs(), (g * hi - G).abs()) + g.abs() * w + 3 * U * g.abs() * torch.maximum(lo.abs(), hi.abs())
    tokq, proq = pair_sums(pr, G, aG)
    n_tok, n_pro = cand.sum(1).double()[..., None], cand.sum((0, 2)).double()[:, None]
    a_tok = tokq[1] + (n_tok + 11 + tok_cancels) * U * (tokq[3] if tok_cancels else tokq[2])
    a_pro = proq[1] + (n_pro + 12) * U * (proq[3] if tiled else proq[2])
    return tokq[0], a_tok, proq[0], a_pro


def make_grads(pr, kind, seed, ppc=0, label=None):
    """Upstream gradients on the host grid of fp32: g_full [B][P][T] | None, g_rows [B][ppc][T] | None, g_max [B][P] | None."""
    g = torch.Generator().manual_seed(seed)
    B, T, P = pr.B, pr.T, pr.P
    out = SimpleNamespace(g_full=None, rows=None, g_max=None)
    if "max" in kind:
        gm = torch.randn(B, P, generator=g)
        gm[torch.rand(B, P, generator=g) < 0.1] = 0.0               # some prototypes without a gradient
        out.g_max = gm.to(DEV)
    if "dense" in kind:
        out.g_full = torch.randn(B, P, T, generator=g).to(DEV)
    if "holes" in kind:                                              # exact zeros inside dense rows
        gf = torch.randn(B, P, T, generator=g)
        gf[torch.rand(B, P, T, generator=g) < 0.3] = 0.0
        out.g_full = gf.to(DEV)
    if "isolated" in kind:
        gf = torch.zeros(B * P * T)
        gf[torch.randperm(B * P * T, generator=g)[:max(3, B * P * T // 50)]] = 1.5
        gf[0], gf[-1] = -0.75, 2.5
        out.g_full = gf.reshape(B, P, T).to(DEV)
    if "rows" in kind:
        out.rows = (torch.randn(B, ppc, T, generator=g).to(DEV), label.to(DEV), ppc)
        if "sparse-rows" in kind:
            out.rows[0][torch.rand(B, ppc, T, generator=g).to(DEV) < 0.5] = 0.0
    return out


def dyadic(shape, seed):
    return (torch.randint(-128, 128, shape, generator=torch.Generator().manual_seed(seed)).float() / 64.0).to(DEV)


def tiled_route(pr, gr, ppc, full_ws):
    """proto_bwd_launch's choice for the prototype gradients (proto_tiled_geometry and the conditions behind it)."""
    return (gr.g_full is None and pr.T >= 2 and pr.Dp % 4 == 0 and pr.Dp <= 384 and pr.stride_b % 4 == 0 and (pr.t0 * pr.Dp) % 4 == 0
            and (gr.rows is None or ppc <= 16) and full_ws)


def run_bwd(tag, pr, gr, fmap, is_act, idx, want_tok=True, want_pro=True, ws="full", dslack=1):
    """ppf_proto_bwd / ppf_proto_bwd_rows twice: sentinels around and between the dtok rows, the dyadic prefill of dprotos, bit-identical runs."""
    B, T, P, Dp, t0 = pr.B, pr.T, pr.P, pr.Dp, pr.t0
    drows = t0 + T + dslack
    full = lib().ppf_proto_bwd_workspace(B, T, P, Dp, int(want_tok), int(want_pro))
    bitmap = lib().ppf_proto_bwd_workspace(B, T, P, Dp, int(want_tok), 0)
    nbytes = full if ws == "full" else bitmap
    pre = dyadic((P, Dp), 5 + P + Dp)
    idx32 = None if idx is None else idx.int().contiguous()
    runs = []
    for _ in range(2):
        dtok = sentinel(B * drows * Dp) if want_tok else None
        dpro = sentinel(P * Dp) if want_pro else None
        if want_pro:
            dpro[:P * Dp] = pre.reshape(-1)
        wbuf = scratch(nbytes)
        wargs = (wbuf, nbytes) if nbytes else (None, 0)
        if gr.rows is None:
            call("ppf_proto_bwd", pr.tok, pr.stride_b, t0, T, pr.pro, B, P, Dp, pr.kind, pr.eps, fmap, int(is_act), gr.g_full, gr.g_max, idx32, dtok, drows * Dp,
                 dpro, *wargs)
        else:
            call("ppf_proto_bwd_rows", pr.tok, pr.stride_b, t0, T, pr.pro, B, P, Dp, pr.kind, pr.eps, fmap, int(is_act), gr.rows[0], gr.rows[1], gr.rows[2],
                 gr.g_max, idx32, dtok, drows * Dp, dpro, *wargs)
        runs.append((dtok, dpro))
    torch.cuda.synchronize()
    for u, v in zip(*runs):
        assert u is None or same_bits(u, v), f"{tag}: two runs differ"
    dtok, dpro = runs[0]
    out = SimpleNamespace(dtok=None, dpro=None, pre=pre.double())
    if want_tok:
        assert all_sentinel(dtok[B * drows * Dp:]), f"{tag}: dtok written past its end"
        grid = dtok[:B * drows * Dp].reshape(B, drows, Dp)
        assert all_sentinel(grid[:, :t0]) and all_sentinel(grid[:, t0 + T:]), f"{tag}: dtok rows outside [t0, t0 + T) were written"
        out.dtok = grid[:, t0:t0 + T]
        assert none_sentinel(out.dtok) and bool(torch.isfinite(out.dtok).all()), f"{tag}: a dtok row was not overwritten, or is not finite"
    if want_pro:
        out.dpro = inner(tag, "dprotos", dpro, P * Dp).reshape(P, Dp)
    return out


def check_bwd(tag, pr, gr, res, idx, is_act, own, tiled, mx):
    dtok, a_tok, dpro, a_pro = backward_reference(pr, gr.g_full, gr.rows, gr.g_max, idx, is_act, own, tiled)
    if res.dtok is not None:
        check_abs(tag, "dtok", res.dtok, dtok, a_tok, mx)
    if res.dpro is not None:
        want = res.pre + dpro
        check_abs(tag, "dprotos", res.dpro, want, a_pro + U * (res.pre.abs() + want.abs()), mx)


def bwd_case(name, pr, gr, modes=("ref-dist", "ref-act", "own-dist", "own-act"), ws="full", want=((True, True),), mx=None, fwd_ok=True):
    """Every feeding mode of one backward problem: the maps of the reference or of the kernel forward, as distances or as activations."""
    mx = Maxima(pr.ref_u) if mx is None else mx
    ppc = gr.rows[2] if gr.rows is not None else 0
    fwd = None
    results = {}
    for mode in modes:
        own, is_act = mode.startswith("own"), mode.endswith("act")
        if is_act and pr.T == 1:
            continue
        if own and not fwd_ok:
            continue
        tag = f"proto_bwd {name} {mode}"
        if own:
            if fwd is None:
                fwd = run_fwd(tag, pr)
                check_fwd(tag, pr, fwd, Maxima())
            fmap, idx = (fwd.act if is_act else fwd.dist).contiguous(), fwd.argmax
        else:
            fmap, idx = (pr.a if is_act else pr.d).float().contiguous(), pr.idx
        for want_tok, want_pro in want:
            res = run_bwd(tag, pr, gr, fmap, is_act, idx if pr.T > 1 else None, want_tok, want_pro, ws)
            check_bwd(tag, pr, gr, res, idx, is_act, own, tiled_route(pr, gr, ppc, ws == "full") and want_pro, mx)
            results[(mode, want_tok, want_pro)] = res
    report(f"proto_bwd[{name}]", **mx)
    return results


# ------------------------------------------------------------------------------------------------ backward: dense g_full
@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("Dp", [4, 6, 64, 68, 128, 132, 192, 196, 256, 260, 320, 384, 388, 512])
def test_bwd_dense_every_nj(Dp, family):
    """NJ = 1, 2, 3, 4, 6, 8 of the token and gather kernels, each at its full width and one float4 past the previous one; Dp = 6 is fed by the
    reference only (the forward refuses it)."""
    pr = problem(family, 2, 5, 33, Dp, 1, 1)
    bwd_case(f"nj-{Dp}-{family}", pr, make_grads(pr, "dense+max", Dp), fwd_ok=Dp % 4 == 0)


def wave_edge_prototypes(P):
    """The prototypes at bits 0 and 31 of the first and the last bitmap word of every wave's range (NW = 8), and P - 1."""
    W = (P + 31) // 32
    nw = 8 if W > 64 else 1
    wpw = (W + nw - 1) // nw
    out = {P - 1}
    for wave in range(nw):
        w0, w1 = wave * wpw, min(W, (wave + 1) * wpw)
        for w in (w0, w1 - 1):
            if w0 <= w < w1:
                out |= {p for p in (32 * w, 32 * w + 31) if p < P}
    return sorted(out)


@pytest.mark.parametrize("P", [2048, 2049, 4100, 8192])
def test_bwd_token_kernel_width(P):
    """proto_bwd_tokens_kernel<1, 1> at its widest (P = 2048: W = 64) and <1, 8> past it: per-wave word ranges, the plist offsets relative to
    w_begin, the LDS partial reduction."""
    for family in ("A", "B"):
        pr = problem(family, 2, 2, P, 4, 1, 1)
        gr = make_grads(pr, "max", P)
        gf = torch.zeros(2, P, 2)
        edge = wave_edge_prototypes(P)
        gf[0, edge, 0], gf[1, edge, 1], gf[1, edge[::2], 0] = 1.25, -0.5, 3.0
        gr.g_full = gf.to(DEV)
        bwd_case(f"width-{P}-{family}", pr, gr)
        gr.g_max = None                                              # the edge entries alone: a lost word or bit is the whole row
        bwd_case(f"width-{P}-{family}-edges-only", pr, gr)


@pytest.mark.parametrize("pattern", ["dense", "isolated", "holes"])
@pytest.mark.parametrize("T,P", [(5, 33), (4, 40), (1, 33)])
def test_bwd_mark_kernel(T, P, pattern):
    """Both alignment branches of the mark kernel ((b P + 32 w) T odd, and a multiple of 4), isolated entries, exact zeros inside dense rows;
    T = 1 through ppf_proto_bwd (no arg-max)."""
    for family in ("A", "C-randn"):
        pr = problem(family, 2, T, P, 64, 1, 1)
        for with_max in (False, True):
            bwd_case(f"mark-{T}-{P}-{pattern}-{family}-{int(with_max)}", pr, make_grads(pr, pattern + ("+max" if with_max else ""), 11 * T + P))


@pytest.mark.parametrize("B", [128, 129])
def test_bwd_gather_block_loop(B):
    """proto_bwd_protos_kernel: B T = 16384 is exactly one block of 16 x 1024 elements, 129 x 128 runs the loop a second time over 128 elements."""
    for family in ("A", "C-rand"):
        pr = problem(family, B, 128, 3, 4)
        gf = torch.zeros(B * 128, 3)
        gf[torch.randperm(B * 128, generator=torch.Generator().manual_seed(B))[:400]] = torch.tensor([0.5, -1.0, 2.0])
        for e in (0, 1023, 1024, 16383, 16384, B * 128 - 1):         # the first and the last element of a wave's range and of each block
            if e < B * 128:
                gf[e] = torch.tensor([1.0, -2.0, 0.25])
        gr = SimpleNamespace(g_full=gf.reshape(B, 128, 3).permute(0, 2, 1).contiguous().to(DEV), rows=None, g_max=None)
        bwd_case(f"blocks-{B}-{family}", pr, gr)


# ------------------------------------------------------------------------------------------------ backward: g_max only, block rows
def labels_for(B, ncls):
    """Two samples of one class, a class without a sample, the last class."""
    lab = [(3 * b) % ncls for b in range(B)]
    lab[0] = ncls - 1
    if B > 1:
        lab[1] = lab[-1] = 0
    if ncls > 2:
        lab = [(c if c != 1 else 0) for c in lab]                    # class 1 has no sample
    return torch.tensor(lab, dtype=torch.int64)


@pytest.mark.parametrize("B,P,Dp,T", [(8, 40, 64, 5), (16, 257, 16, 3), (5, 40, 64, 5), (40, 4097, 4, 2), (32, 4097, 4, 2)])
def test_bwd_tiled_grid_mapping(B, P, Dp, T):
    """proto_bwd_protos_tiled_kernel's workgroup -> (tile, sample group) map with the XCD remap (gridDim.x % 8 == 0 and nsg % 8 == 0) and without."""
    pt = (P + 255) // 256
    sg = min(B, (256 + pt - 1) // pt)
    spg = (B + sg - 1) // sg
    nsg = (B + spg - 1) // spg
    assert ((pt * nsg) % 8 == 0 and nsg % 8 == 0) == ((B, P) in ((8, 40), (16, 257), (32, 4097))) and (P != 4097 or pt == 17)
    assert (B, P) != (40, 4097) or (spg == 3 and B % spg != 0)
    for family in ("A", "C-randn"):
        pr = problem(family, B, T, P, Dp)
        bwd_case(f"grid-{B}-{P}-{family}", pr, make_grads(pr, "max", B + P))
        if P == 40:
            ppc = 10
            bwd_case(f"grid-{B}-{P}-{family}-rows", pr, make_grads(pr, "max+rows", B + P, ppc, labels_for(B, P // ppc)))


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("Dp", [4, 64, 68, 128, 132, 192, 196, 256, 260, 320, 384, 388, 512])
def test_bwd_tiled_every_nj(Dp, family):
    """NJ = 1, 2, 3, 4, 6 of the tiled and rows kernels (g_max only, and g_max + block rows); Dp = 388 and 512 are past one LDS image
    (proto_tiled_geometry: Dp > 384): the gather kernel at NJ = 8 reads g_rows."""
    pr = problem(family, 3, 5, 40, Dp, 1, 1)
    bwd_case(f"tiled-nj-{Dp}-{family}", pr, make_grads(pr, "max", Dp))
    bwd_case(f"tiled-nj-{Dp}-{family}-rows", pr, make_grads(pr, "max+rows", Dp, 10, labels_for(3, 4)))


@pytest.mark.parametrize("T,Dp", [(50, 384), (51, 384), (101, 384), (128, 384), (2, 4)])
def test_bwd_tiled_lds_chunks(T, Dp):
    """One, two and three LDS images per sample (50 rows of 1536 bytes fill the 76 KiB image), the rows kernel's coefficient window at a chunk
    start that is no multiple of 64, and the 32-byte image whose copy clamps to its last 16 bytes."""
    for family in ("A", "C-randn"):
        pr = problem(family, 3, T, 40, Dp, 1, 1)
        bwd_case(f"chunks-{T}-{Dp}-{family}", pr, make_grads(pr, "max+rows", T + Dp, 10, labels_for(3, 4)))


@pytest.mark.parametrize("with_max", [True, False])
@pytest.mark.parametrize("ppc", [1, 10, 16, 17])
def test_bwd_rows_classes(ppc, with_max):
    """ppc <= 16: the tiled / rows / finish kernels; ppc = 17: the gather kernel reads g_rows.  Labels: two samples of one class, a class
    without a sample, the last class (label ppc == P - ppc)."""
    ncls = 5
    for family in ("A", "C-rand"):
        pr = problem(family, 6, 9, ncls * ppc, 48, 1, 1)
        gr = make_grads(pr, ("max+" if with_max else "") + "rows" + ("+sparse-rows" if family == "A" else ""), ppc, ppc, labels_for(6, ncls))
        assert int(gr.rows[1].max()) * ppc == pr.P - ppc and 1 not in gr.rows[1].tolist() and gr.rows[1].tolist().count(0) >= 2
        bwd_case(f"classes-{ppc}-{int(with_max)}-{family}", pr, gr)


@pytest.mark.parametrize("form", ["max", "max+rows", "dense+max"])
def test_bwd_outputs_separately(form):
    """dtok only, dprotos only and both: the separate calls are bit-identical to the combined one."""
    pr = problem("C-randn", 4, 9, 40, 64, 1, 1)
    gr = make_grads(pr, form, 3, 10, labels_for(4, 4))
    res = bwd_case(f"separately-{form}", pr, gr, want=((True, True), (True, False), (False, True)))
    for mode in ("ref-dist", "ref-act", "own-dist", "own-act"):
        both, tok, pro = (res[(mode, *w)] for w in ((True, True), (True, False), (False, True)))
        assert tok.dpro is None and pro.dtok is None
        assert same_bits(tok.dtok, both.dtok) and same_bits(pro.dpro, both.dpro), f"{form} {mode}: the separate calls differ from the combined one"


@pytest.mark.parametrize("form", ["max", "max+rows"])
def test_bwd_bitmap_only_workspace(form):
    """A workspace that holds the bitmap only: the gather kernel computes the prototype gradients -- within the gates of the tiled result."""
    for family in ("A", "C-randn"):
        pr = problem(family, 4, 9, 40, 64, 1, 1)
        gr = make_grads(pr, form, 4, 10, labels_for(4, 4))
        mx = Maxima(pr.ref_u)
        tiled = bwd_case(f"bitmap-{form}-{family}-tiled", pr, gr, modes=("ref-dist",), mx=mx)[("ref-dist", True, True)]
        gather = bwd_case(f"bitmap-{form}-{family}-gather", pr, gr, modes=("ref-dist",), ws="bitmap", mx=mx)[("ref-dist", True, True)]
        assert same_bits(gather.dtok, tiled.dtok)
        _, _, _, a_t = backward_reference(pr, gr.g_full, gr.rows, gr.g_max, pr.idx, False, False, True)
        _, _, dpro, a_g = backward_reference(pr, gr.g_full, gr.rows, gr.g_max, pr.idx, False, False, False)
        assert bool((a_g <= a_t).all())
        check_abs("gather against tiled", "dprotos_vs_tiled", gather.dpro, tiled.dpro.double(), 2 * (a_t + U * (tiled.pre.abs() + (tiled.pre + dpro).abs())), mx)
        report(f"proto_bwd[bitmap-{form}-{family}]", **mx)


def test_bwd_refusals():
    """The same for the three backward entry points.  (The workspace refusal of ppf_proto_bwd_rows used to name ppf_proto_bwd: the launcher
    the two share now takes the caller's name.)"""
    B, T, P, Dp = 2, 5, 40, 16
    tok, pro = torch.zeros(B, T, 520, device=DEV), torch.zeros(8200, 4, device=DEV)
    fmap, g = torch.ones(B * 8200 * T, device=DEV), torch.ones(B * 8200 * T, device=DEV)
    idx, label = torch.zeros(B * 8200, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int64, device=DEV)
    dtok, dpro = sentinel(B * T * 520), sentinel(8200 * 4)
    ws = scratch(1 << 20)

    def bwd(T=T, P=P, Dp=Dp, fmap=fmap, g_full=g, g_max=g, idx=idx, dtok=dtok, ws=ws, nbytes=1 << 20, tok=tok, pro=pro):
        return ("ppf_proto_bwd", tok, T * Dp, 0, T, pro, B, P, Dp, 0, 1e-4, fmap, 0, g_full, g_max, idx, dtok, T * Dp, dpro, ws, nbytes)

    def rows(T=T, P=P, Dp=Dp, g_rows=g, label=label, ppc=4, g_max=g, idx=idx, dtok=dtok, ws=ws, nbytes=1 << 20):
        return ("ppf_proto_bwd_rows", tok, T * Dp, 0, T, pro, B, P, Dp, 0, 1e-4, fmap, 0, g_rows, label, ppc, g_max, idx, dtok, T * Dp, dpro, ws, nbytes)

    def single(nbytes=1 << 20, ws=ws, g=g):
        return ("ppf_proto_bwd_single", tok, T * Dp, 0, pro, B, P, Dp, 0, 1e-4, fmap, g, dtok, T * Dp, dpro, ws, nbytes)

    W = (P + 31) // 32
    cases = [(ERR_SHAPE, [bwd(Dp=516), bwd(P=8193), bwd(T=0), bwd(P=0), rows(Dp=516), rows(P=8193), rows(ppc=0), rows(ppc=P + 1), rows(T=1)]),
             (ERR_ARG, [bwd(ws=None, nbytes=0), bwd(nbytes=B * T * W * 4 - 1), rows(ws=None, nbytes=0), rows(nbytes=B * T * W * 4 - 1), rows(g_rows=None),
                        rows(label=None), bwd(idx=None), rows(idx=None), bwd(fmap=None), bwd(g_full=None, g_max=None), bwd(tok=None), bwd(pro=None),
                        single(nbytes=lib().ppf_proto_bwd_single_workspace(B, P, Dp) - 1), single(ws=None), single(g=None)])]
    for rc, calls in cases:
        for args in calls:
            with pytest.raises(RuntimeError, match=rf"rc={rc}\): {args[0]}\b"):
                call(*args)
    torch.cuda.synchronize()
    assert all_sentinel(dtok) and all_sentinel(dpro), "a refused call wrote an output"
    dpro[:P * Dp] = 0.0
    for args in (bwd(), rows(), single(), bwd(idx=None, g_max=None), rows(idx=None, g_max=None), bwd(nbytes=B * T * W * 4)):
        call(*args)                                                  # the argument builders are sound, and the documented minima are accepted
    torch.cuda.synchronize()
    assert none_sentinel(dtok[:B * T * Dp])


# ------------------------------------------------------------------------------------------------ T == 1: the dense form
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("B", [1, 63, 65])
def test_bwd_single(B, P):
    """ppf_proto_bwd_single: G, its row and column sums, two fp32 products and the fix-up, at every Dp and both activation kinds."""
    for Dp, kind, family in ((4, 0, "A"), (48, 1, "A"), (100, 0, "C-rand"), (48, 0, "B"), (100, 1, "C-randn"), (4, 1, "C-randn8")):
        pr = problem(family, B, 1, P, Dp, 1, 1, kind)
        name = f"single-{B}-{P}-{Dp}-{kind}-{family}"
        mx = Maxima(pr.ref_u)
        g = torch.randn(B, P, generator=torch.Generator().manual_seed(B + P)).to(DEV)
        fwd = run_fwd(name, pr)
        check_fwd(name, pr, fwd, Maxima())
        need = lib().ppf_proto_bwd_single_workspace(B, P, Dp)
        drows = pr.rows + 1
        pre = dyadic((P, Dp), 9 + P)
        for own in (False, True):
            dist = (fwd.dist if own else pr.d.float()).reshape(B, P).contiguous()
            dtok_ref, a_tok, dpro_ref, a_pro = backward_reference(pr, None, None, g, pr.idx, False, own, True, True)
            want = pre.double() + dpro_ref
            a_pro = a_pro + U * (pre.double().abs() + want.abs())
            outs = {}
            for want_tok, want_pro in ((True, True), (True, False), (False, True)):
                runs = []
                for _ in range(2):
                    dtok = sentinel(B * drows * Dp) if want_tok else None
                    dpro = sentinel(P * Dp) if want_pro else None
                    if want_pro:
                        dpro[:P * Dp] = pre.reshape(-1)
                    call("ppf_proto_bwd_single", pr.tok, pr.stride_b, pr.t0, pr.pro, B, P, Dp, kind, pr.eps, dist, g, dtok, drows * Dp, dpro, scratch(need), need)
                    runs.append((dtok, dpro))
                torch.cuda.synchronize()
                for u, v in zip(*runs):
                    assert u is None or same_bits(u, v), f"{name}: two runs differ"
                dtok, dpro = runs[0]
                tag = f"{name} own={own} dtok={want_tok} dprotos={want_pro}"
                if want_tok:
                    assert all_sentinel(dtok[B * drows * Dp:])
                    grid = dtok[:B * drows * Dp].reshape(B, drows, Dp)
                    assert all_sentinel(grid[:, :pr.t0]) and all_sentinel(grid[:, pr.t0 + 1:]), f"{tag}: dtok rows outside the token row were written"
                    check_abs(tag, "dtok", grid[:, pr.t0:pr.t0 + 1], dtok_ref, a_tok, mx)
                    outs[("tok", want_pro)] = grid[:, pr.t0]
                if want_pro:
                    check_abs(tag, "dprotos", inner(tag, "dprotos", dpro, P * Dp).reshape(P, Dp), want, a_pro, mx)
                    outs[("pro", want_tok)] = dpro
            assert same_bits(outs[("tok", True)], outs[("tok", False)]) and same_bits(outs[("pro", True)], outs[("pro", False)])
        report(f"proto_bwd_single[{B}-{P}-{Dp}-{kind}-{family}]", **mx)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("family", ["A", "B", "C-rand", "C-randn", "C-randn8", "D"])
def test_reference_against_the_oracle(family):
    """The closed forms of this file against oracle.ppf_oracle.proto_activations and its autograd, in fp64 (eps = 1e-4, the oracle's constant;
    the reference's eps is the fp64 value of fp32(1e-4): the activations may differ by |eps64 - 1e-4| / (d + eps))."""
    from oracle import ppf_oracle as O
    T = 40
    pr = problem(family, 4, T, 33, 48, 1, 0)
    x = pr.x.cpu().clone().requires_grad_(True)
    p = pr.p.cpu().clone().requires_grad_(True)
    amax, d, a = O.proto_activations(x, p)
    assert d.dtype == torch.float64
    dref, aref = pr.d.cpu(), pr.a.cpu()
    scale = ((pr.x ** 2).sum(-1)[:, None, :] + (pr.p ** 2).sum(-1)[None, :, None]).cpu()
    assert bool(((d - dref).abs() <= 1e-13 * scale).all())
    slack = (1e-13 * scale + abs(pr.eps64 - O.PROTO_EPS)) / (dref + pr.eps64) + 1e-13
    assert bool(((a - aref).abs() <= slack).all())
    idx = pr.idx.cpu()
    assert bool(((amax - a.gather(-1, idx[..., None])[..., 0]).abs() <= 2 * slack.gather(-1, idx[..., None])[..., 0]).all())
    if family == "D":
        return                                                       # exact ties: autograd's choice among them is not the rule under test
    gr = make_grads(pr, "dense+max", 17)
    loss = (a * gr.g_full.cpu().double()).sum() + (a.gather(-1, idx[..., None])[..., 0] * gr.g_max.cpu().double()).sum()
    loss.backward()
    dtok, _, dpro, _ = backward_reference(pr, gr.g_full, None, gr.g_max, pr.idx, False, False, False)
    # d (da/dd) / d eps = 1 / (d + eps)**2: the oracle's eps against fp32(eps), and 1e-12 of the coefficients for the arithmetic
    g_abs = (gr.g_full.double() + torch.zeros_like(pr.d).scatter_(-1, pr.idx[..., None], gr.g_max.double()[..., None])).abs()
    slack_g = float((g_abs * (1e-12 / (pr.d + pr.eps64) + abs(pr.eps64 - O.PROTO_EPS) / (pr.d + pr.eps64) ** 2)).sum())
    tol = 2 * slack_g * float((pr.x.abs().max() + pr.p.abs().max()).detach())
    assert float((x.grad - dtok.cpu()).abs().max()) <= tol and float((p.grad - dpro.cpu()).abs().max()) <= tol
