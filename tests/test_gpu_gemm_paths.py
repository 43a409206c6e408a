"""Every kernel and epilogue branch of ppf_gemm_bf16 (csrc/gemm_bf16.hip, gemm_common.h) against an fp64 reference at the smallest shapes
that reach it, called through the C ABI with explicit lda / ldb / ldc / ldres / ldaux (ops.gemm cannot express a pitch).  Every call
asserts the kernel that served it (ppf_gemm_test_last_kernel), so a cost-model change fails these tests instead of hollowing them out.

Routes (code), how they are reached, epilogues and edges:
  1  gemm_kernel NT        default; BF16 F32 GELU SIGMOID RESID DGELU; (1,8,8) all MFMA blocks but one masked, (33,132,72) N % 8 == 4 and a K
                           tail of 8, (130,260,200) two ragged tiles each way, (257,128,64) one K tile
  6  gemm128g              default cost model (>= 512 tiles, K <= 512, N >= 512); BF16 GELU RESID DGELU; M = 16261 leaves a 5-row last tile
                           (the min(row, M - 1) clamp), N = 520 / 516 a ragged last column tile (516: the 4-column remainder)
  7  gemm224g              ppf_gemm_test_force_g224(1); BF16 without bias; (1,8,64) (225,136,128) (449,392,192)
  2  gemm_kernel NN        default; BF16 F32 DGELU; (33,136,72) (130,264,200)
  3  gemm_kernel TT F32    default; (136,72,264) (264,136,200)
  4  gemm_kernel TT ATOMIC no workspace: (192,192,520) with ldb = 5 * 192, three slices of real atomics; (136,72,200) one slice, also with a
                           workspace (ns == 1 keeps the atomic kernel); + colsum
  5  TT PARTIAL + reduce   workspace, a narrow side: (192,192,520) slices 192 / 192 / 136, (136,200,264); with and without colsum
  8 / 9    wgrad8<4,2> register-staged / DMA   (512,320,512), (1032,328,520) and (512,320,264): K % 64 != 0, register-staged only; + colsum
  10 / 11  wgrad8<2,4> register-staged / DMA   (320,512,512), (328,1032,520) and (320,512,264): register-staged only; + colsum
Every NT / NN route runs each (shape, epilogue) in these forms: bias present and absent, alpha in {1, -0.375}, ldc = ldaux = N + 8 with
ldres = N + 4, ldc = ldaux = ldres = N + 4, lda = 3 K with ldb = 2 K (the CaiT cls-row form).  Of the pitches, N + 4 makes the row pitch
8-aligned when N % 8 == 4 (the wide branch of epilogue_rows with its 4-column remainder) and unaligned when N % 8 == 0 (the narrow fallback
of the wide epilogues); N + 8 does the opposite.  One form has ldc = N + 8 with ldaux = N + 16 (a kernel that takes one pitch for the
other).  RESID additionally: rowscale with rows_per_group 7 and 197, no rowscale, no colscale,
no aux_out.  So every instantiated (mode, epilogue) pair is hit: NT x {0..5}, gemm128g x {0,2,4,5}, gemm224g x {0}, NN x {0,1,5},
TT x {F32, ATOMIC, PARTIAL}, wgrad8 x {<4,2>, <2,4>} x {registers, DMA}.

Sentinels: every output, aux_out and colsum has 16 extra rows and, under a pitch, ld - N extra columns prefilled with a sentinel bit pattern;
everything outside [0, M) x [0, N) must keep it bit for bit.  The split-K workspace carries a guard behind the bytes the library asks for.

Reference: fp64 torch on the device from the exactly representable bf16 operands: P = A B^T, S = |A| |B|^T, every epilogue written out in
fp64 (torch.special.erf, torch.sigmoid, helpers.gelu8_decode on the given codes).

Gates, in u = 2**-24, all scales from the fp64 reference (mass = |alpha| S + |bias|):
  accumulation  a bf16 x bf16 product is exact in fp32, only the additions round: any-order bound a_acc = (K + 8) u |alpha| S (the column-sum
                convention of test_gpu_explain.py / test_gpu_layernorm_paths.py).  The kernel guides document MFMA accumulation as a chain of
                correctly rounded fused multiply-adds (cdna_hip_programming.md, "Numerics"); nothing there says truncation, so u is not widened.
  pre-activation v = alpha acc + bias: a_v = a_acc + c u mass, c = 1 (alpha) + 1 (bias, when present)
  F32           |out - v| <= a_v
  BF16          bf16_rne(v - a_v) <= out <= bf16_rne(v + a_v)  (the exact interval of the LayerNorm file; no rtol)
  RESID         out = res + v w, w = colscale rowscale: |err| <= a_acc |w| + 5 u (|res| + mass |w|) (alpha, bias, colscale, rowscale, add);
                raw branch: the bf16 interval of v with a_v
  DGELU         out = v h, h = the decoded code (the same fp32 expression as the kernel, exact): bf16 interval with (a_acc + 3 u mass) |h|
  GELU          bf16 interval of gelu(v) with a_g = 1.13 a_v + |v| (E / 2 + 4 u): |gelu'| <= 1.13, and cdf = 1/2 + erf / 2 carries half the error
                E of the kernel's erf.  E = 1.5e-7 + 80 u: Abramowitz-Stegun 7.1.26 "|abs err| <= 1.5e-7" (ppf_common.h, fast_erf); t = rcp(den) is
                "v_rcp_f32 (1 ulp)" (same comment) = 2 u relative, + 2 u for den and z, and |t poly'(t)| <= sum k |a_k| = 16.2 on t <= 1: 65 u;
                exp2 is v_exp_f32, 1 ulp in AMD's public CDNA ISA guide (the project's files give no figure): with its argument's three
                roundings |d e| <= 2 u e + 3 u ln2 |a2| 2^-|a2| <= 3.2 u; five FMAs of the Horner chain on values <= 1.5: the rest of the 80.
  gelu' code    a_d = 0.8 a_v + E / 2 + 4 u (1 + |v|) + 2 u (|gelu''| <= 0.8; the last 2 u: the fp32 FMA 196 d + 26 <= 250 u / 196); the code
                must lie in [rint(196 (d - a_d) + 26), rint(196 (d + a_d) + 26)] clamped to [0, 255] (no atol)
  SIGMOID       a_v / 4 + e_sig; there is no documented figure for __expf, so e_sig = 4 x the largest error of a plain fp32 torch evaluation
                of the same epilogue against fp64 on the same inputs (reference against reference; reported as sig_ref_u)
  split-K       C += alpha acc: (K + 8 + ns + 1) u (|alpha| S + |C0|) + u |alpha| S: ns slab additions (or atomics) and the non-zero initial
                C, whose magnitude joins the sum; column sums (not scaled by alpha): (K + 8 + ns + 1) u (sum|A| + |colsum0|)
  repeats       three runs bit-identical on every path but real atomics (ATOMIC with ns > 1); wgrad8 register-staged == DMA bit for bit
  one transpose-detecting integer pattern per kernel, torch.equal against the exact product.

Measured maxima on an MI355X (helpers.report: *_frac = the worst error as a fraction of its gate -- for bf16 outputs the part beyond half a
bf16 ulp as a fraction of the fp32 allowance --, *_u = the same error in u of the gate's own scale).  The any-order bound is a worst case; a
k-ordered fp32 chain on random signs stays near sqrt(K) u, hence the small fractions at large K:
  generic NT   F32 0.125 (1.61 u)   BF16 0.0022   RESID 0.160 (1.79 u), raw 0.0022   DGELU 0.0046   GELU 0.0077, every code within 1 of
               rint(196 d + 26) and the interval is a single code at 95.2 % of the elements   SIGMOID 0.228 (2.59 u; e_sig / 4 = 1.62 u)
  gemm128g     BF16 0.0096   RESID 0.135 (2.74 u), raw 0.0096   DGELU 0.0133   GELU 0.0112, single-code interval at 72 % (K = 512: a_acc alone
               is 0.2 of a code step)
  generic NN   F32 0.0146 (1.58 u)   BF16 0.0007   DGELU 0.0027         gemm224g  BF16 0.0016          TT F32  0.0066 (1.38 u)
  TT ATOMIC    C 0.0048 (1.00 u), colsum 0.0009 (0.19 u)     TT PARTIAL  C 0.0053 (1.46 u), colsum 0.0005 (0.14 u)
  wgrad8       C 0.0053 (1.46 u), colsum 0.0010 (0.28 u); register-staged and DMA bit-identical at every shape
The whole file runs in 4 s (68 tests; the slowest, the first, 0.9 s with the library load).

The gates bite: seven value-only edits of the kernels (a scratch build, nothing committed), each run against this file and against
test_gpu_gemm.py as it stands -- every edit fails tests here and none fails there:
  1. epi_store8 without alpha                                   -> generic NT / gemm128g / NN x {BF16, GELU, DGELU}: 25 tests
  2. gemm224g's store without alpha                             -> test_gemm224g, all three shapes
  3. the 4-column remainder of the wide branch reads the strip at col + 4
                                                                -> NT (33,132,72) and (130,260,200), gemm128g (16261,516,192) x {BF16, GELU,
                                                                   DGELU}, test_transpose_detecting[gemm128g]: 10 tests
  4. epi_store8's DGELU drops the bias of its first column      -> every DGELU case of NT / gemm128g / NN: 9 tests
  5. DirectLds clamps A rows to M - 2 in gemm128g               -> all 12 gemm128g cases (M = 16384 too: its last row is row M - 1)
  6. the partial / atomic column sums multiplied by alpha       -> test_tt_atomic, test_tt_partial_reduce, test_wgrad8: all 11 cases
  7. epi_store8's GELU writes its codes at pitch ldc, not ldaux -> NT (257,128,64) GELU, gemm128g (16261,520,64) and (16384,512,512) GELU
Four more edits were run the same way and fail in BOTH files, so they do not count above: "bias + n0" for the second float4 of
epi_load_cols8 (25 tests here, 8 there), "n + 8 < p.N" in the wide branch (16 / 13), rowscale indexed by m % 128 (5 / 1) and gload's kend
short by 8 (31 / 15): test_gpu_gemm.py has a bias on wide bf16 outputs, uninitialised outputs, two DropPath groups over 394 rows, K = 72."""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from helpers import SENT, U, bf16_rne, bits, gelu8_decode, half_ulp_bf16, report

pytestmark = pytest.mark.gpu

BF16, F32, GELU, SIGMOID, RESID, DGELU, ATOMIC = range(7)
EPI_NAME = {BF16: "BF16", F32: "F32", GELU: "GELU", SIGMOID: "SIGMOID", RESID: "RESID", DGELU: "DGELU", ATOMIC: "ATOMIC"}
ERR_ALIGN, ERR_ARG, ERR_SHAPE = -2, -3, -1
PAD = 16                                 # sentinel rows behind every output
SENT8 = 0xA5                             # sentinel byte of the 8-bit gelu' codes and the workspace guard
E_ERF = 1.5e-7 + 80 * U                  # the kernel's erf against the true one (module docstring)
(R_NT, R_NN, R_TT_F32, R_TT_ATOMIC, R_TT_PARTIAL, R_G128, R_G224, R_WG42, R_WG42_DMA, R_WG24, R_WG24_DMA) = range(1, 12)


def _rand(shape, scale, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g) * scale


def last_kernel():
    from protopformer_amd import _lib
    return _lib.lib().ppf_gemm_test_last_kernel()


def gemm_raw(A, B, C, M, N, K, lda, ldb, ldc, ta, tb, epi, *, bias=None, res=None, ldres=0, rowscale=None, rpg=1, colscale=None, aux_in=None,
             aux_out=None, ldaux=0, colsum=None, alpha=1.0, ws=None, ws_bytes=None):
    """ppf_gemm_bf16 as the C ABI has it; returns the code of the kernel that was launched."""
    from protopformer_amd import _lib
    _lib.call("ppf_gemm_bf16", A, B, C, M, N, K, lda, ldb, ldc, int(ta), int(tb), epi, bias, res, ldres, rowscale, rpg, colscale, aux_in, aux_out,
              ldaux, colsum, float(alpha), ws, (ws.numel() if ws_bytes is None else ws_bytes) if ws is not None else 0)
    return last_kernel()


def sentinel_buf(M, N, ld, dtype, inner=None):
    """(M + PAD) x ld, all sentinel; `inner` (M x N) goes to the top-left block (accumulating outputs)."""
    t = torch.full((M + PAD, ld), SENT8 if dtype == torch.uint8 else SENT, dtype=dtype, device="cuda")
    if inner is not None:
        t[:M, :N] = inner
    return t


def same_bits(a, b):
    """Bit-for-bit equality of two device tensors (NaNs and signed zeros included), without a trip to the host."""
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def assert_pad_untouched(tag, name, buf, M, N):
    want = SENT8 if buf.dtype == torch.uint8 else SENT
    for what, part in (("rows past M", buf[M:]), ("columns past N", buf[:M, N:])):
        assert torch.equal(bits(part), bits(torch.full(part.shape, want, dtype=buf.dtype))), f"{tag}: {name} written in the {what}"


@functools.lru_cache(maxsize=4)
def problem(ta, tb, M, N, K, lda, ldb, integer=False):
    """Operands as stored (contraction-contiguous [R][ld] or contraction-strided [K][ld]) and the fp64 P = A B^T, S = |A| |B|^T."""
    sa, sb = ((K, lda) if ta else (M, lda)), ((K, ldb) if tb else (N, ldb))
    if integer:                          # asymmetric: an (m, n)-swapped write or a k-permutation mismatch between A and B cannot pass
        al, bl = torch.zeros(M, K), torch.zeros(N, K)
        m, n = torch.arange(M), torch.arange(N)
        al[m, m % K] = 1.0 + (m % 7)
        bl[n, (3 * n + 1) % K] = 2.0 + (n % 5)
        a_store, b_store = torch.full(sa, 3.0), torch.full(sb, -5.0)        # what lies between the rows must not be read
        if ta: a_store[:, :M] = al.T
        else: a_store[:, :K] = al
        if tb: b_store[:, :N] = bl.T
        else: b_store[:, :K] = bl
        a_store, b_store = a_store.cuda().bfloat16(), b_store.cuda().bfloat16()
    else:
        a_store = _rand(sa, 1.0, 1000 + M + 3 * K).bfloat16()
        b_store = _rand(sb, 0.1, 2000 + N + 5 * K).bfloat16()
    A = (a_store[:, :M].T if ta else a_store[:, :K]).double()
    B = (b_store[:, :N].T if tb else b_store[:, :K]).double()
    return SimpleNamespace(a=a_store, b=b_store, A=A, P=A @ B.T, S=A.abs() @ B.abs().T, M=M, N=N, K=K, lda=lda, ldb=ldb, ta=ta, tb=tb)


def frac(err, bound):
    """max err / bound where the bound is positive; where it is zero the error must be zero too."""
    z = bound <= 0
    assert not bool((err[z] != 0).any()), "non-zero error where the bound is exactly zero"
    return float((err[~z] / bound[~z]).max()) if bool((~z).any()) else 0.0


class Maxima(dict):
    def up(self, **kv):
        for k, v in kv.items():
            self[k] = max(self.get(k, 0.0), float(v))


def check_f32(tag, name, got, ref, bound, scale, mx):
    err = (got.double() - ref).abs()
    mx.up(**{name + "_frac": frac(err.nan_to_num(nan=math.inf), bound), name + "_u": frac(err.nan_to_num(nan=math.inf), U * scale)})
    bad = ~(err <= bound)
    assert not bool(bad.any()), f"{tag}: {name} over its bound at {int(bad.sum())} places (worst {mx[name + '_frac']:.3g} of the bound)"


def check_bf16(tag, name, got, ref, a, mx):
    got = got.double()
    ok = (got >= bf16_rne(ref - a)) & (got <= bf16_rne(ref + a))
    beyond = ((got - ref).abs() - half_ulp_bf16(ref)).clamp_min(0).nan_to_num(nan=math.inf)
    mx.up(**{name + "_frac": frac(beyond, a)})         # the fp32 part of the error (beyond half a bf16 ulp) as a fraction of the allowance
    assert bool(ok.all()), f"{tag}: {name} outside [bf16(v - a), bf16(v + a)] at {int((~ok).sum())} places (worst {mx[name + '_frac']:.3g} of a beyond half an ulp)"


# ------------------------------------------------------------------------------------------------ NT / NN: the fused epilogues
# (pitch added to N for ldc and ldaux, lda = 3 K and ldb = 2 K, bias, alpha[, another pitch for ldaux: a kernel that takes one pitch for the other])
FORMS = [(0, False, True, 1.0), (0, False, True, -0.375), (0, False, False, 1.0), (8, False, True, -0.375), (4, False, True, 1.0),
         (4, False, False, -0.375), (0, True, True, 1.0), (8, True, False, -0.375), (8, False, True, 1.0, 16)]
# RESID only: (rows_per_group or None, colscale, aux_out); the first runs with every form, the others with the first two pitched forms
RESID_FORMS = [(7, True, True), (197, True, True), (None, True, True), (7, False, True), (7, True, False)]


def run_fused(tag, route, tb, epi, M, N, K, form, resid=RESID_FORMS[0], mx=None, integer=False):
    """One call form of an NT (tb = False) or NN product, three times; every output gated against fp64."""
    pitch, ld, has_bias, alpha = form[:4]
    auxpitch = form[4] if len(form) > 4 else pitch
    lda = 3 * K if ld else K
    ldb = (2 * K if ld else N) if tb else (2 * K if ld else K)
    pr = problem(False, tb, M, N, K, lda, ldb, integer)
    mx = Maxima() if mx is None else mx
    ldc = N + pitch
    ldaux = N + auxpitch if epi in (GELU, RESID, DGELU) else 0
    ldres = N + (4 if pitch else 0) if epi == RESID else 0
    seed = 31 * M + 7 * N + K
    bias = _rand((N,), 0.5, seed + 1) if has_bias else None
    kw = dict(bias=bias, alpha=alpha, ldaux=ldaux, ldres=ldres)
    cdt = torch.float32 if epi in (F32, SIGMOID, RESID) else torch.bfloat16
    rpg, has_cs, has_aux = resid
    if epi == RESID:
        res_store = _rand((M, ldres), 1.0, seed + 2)
        kw["res"] = res_store
        if rpg is not None:
            groups = (M + rpg - 1) // rpg
            rs = 0.25 + torch.rand(groups, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 3))
            rs[1::3] = 0.0                              # a dropped sample: out = res exactly
            kw["rowscale"], kw["rpg"] = rs, rpg
        if has_cs:
            kw["colscale"] = 1.0 + _rand((N,), 0.3, seed + 4)
    if epi == DGELU:
        codes = torch.randint(0, 256, (M, ldaux), device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed + 5), dtype=torch.uint8)
        codes[0, :8] = torch.tensor([0, 26, 222, 255, 255, 222, 26, 0], dtype=torch.uint8)
        kw["aux_in"] = codes

    runs = []
    for _ in range(3):
        C = sentinel_buf(M, N, ldc, cdt)
        aux = None
        if epi == GELU:
            aux = sentinel_buf(M, N, ldaux, torch.uint8)
        elif epi == RESID and has_aux:
            aux = sentinel_buf(M, N, ldaux, torch.bfloat16)
        code = gemm_raw(pr.a, pr.b, C, M, N, K, lda, ldb, ldc, False, tb, epi, aux_out=aux, **kw)
        assert code == route, f"{tag}: served by kernel {code}, this test is about kernel {route}"
        runs.append((C, aux))
    torch.cuda.synchronize()
    C, aux = runs[0]
    for C2, aux2 in runs[1:]:
        assert same_bits(C, C2) and (aux is None or same_bits(aux, aux2)), f"{tag}: two runs differ"
    assert_pad_untouched(tag, "C", C, M, N)
    if aux is not None:
        assert_pad_untouched(tag, "aux_out", aux, M, N)
    out = C[:M, :N]

    b64 = bias.double() if has_bias else torch.zeros(N, dtype=torch.float64, device="cuda")
    v = alpha * pr.P + b64
    if integer:
        assert epi in (BF16, F32) and torch.equal(out.double(), v), f"{tag}: integer pattern is not the exact product"
        return mx
    a_acc = (K + 8) * U * abs(alpha) * pr.S
    mass = abs(alpha) * pr.S + b64.abs()
    a_v = a_acc + (1 + has_bias) * U * mass
    n = EPI_NAME[epi].lower()
    if epi == BF16:
        check_bf16(tag, n, out, v, a_v, mx)                      # (measured maxima of every gate: module docstring)
    elif epi == F32:
        check_f32(tag, n, out, v, a_v, mass, mx)
    elif epi == GELU:
        cdf = 0.5 * (1 + torch.special.erf(v / math.sqrt(2)))
        d = cdf + v * torch.exp(-0.5 * v * v) / math.sqrt(2 * math.pi)
        check_bf16(tag, n, out, v * cdf, 1.13 * a_v + v.abs() * (0.5 * E_ERF + 4 * U), mx)
        a_d = 0.8 * a_v + 0.5 * E_ERF + 4 * U * (1 + v.abs()) + 2 * U
        q = aux[:M, :N].double()
        lo, hi = torch.round(196 * (d - a_d) + 26).clamp(0, 255), torch.round(196 * (d + a_d) + 26).clamp(0, 255)
        bad = (q < lo) | (q > hi)
        mx.up(code_ambiguous=float((lo != hi).double().mean()), code_off=float((q - torch.round(196 * d + 26).clamp(0, 255)).abs().max()))
        assert not bool(bad.any()), f"{tag}: gelu' code outside [rint(196 (d - a) + 26), rint(196 (d + a) + 26)] at {int(bad.sum())} places"
    elif epi == SIGMOID:
        s = torch.sigmoid(v)
        v32 = pr.P.float() * alpha + (bias if has_bias else 0.0)
        e_sig = 4 * float((torch.sigmoid(v32).double() - s).abs().max())
        mx.up(sig_ref_u=e_sig / 4 / U)
        check_f32(tag, n, out, s, a_v / 4 + e_sig, torch.ones_like(s), mx)
    elif epi == RESID:
        w = torch.ones(M, N, dtype=torch.float64, device="cuda")
        if rpg is not None:
            w = w * kw["rowscale"].double()[torch.arange(M, device="cuda") // rpg][:, None]
        if has_cs:
            w = w * kw["colscale"].double()
        r64 = res_store[:, :N].double()
        scale = r64.abs() + mass * w.abs()
        check_f32(tag, n, out, r64 + v * w, a_acc * w.abs() + 5 * U * scale, scale, mx)
        if has_aux:
            check_bf16(tag, "raw", aux[:M, :N], v, a_v, mx)
    elif epi == DGELU:
        h = gelu8_decode(codes[:, :N]).double()
        check_bf16(tag, n, out, v * h, (a_acc + 3 * U * mass) * h.abs(), mx)
    return mx


def fused_matrix(name, route, tb, epi, M, N, K):
    mx = Maxima()
    for i, form in enumerate(FORMS):
        tag = f"{name} {EPI_NAME[epi]} {M}x{N}x{K} pitch+{form[0]} ld={form[1]} bias={form[2]} alpha={form[3]} ldaux+{form[-1] if len(form) > 4 else form[0]}"
        run_fused(tag, route, tb, epi, M, N, K, form, mx=mx)
        if epi == RESID and i in (3, 4):
            for resid in RESID_FORMS[1:]:
                run_fused(f"{tag} rpg={resid[0]} cs={resid[1]} aux={resid[2]}", route, tb, epi, M, N, K, form, resid, mx=mx)
    report(f"gemm_paths {name} {EPI_NAME[epi]} {M}x{N}x{K}", **mx)


@pytest.mark.parametrize("epi", [BF16, F32, GELU, SIGMOID, RESID, DGELU], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("M,N,K", [(1, 8, 8), (33, 132, 72), (130, 260, 200), (257, 128, 64)])
def test_generic_nt(M, N, K, epi):
    """gemm_kernel<0,0,EPI>: every epilogue, both branches of the wide ones and the 4-column remainder, pitched outputs and operands."""
    fused_matrix("nt", R_NT, False, epi, M, N, K)


@pytest.mark.parametrize("epi", [BF16, GELU, RESID, DGELU], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("M,N,K", [(16261, 520, 64), (16261, 516, 192), (16384, 512, 512)])
def test_gemm128g(M, N, K, epi):
    """gemm128g_kernel<EPI> under the default cost model: the clamped loads of a 5-row last tile, the swizzle on the source address, its four
    epilogues.  640 / 640 / 512 tiles: over g4_eligible's floor of 512."""
    fused_matrix("gemm128g", R_G128, False, epi, M, N, K)


@pytest.mark.parametrize("epi", [BF16, F32, DGELU], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("M,N,K", [(33, 136, 72), (130, 264, 200)])
def test_generic_nn(M, N, K, epi):
    """gemm_kernel<0,1,EPI>: B stored [K][ldb] (the proj / fc1 input gradients)."""
    fused_matrix("nn", R_NN, True, epi, M, N, K)


@pytest.mark.parametrize("M,N,K", [(1, 8, 64), (225, 136, 128), (449, 392, 192)])
def test_gemm224g(M, N, K):
    """gemm224g_kernel through the force hook: alpha, the n < N store mask under ldc = N + 8, the clamped rows of a 1-row last tile."""
    from protopformer_amd import _lib
    mx = Maxima()
    _lib.call("ppf_gemm_test_force_g224", 1)
    try:
        for form in [(0, False, False, 1.0), (8, False, False, -0.375), (8, True, False, -0.375), (0, True, False, 1.0)]:
            run_fused(f"gemm224g {M}x{N}x{K} pitch+{form[0]} ld={form[1]} alpha={form[3]}", R_G224, False, BF16, M, N, K, form, mx=mx)
    finally:
        _lib.call("ppf_gemm_test_force_g224", 0)
    report(f"gemm_paths gemm224g {M}x{N}x{K}", **mx)


# ------------------------------------------------------------------------------------------------ TT: F32, split-K
def splitk(M, N, K):
    """pick_splitk as the library computes it (read back from the workspace size it asks for)."""
    from protopformer_amd import _lib
    return (_lib.lib().ppf_gemm_workspace_bytes(M, N, K) - 16384) // ((M * N + M) * 4)


def predict_tt(M, N, K, ws, path):
    """The dispatcher's rule for epi 6: atomics without a workspace or with one slice; eight-wave tiles where both sides are >= 320 and the
    long one fills 256-wide tiles; DMA where K is whole tiles and the hook does not say registers."""
    if not ws or splitk(M, N, K) == 1:
        return R_TT_ATOMIC
    wide, dma = min(M, N) >= 320, int(K % 64 == 0 and path != 1)
    if wide and M >= 512 and M >= N and (M % 256 == 0 or M >= 1024):
        return R_WG42 + dma
    if wide and N >= 512 and (N % 256 == 0 or N >= 1024):
        return R_WG24 + dma
    return R_TT_PARTIAL


def run_tt(tag, route, epi, M, N, K, *, lda=None, ldb=None, pitch=0, alpha=1.0, ws=False, colsum=False, mx=None, integer=False, repeat=True):
    """One TT call form (F32, or the accumulating epi 6 into a non-zero C), three times; returns the first run's (C, colsum) buffers."""
    from protopformer_amd import _lib
    lda, ldb, ldc = lda or M, ldb or N, N + pitch
    pr = problem(True, True, M, N, K, lda, ldb, integer)
    mx = Maxima() if mx is None else mx
    seed = 17 * M + 3 * N + K
    ns = splitk(M, N, K) if epi == ATOMIC else 1
    C0 = torch.zeros(M, N, device="cuda") if integer or epi == F32 else _rand((M, N), 1.0, seed + 1)
    cs0 = _rand((M,), 1.0, seed + 2)
    need = _lib.lib().ppf_gemm_workspace_bytes(M, N, K)
    runs = []
    for _ in range(3 if repeat else 1):
        C = sentinel_buf(M, N, ldc, torch.float32, inner=C0 if epi == ATOMIC else None)
        cs = None
        if colsum:
            cs = torch.full((M + PAD,), SENT, device="cuda")
            cs[:M] = cs0
        wsb = None
        if ws:
            wsb = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device="cuda")       # NaN: a slab the reduce reads must have been written
            wsb[need:] = SENT8
        code = gemm_raw(pr.a, pr.b, C, M, N, K, lda, ldb, ldc, True, True, epi, colsum=cs, alpha=alpha, ws=wsb, ws_bytes=need)
        assert code == route, f"{tag}: served by kernel {code}, this test is about kernel {route}"
        runs.append((C, cs))
        if ws:
            torch.cuda.synchronize()
            assert bool((wsb[need:] == SENT8).all()), f"{tag}: written behind the workspace the library asked for"
    torch.cuda.synchronize()
    C, cs = runs[0]
    if not (route == R_TT_ATOMIC and ns > 1):                            # real atomics from several slices are not ordered
        for C2, cs2 in runs[1:]:
            assert same_bits(C, C2) and (cs is None or same_bits(cs, cs2)), f"{tag}: two runs differ"
    assert_pad_untouched(tag, "C", C, M, N)
    if cs is not None:
        assert torch.equal(bits(cs[M:]), bits(torch.full((PAD,), SENT))), f"{tag}: colsum written past M"
    out = C[:M, :N]
    ref = C0.double() + alpha * pr.P
    if integer:
        assert torch.equal(out.double(), ref), f"{tag}: integer pattern is not the exact product"
        return runs[0]
    if epi == F32:
        check_f32(tag, "f32", out, ref, (K + 8 + 1) * U * abs(alpha) * pr.S, abs(alpha) * pr.S, mx)
    else:
        scale = abs(alpha) * pr.S + C0.double().abs()
        check_f32(tag, "acc", out, ref, (K + 8 + ns + 1) * U * scale + U * abs(alpha) * pr.S, scale, mx)
        if cs is not None:
            scale = pr.A.abs().sum(1) + cs0.double().abs()
            check_f32(tag, "colsum", cs[:M], cs0.double() + pr.A.sum(1), (K + 8 + ns + 1) * U * scale, scale, mx)
    return runs[0]


@pytest.mark.parametrize("M,N,K", [(136, 72, 264), (264, 136, 200)])
def test_tt_f32(M, N, K):
    """gemm_kernel<1,1,EPI_F32>: both operands read through the transposing LDS reads, a K tail of 8, pitched operands and output."""
    mx = Maxima()
    for lda, ldb, pitch, alpha in [(None, None, 0, 1.0), (None, None, 4, -0.375), (M + 8, N + 16, 0, -0.375), (M + 8, N + 16, 4, 1.0)]:
        run_tt(f"tt f32 {M}x{N}x{K} lda={lda} ldb={ldb} pitch+{pitch} alpha={alpha}", R_TT_F32, F32, M, N, K, lda=lda, ldb=ldb, pitch=pitch, alpha=alpha, mx=mx)
    report(f"gemm_paths tt_f32 {M}x{N}x{K}", **mx)


@pytest.mark.parametrize("M,N,K,ldb,ws,ns", [(192, 192, 520, 5 * 192, False, 3), (136, 72, 200, None, False, 1), (136, 72, 200, None, True, 1)])
def test_tt_atomic(M, N, K, ldb, ws, ns):
    """gemm_kernel<1,1,EPI_ATOMIC,colsum>: real atomics from three slices (192 / 192 / 136) with a strided B, and the single-slice case
    that keeps this kernel even when a workspace is offered."""
    assert splitk(M, N, K) == ns and predict_tt(M, N, K, ws, 0) == R_TT_ATOMIC
    mx = Maxima()
    for pitch, alpha, colsum in [(0, 1.0, True), (4, -0.375, True), (0, -0.375, False)]:
        run_tt(f"tt atomic {M}x{N}x{K} ws={ws} pitch+{pitch} alpha={alpha} colsum={colsum}", R_TT_ATOMIC, ATOMIC, M, N, K, ldb=ldb, pitch=pitch,
               alpha=alpha, ws=ws, colsum=colsum, mx=mx)
    report(f"gemm_paths tt_atomic {M}x{N}x{K} ws={ws}", **mx)


@pytest.mark.parametrize("M,N,K,ns", [(192, 192, 520, 3), (136, 200, 264, 2)])
def test_tt_partial_reduce(M, N, K, ns):
    """gemm_kernel<1,1,EPI_PARTIAL,colsum> + splitk_reduce_kernel: ordered slabs, with and without the column sums (the slab stride differs)."""
    assert splitk(M, N, K) == ns and predict_tt(M, N, K, True, 0) == R_TT_PARTIAL
    mx = Maxima()
    for pitch, alpha, colsum in [(0, 1.0, True), (4, -0.375, True), (0, -0.375, False), (4, 1.0, False)]:
        run_tt(f"tt partial {M}x{N}x{K} pitch+{pitch} alpha={alpha} colsum={colsum}", R_TT_PARTIAL, ATOMIC, M, N, K, pitch=pitch, alpha=alpha, ws=True,
               colsum=colsum, mx=mx)
    report(f"gemm_paths tt_partial {M}x{N}x{K}", **mx)


@pytest.mark.parametrize("M,N,K,base,ns", [(512, 320, 512, R_WG42, 2), (1032, 328, 520, R_WG42, 3), (512, 320, 264, R_WG42, 2),
                                           (320, 512, 512, R_WG24, 2), (328, 1032, 520, R_WG24, 3), (320, 512, 264, R_WG24, 2)])
def test_wgrad8(M, N, K, base, ns):
    """wgrad8_kernel<4,2> / <2,4>, register-staged and LDS-DMA through ppf_gemm_test_wgrad_path: ragged tiles on both sides, a K tail (register
    path only), column sums, pitched operands; the two data paths must give the same bits."""
    from protopformer_amd import _lib
    assert splitk(M, N, K) == ns
    mx = Maxima()
    try:
        for lda, ldb, pitch, alpha, colsum in [(None, None, 0, 1.0, True), (M + 8, N + 16, 4, -0.375, True), (None, None, 0, -0.375, False)]:
            got = {}
            for path in (1, 2, 0):
                _lib.call("ppf_gemm_test_wgrad_path", path)
                route = base + int(K % 64 == 0 and path != 1)
                assert predict_tt(M, N, K, True, path) == route
                got[path] = run_tt(f"wgrad8 {M}x{N}x{K} path={path} lda={lda} pitch+{pitch} alpha={alpha} colsum={colsum}", route, ATOMIC, M, N, K, lda=lda,
                                   ldb=ldb, pitch=pitch, alpha=alpha, ws=True, colsum=colsum, mx=mx, repeat=path != 0)
            for path in (2, 0):
                assert same_bits(got[1][0], got[path][0]), f"wgrad8 {M}x{N}x{K}: path {path} and the register-staged path differ in C"
                assert not colsum or same_bits(got[1][1], got[path][1]), f"wgrad8 {M}x{N}x{K}: path {path} and the register-staged path differ in colsum"
    finally:
        _lib.call("ppf_gemm_test_wgrad_path", 0)
    report(f"gemm_paths wgrad8 {M}x{N}x{K}", **mx)


# ------------------------------------------------------------------------------------------------ integer patterns, refusals
@pytest.mark.parametrize("name", ["nt", "gemm128g", "gemm224g", "nn", "tt_f32", "tt_atomic", "tt_partial", "wgrad8_42", "wgrad8_24"])
def test_transpose_detecting(name):
    """Small integers placed asymmetrically in m, n and k (between the rows of pitched operands: values that must not be read): every kernel must
    return the exact product, so an (m, n)-swapped store or a k permutation that differs between A and B cannot pass."""
    from protopformer_amd import _lib
    form = (4, True, False, 1.0)
    try:
        if name == "nt":
            run_fused(name, R_NT, False, F32, 130, 260, 200, form, integer=True)
            run_fused(name, R_NT, False, BF16, 130, 260, 200, form, integer=True)
        elif name == "gemm128g":
            run_fused(name, R_G128, False, BF16, 16261, 516, 192, form, integer=True)
        elif name == "gemm224g":
            _lib.call("ppf_gemm_test_force_g224", 1)
            run_fused(name, R_G224, False, BF16, 449, 392, 192, (8, True, False, 1.0), integer=True)
        elif name == "nn":
            run_fused(name, R_NN, True, F32, 130, 264, 200, form, integer=True)
            run_fused(name, R_NN, True, BF16, 130, 264, 200, form, integer=True)
        elif name == "tt_f32":
            run_tt(name, R_TT_F32, F32, 264, 136, 200, lda=272, ldb=152, pitch=4, integer=True)
        elif name == "tt_atomic":
            run_tt(name, R_TT_ATOMIC, ATOMIC, 192, 192, 520, ldb=5 * 192, integer=True)
        elif name == "tt_partial":
            run_tt(name, R_TT_PARTIAL, ATOMIC, 192, 192, 520, lda=200, ws=True, integer=True)
        else:
            M, N, base = (1032, 328, R_WG42) if name == "wgrad8_42" else (328, 1032, R_WG24)
            for path, K in ((1, 520), (2, 512)):
                _lib.call("ppf_gemm_test_wgrad_path", path)
                run_tt(f"{name} path={path}", base + (path == 2), ATOMIC, M, N, K, lda=M + 8, ldb=N + 8, ws=True, integer=True)
    finally:
        _lib.call("ppf_gemm_test_force_g224", 0)
        _lib.call("ppf_gemm_test_wgrad_path", 0)


def test_argument_refusals():
    """One minimal offending call per PPF_CHECK_ARG of ppf_gemm_bf16: its error code, nothing launched (the route code keeps its value), the
    output sentinel untouched -- and the next valid call works."""
    M, N, K = 16, 16, 16
    a = torch.ones(64, 64, dtype=torch.bfloat16, device="cuda")
    b = torch.ones(64, 64, dtype=torch.bfloat16, device="cuda")
    C = torch.full((4096,), SENT, device="cuda")
    aux = torch.full((4096,), SENT, device="cuda")
    ok = dict(M=M, N=N, K=K, lda=16, ldb=16, ldc=16, ta=0, tb=0, epi=F32)
    assert gemm_raw(a, b, C, **ok) == R_NT
    C.fill_(SENT)
    before = last_kernel()
    off8 = lambda t: t.data_ptr() + 8
    cases = [("K = 0", ERR_SHAPE, dict(K=0)), ("M < 0", ERR_SHAPE, dict(M=-8)),
             ("lda % 8", ERR_ALIGN, dict(lda=20)), ("ldb % 8", ERR_ALIGN, dict(ldb=20)), ("ldc % 4", ERR_ALIGN, dict(ldc=18)), ("N % 4", ERR_ALIGN, dict(N=14)),
             ("A inner extent K % 8", ERR_ALIGN, dict(K=12)), ("A inner extent M % 8 (trans_a)", ERR_ALIGN, dict(M=12, ta=1, tb=1)),
             ("B inner extent N % 8 (trans_b)", ERR_ALIGN, dict(N=12, tb=1)),
             ("A pointer", ERR_ALIGN, dict(A=off8(a))), ("B pointer", ERR_ALIGN, dict(B=off8(b))), ("C pointer", ERR_ALIGN, dict(C=off8(C))),
             ("trans_a without trans_b", ERR_ARG, dict(ta=1, tb=0)),
             ("res pointer", ERR_ALIGN, dict(epi=RESID, res=off8(aux), ldres=16)), ("ldres % 4", ERR_ALIGN, dict(epi=RESID, res=aux, ldres=18)),
             ("aux_out pointer", ERR_ALIGN, dict(epi=GELU, aux_out=off8(aux), ldaux=16)), ("ldaux % 4", ERR_ALIGN, dict(epi=GELU, aux_out=aux, ldaux=18)),
             ("aux_in pointer", ERR_ALIGN, dict(epi=DGELU, aux_in=off8(aux), ldaux=16)),
             ("RESID without res", ERR_ARG, dict(epi=RESID)), ("GELU without aux_out", ERR_ARG, dict(epi=GELU)), ("DGELU without aux_in", ERR_ARG, dict(epi=DGELU)),
             ("NT has no ATOMIC", ERR_ARG, dict(epi=ATOMIC)), ("NT has no epilogue 7", ERR_ARG, dict(epi=7)),
             ("NN has no GELU", ERR_ARG, dict(tb=1, epi=GELU, aux_out=aux, ldaux=16)), ("NN has no SIGMOID", ERR_ARG, dict(tb=1, epi=SIGMOID)),
             ("NN has no RESID", ERR_ARG, dict(tb=1, epi=RESID, res=aux, ldres=16)),
             ("TT has no BF16", ERR_ARG, dict(ta=1, tb=1, epi=BF16)), ("TT has no DGELU", ERR_ARG, dict(ta=1, tb=1, epi=DGELU, aux_in=aux, ldaux=16))]
    for what, rc, change in cases:
        kw = dict(ok, **change)
        A_, B_, C_ = kw.pop("A", a), kw.pop("B", b), kw.pop("C", C)
        with pytest.raises(RuntimeError, match=rf"rc={rc}\)"):
            gemm_raw(A_, B_, C_, **kw)
        assert last_kernel() == before, f"{what}: a refused call changed the route code"
    torch.cuda.synchronize()
    assert torch.equal(bits(C), bits(torch.full((4096,), SENT))) and torch.equal(bits(aux), bits(torch.full((4096,), SENT))), "a refused call wrote to an output"
    assert gemm_raw(a, b, C, **dict(ok, tb=1)) == R_NN
    torch.cuda.synchronize()
    assert torch.equal(C[:M * N].cpu(), torch.full((M * N,), float(K))) and torch.equal(bits(C[M * N:]), bits(torch.full((4096 - M * N,), SENT)))
