"""The row-plumbing kernels (csrc/elementwise.hip, ppf_merge3_cast in csrc/cait.hip, ppf_axpby / ppf_axpbypcz in csrc/head.hip) on
their own: the token-reservation map, row gather / scatter, the strided copies of the class-attention stage, the bf16 wire format,
the add-on head's sigmoid backward, im2col and token assembly.  All are grid-stride loops behind a grid cap (2048 or 1024
workgroups of 256 lanes); every kernel is also run at a size that needs the loop's second trip.

Moves and casts are exact: they are compared as bit patterns, with payloads that hold NaN and inf patterns, so a copy that goes
through arithmetic is caught.  The few rounded results are held to derived bounds (u = 2**-24) against fp64, stated at the gate."""
import numpy as np
import pytest
import torch

from helpers import report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 2048 * 256                       # lanes of the capped grid in elementwise.hip / cait.hip
CAP_HEAD = 1024 * 256                  # ... and of the axpby kernels in head.hip
LONG8 = 8 * (CAP + 37)                 # casts handle 8 elements per lane


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def payload(shape, dtype, g):
    """Random BIT PATTERNS of the dtype (NaNs with payloads, infs, denormals among them), plus a few explicit specials."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        raw = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        special = torch.tensor([0x7FC00000, 0x7F800001, 0x7F800000, 0xFF800000 - 2 ** 32, 0xFFFFFFFF - 2 ** 32, 0x00000001, 0x80000000 - 2 ** 32], dtype=torch.int64).to(torch.int32)
    else:
        raw = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int64).to(torch.int16)
        special = torch.tensor([0x7FC0, 0x7F81, 0x7F80, 0xFF80 - 2 ** 16, 0xFFFF - 2 ** 16, 0x0001, 0x8000 - 2 ** 16], dtype=torch.int64).to(torch.int16)
    k = min(n, special.numel())
    raw[torch.randperm(n, generator=g)[:k]] = special[:k]
    return raw.view(dtype).reshape(shape)


def bf16_rne(v):
    """fp64 -> nearest bf16 (ties to even) as fp64, in one rounding."""
    m, e = torch.frexp(v)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def ulp_bf16(v):
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), e - 8)


# ------------------------------------------------------------------------------------------------ token reservation
@pytest.mark.parametrize("B,k,N", [(1, 1, 2), (3, 9, 17), (8, 31, 40), (5, 81, 197), (7, 196, 197)])
def test_reserved_rows_map(B, k, N):
    """rows[b (k+1)] = b N, rows[b (k+1) + 1 + j] = b N + 1 + idx[b][j]; B (k+1) = 2, 30, 256 (one full workgroup), 410, 1379."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + k)
    idx = torch.stack([torch.randperm(N - 1, generator=g)[:k] for _ in range(B)]).to(torch.int32)      # unsorted, distinct
    got = ops.reserved_rows_map(idx.cuda(), N).cpu().numpy()
    ref = np.concatenate([np.zeros((B, 1), np.int64), 1 + idx.numpy().astype(np.int64)], 1) + np.arange(B)[:, None] * N
    assert got.dtype == np.int32 and np.array_equal(got, ref.reshape(-1))


def test_reserved_rows_map_refuses_n_le_k():
    from protopformer_amd import _lib
    idx = torch.zeros((2, 5), dtype=torch.int32, device="cuda")
    rows = torch.full((12,), -7, dtype=torch.int32, device="cuda")
    for N in (5, 4):
        with pytest.raises(RuntimeError):
            _lib.call("ppf_reserved_rows_map", idx, rows, 2, 5, N)
    torch.cuda.synchronize()
    assert bool((rows == -7).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("row_bytes", [16, 48, 1536])
def test_gather_scatter_rows(dtype, row_bytes):
    from protopformer_amd import _lib, ops
    g = torch.Generator().manual_seed(row_bytes)
    D = row_bytes // (4 if dtype == torch.float32 else 2)
    n = 37
    x = payload((n, D), dtype, g)
    xd = x.cuda()
    # gather: duplicates, out of order; CaiT's all-zero map broadcasts one row B times
    for rows in (torch.randint(0, n, (50,), generator=g), torch.zeros(5, dtype=torch.int64), torch.tensor([n - 1])):
        got = ops.gather_rows(xd, rows.to(torch.int32).cuda())
        assert same_bits(got, x[rows]), f"gather_rows {dtype} row_bytes={row_bytes}"
    # scatter into a NaN-filled destination: listed rows exact, every other row exactly zero
    rows = torch.randperm(n + 20, generator=g)[:n]
    dst = torch.full((n + 20, D), float("nan"), dtype=dtype, device="cuda")
    _lib.call("ppf_scatter_rows", xd, rows.to(torch.int32).cuda(), dst, n, n + 20, row_bytes)
    ref = torch.zeros((n + 20, D), dtype=dtype)
    ref[rows] = x
    assert same_bits(dst, ref), f"scatter_rows {dtype} row_bytes={row_bytes}"
    # scatter(gather(x, rows), rows, n) = x on the listed rows, zero elsewhere
    rows = torch.randperm(n, generator=g)[:20]
    rd = rows.to(torch.int32).cuda()
    back = ops.scatter_rows(ops.gather_rows(xd, rd), rd, n)
    ref = torch.zeros((n, D), dtype=dtype)
    ref[rows] = x[rows]
    assert same_bits(back, ref), "scatter_rows(gather_rows(x))"


def test_gather_scatter_rows_past_grid_cap():
    """8 200 rows of 96 16-byte words = 787 200 words for a grid of 524 288 lanes."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(5)
    n, D = 8200, 384
    assert n * (D * 4 // 16) > CAP
    x = payload((300, D), torch.float32, g)
    rows = torch.randint(0, 300, (n,), generator=g)
    got = ops.gather_rows(x.cuda(), rows.to(torch.int32).cuda())
    ref = x[rows]
    assert same_bits(got, ref)
    where = torch.randperm(n + 100, generator=g)[:n]
    back = ops.scatter_rows(got, where.to(torch.int32).cuda(), n + 100)
    full = torch.zeros((n + 100, D))
    full[where] = ref
    assert same_bits(back, full)


def test_gather_scatter_rows_refuse_unaligned():
    """row_bytes = 24 is no multiple of 16: refused, destination untouched (the scatter's memset included)."""
    from protopformer_amd import _lib
    src = torch.ones((4, 6), device="cuda")
    rows = torch.tensor([3, 1, 0, 2], dtype=torch.int32, device="cuda")
    dst = torch.full((4, 6), -3.5, device="cuda")
    with pytest.raises(RuntimeError):
        _lib.call("ppf_gather_rows", src, rows, dst, 4, 24)
    with pytest.raises(RuntimeError):
        _lib.call("ppf_scatter_rows", src, rows, dst, 4, 4, 24)
    torch.cuda.synchronize()
    assert bool((dst == -3.5).all())


# ------------------------------------------------------------------------------------------------ strided copies
def _copy_case(src_cols, dst_cols, c0_src, c0_dst, width, rows, g, dtype=torch.float32):
    """dst[:, c0_dst : c0_dst + width] = src[:, c0_src : c0_src + width]; everything else in dst must keep its sentinel."""
    from protopformer_amd import ops
    src = payload((rows, src_cols), dtype, g)
    sent = payload((1, 1), dtype, g).expand(rows, dst_cols).contiguous()
    dst = sent.clone().cuda()
    ops.copy_2d(dst[:, c0_dst:c0_dst + width], src.cuda()[:, c0_src:c0_src + width])
    ref = sent.clone()
    ref[:, c0_dst:c0_dst + width] = src[:, c0_src:c0_src + width]
    assert same_bits(dst, ref), f"copy_2d src_cols={src_cols} dst_cols={dst_cols} offsets {c0_src}/{c0_dst} width={width} rows={rows}"


def test_copy_2d_kernel_path():
    """Pointers, pitches and width all multiples of 16 bytes: copy_2d_kernel.  src_pitch > width, dst_pitch > width."""
    g = torch.Generator().manual_seed(21)
    _copy_case(24, 16, 4, 4, 8, 37, g)                  # sub-matrix on both sides
    _copy_case(8, 8, 0, 0, 8, 1, g)                     # one full row
    _copy_case(16, 24, 8, 0, 8, 300, g, torch.bfloat16)
    _copy_case(388, 384, 4, 0, 384, 8200, g)            # 8 200 x 96 words > 524 288 lanes, pitched source
    assert 8200 * 96 > CAP


@pytest.mark.parametrize("what", ["width_24_bytes", "source_offset_one_element", "pitch_not_16"])
def test_copy_2d_runtime_fallback(what):
    """One side off the 16-byte grid: the runtime's rectangular copy does the same job."""
    g = torch.Generator().manual_seed(22)
    if what == "width_24_bytes":
        _copy_case(24, 16, 4, 4, 6, 37, g)
    elif what == "source_offset_one_element":
        _copy_case(24, 16, 1, 4, 8, 37, g)
    else:
        _copy_case(13, 16, 0, 4, 8, 37, g)              # 52-byte source pitch


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,D", [(1, 1, 4), (3, 196, 192), (130, 17, 64)])
def test_cat_rows(B, N, D, dtype):
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(B + N + D)
    first, rest = payload((B, 1, D), dtype, g), payload((B, N, D), dtype, g)
    got = ops.cat_rows(first.cuda(), rest.cuda())
    assert same_bits(got, torch.cat([first, rest], 1))


# ------------------------------------------------------------------------------------------------ bf16 wire format
# fp32 bit patterns: ties between two bf16 neighbours (to even: down and up), +-0, denormals (and a denormal tie), the largest finite
# value (rounds to inf), +-inf, quiet / signalling / negative NaNs (a truncating cast turns 0x7F800001 into inf)
SPECIAL_F32 = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000000, 0x80000000, 0x00000001, 0x007FFFFF,
               0x00008000, 0x00018000, 0x80008000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001,
               0xFFFFFFFF, 0x7FFF8000, 0x3F800000, 0x477FE000]


def _f32_from_bits(words):
    return torch.tensor([w - 2 ** 32 if w >= 2 ** 31 else w for w in words], dtype=torch.int64).to(torch.int32).view(torch.float32)


def _check_cast(x):
    from protopformer_amd import ops
    got, ref = ops.cast_bf16(x.cuda()).cpu(), x.bfloat16()
    nan = torch.isnan(x)
    assert bool(torch.isnan(got[nan]).all()), "a NaN came out as a number"          # NaN compared as NaN, not by payload
    assert torch.equal(bits(got)[~nan], bits(ref)[~nan]), f"{int((bits(got)[~nan] != bits(ref)[~nan]).sum())} values differ from round-to-nearest-even"


def test_cast_f32_bf16():
    g = torch.Generator().manual_seed(31)
    sp = _f32_from_bits(SPECIAL_F32)
    _check_cast(_f32_from_bits([0x3F808000, 0x3F818000, 0x7F7FFFFF, 0x7F800001, 0x80000000, 0x00018000, 0xFF800000, 0xBF818000]))     # n = 8
    x = torch.randn(LONG8, generator=g) * torch.exp(4 * torch.randn(LONG8, generator=g))
    pos = torch.randperm(LONG8, generator=g)[:64 * sp.numel()]                       # the specials tiled through the long vector
    x[pos] = sp.repeat(64)
    x[-sp.numel():] = sp                                                             # ... and in the loop's second trip
    _check_cast(x)


def test_cast_f32_bf16_refuses_n12():
    from protopformer_amd import _lib
    out = torch.full((16,), 3.0, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        _lib.call("ppf_cast_f32_bf16", torch.ones(16, device="cuda"), out, 12)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


def test_cast_bf16_f32_all_patterns():
    """Widening is exact: every one of the 65 536 bf16 patterns comes out as pattern << 16 (NaN payloads included)."""
    from protopformer_amd import _lib
    g = torch.Generator().manual_seed(32)
    for pat in (torch.arange(65536, dtype=torch.int64), torch.randint(0, 65536, (LONG8,), generator=g, dtype=torch.int64)):
        src = (pat - (pat >= 32768) * 65536).to(torch.int16)
        out = torch.empty(pat.numel(), device="cuda")
        _lib.call("ppf_cast_bf16_f32", src.view(torch.bfloat16).cuda(), out, pat.numel())
        assert torch.equal(bits(out).to(torch.int64) & 0xFFFFFFFF, pat << 16)


# ------------------------------------------------------------------------------------------------ CaiT gradient merge
@pytest.mark.parametrize("N1,D,B", [(1, 2, 3), (17, 2, 3), (197, 2, 2), (1, 192, 5), (17, 192, 3), (197, 192, 2), (197, 192, 30)])
def test_merge3_cast(N1, D, B):
    """out = bf16((a + b) + cq[r / N1]) on rows r % N1 == 0, bf16(a + b) elsewhere.  Two fp32 additions and one rounding, nothing to
    contract into an FMA: bit-exact against the same expression in torch fp32 (measured: 0 mismatches).  The last size has
    5 910 x 96 column pairs > 524 288 lanes."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(N1 * 7 + D + B)
    rows = B * N1
    a, b, cq = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g), torch.randn(B, D, generator=g) * 2
    ref = a + b
    ref[::N1] = ref[::N1] + cq
    got = ops.merge3_cast(a.cuda(), b.cuda(), cq.cuda(), N1)
    assert same_bits(got, ref.bfloat16()), f"{int((bits(got) != bits(ref.bfloat16())).sum())} of {rows * D} values differ"
    if B == 30:
        assert rows * D // 2 > CAP


# ------------------------------------------------------------------------------------------------ scalars and linear combinations
@pytest.mark.parametrize("n", [1, 257, CAP + 5])
def test_scale_by_scalar(n):
    """One fp32 multiply per element by a device-resident scalar: bit-exact to torch's."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * torch.exp(3 * torch.randn(n, generator=g))
    x[0] = float("inf")
    s = torch.tensor(-0.3718)
    got = ops.scale_by_scalar(x.cuda(), s.cuda())
    assert same_bits(got, x * s)


@pytest.mark.parametrize("n", [1, 257, CAP_HEAD + 5])
def test_axpby_axpbypcz(n):
    """|err| <= 2**-23 (|a x| + |b y| (+ |c z|)) against fp64: two roundings per result, fused or not -- a x is rounded, b y is added
    in one (fused) or two steps.  axpbypcz runs with a = 1 as in its one caller (loss = ce + c1 cov + c2 mean), where a x is exact and
    the two roundings are those of the two additions.  Measured max: axpby 0.94, axpbypcz 0.95 of the bound.  out may alias x."""
    from protopformer_amd import _lib, ops
    g = torch.Generator().manual_seed(n + 1)
    x, y, z = (torch.randn(n, generator=g) * torch.exp(2 * torch.randn(n, generator=g)) for _ in range(3))
    vals = {}
    for name, (a, b, c) in (("axpby", (0.7, -1.3, None)), ("axpbypcz", (1.0, 0.1, 0.5))):
        a32, b32 = float(np.float32(a)), float(np.float32(b))                 # the coefficients travel as floats
        ref = a32 * x.double() + b32 * y.double()
        mass = (a32 * x.double()).abs() + (b32 * y.double()).abs()
        if c is None:
            got = ops.axpby(x.cuda(), y.cuda(), a, b)
            alias = x.clone().cuda()
            assert ops.axpby(alias, y.cuda(), a, b, out=alias) is alias
        else:
            c32 = float(np.float32(c))
            ref, mass = ref + c32 * z.double(), mass + (c32 * z.double()).abs()
            got = ops.axpbypcz(x.cuda(), y.cuda(), z.cuda(), a, b, c)
            alias = x.clone().cuda()
            _lib.call("ppf_axpbypcz", alias, y.cuda(), z.cuda(), alias, a, b, c, n)
        assert same_bits(alias, got), f"{name}: out aliasing x changes the result"
        err = (got.cpu().double() - ref).abs()
        bound = 2.0 ** -23 * mass
        vals[name] = float((err / bound).max())
        assert not bool((err > bound).any()), f"{name}: {vals[name]:.3f} of 2**-23 (|a x| + |b y| ...)"
    report(f"axpby n={n}", **vals)


# ------------------------------------------------------------------------------------------------ add-on head: sigmoid backward
@pytest.mark.parametrize("rows,cols", [(1, 1), (37, 300), (20992, 64), (32801, 8)])
def test_sigmoid_bwd(rows, cols):
    """dz = bf16(df f (1 - f)): within one bf16 ulp of the fp64 value (three fp32 roundings in front of the bf16 one: NOT bit-exact
    against bf16 of fp64 -- measured: 10 of 1 343 488 values land on the neighbour -- but bit-exact against the same expression in
    torch fp32, which is asserted too).  dbias += column sums of the ROUNDED dz: compared with the fp64 column sum of the kernel's
    own dz within rows u (|prefill| + sum|dz|) -- the prefilled value is one more term.  32 801 rows double rows_per_block (2 048 blocks)."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(rows + cols)
    f = torch.sigmoid(2 * torch.randn(rows, cols, generator=g))
    df = torch.randn(rows, cols, generator=g)
    init = torch.randn(cols, generator=g)
    fd, dfd = f.cuda(), df.cuda()
    runs = []
    for _ in range(2):
        dbias = init.clone().cuda()
        runs.append((ops.sigmoid_bwd(dfd, fd, dbias).cpu(), dbias.cpu()))
    dz, dbias = runs[0]
    assert same_bits(dz, runs[1][0]) and same_bits(dbias, runs[1][1]), "second run differs"          # fixed-order reduce
    v = df.double() * f.double() * (1 - f.double())
    err = (dz.double() - v).abs()
    assert not bool((err > ulp_bf16(v)).any()), f"dz more than one bf16 ulp off: {float((err / ulp_bf16(v)).max()):.3f}"
    mism = int((bits(dz) != bits(bf16_rne(v).bfloat16())).sum())
    assert same_bits(dz, (df * f * (1.0 - f)).bfloat16()), "dz differs from the fp32 expression"
    ref = init.double() + dz.double().sum(0)
    bound = rows * U * (init.double().abs() + dz.double().abs().sum(0))
    e = (dbias.double() - ref).abs()
    frac = float((e / bound).max())                                                                      # measured max 0.014 (37 rows), 6e-7 at 32 801 rows
    assert not bool((e > bound).any()), f"dbias at {frac:.3f} of rows u sum|dz|"
    report(f"sigmoid_bwd {rows}x{cols}", dz_ulp=float((err / ulp_bf16(v)).max()), dz_not_rne_of_fp64=mism / dz.numel(), dbias_frac=frac)
    only = ops.sigmoid_bwd(dfd, fd, None)                                                                 # dbias = NULL: dz only
    assert same_bits(only.cpu(), dz)


# ------------------------------------------------------------------------------------------------ patch embedding plumbing
def test_im2col_past_grid_cap():
    """30 x 3 x 224 x 224: 564 480 groups of 8 pixels for 524 288 lanes."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(41)
    B, p = 30, 16
    assert B * 3 * 224 * 224 // 8 > CAP
    img = torch.randn(B, 3, 224, 224, generator=g)
    cols = ops.im2col_patch(img.cuda(), p).cpu()
    ref = img.reshape(B, 3, 14, p, 14, p).permute(0, 2, 4, 1, 3, 5).reshape(B * 196, 3 * p * p).bfloat16()
    assert same_bits(cols, ref)


def test_assemble_tokens_past_grid_cap():
    """B = 32, Np = 196, D = 384, lead 1: 605 184 float4 for 524 288 lanes; one fp32 addition per element, exact."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(42)
    B, Np, D = 32, 196, 384
    assert B * (Np + 1) * D // 4 > CAP
    tok, cls, pos = torch.randn(B * Np, D, generator=g), torch.randn(D, generator=g), torch.randn(Np + 1, D, generator=g)
    x = ops.assemble_tokens(tok.cuda(), cls.cuda(), pos.cuda(), B, Np, D, 1).cpu()
    assert same_bits(x, torch.cat([cls.expand(B, 1, D), tok.reshape(B, Np, D)], 1) + pos)


@pytest.mark.parametrize("lead", [1, 0])
@pytest.mark.parametrize("B", [1, 2, 5])
def test_assemble_tokens_bwd_ragged_batch(B, lead):
    """The four waves of a workgroup sum a quarter of the batch each, ceil(B/4) samples: B = 1, 2, 5 leave quarters short or empty.
    Exact against the kernel's own order in torch fp32: each quarter from zero in batch order, then dpos += (q0 + q1) + (q2 + q3).
    D = 130: the second column block has one active lane."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(50 + B)
    Np, D = 5, 130
    T = Np + lead
    dx = torch.randn(B, T, D, generator=g)
    dpos0, dcls0 = torch.randn(T, D, generator=g), torch.randn(D, generator=g)
    dpos, dcls = dpos0.clone().cuda(), dcls0.clone().cuda()
    dtok = ops.assemble_tokens_bwd(dx.cuda(), dpos, dcls, B, Np, D, lead).cpu()
    bq = (B + 3) // 4
    q = []
    for i in range(4):
        acc = torch.zeros(T, D)
        for b in range(i * bq, min(B, (i + 1) * bq)):
            acc = acc + dx[b]
        q.append(acc)
    s = (q[0] + q[1]) + (q[2] + q[3])
    assert same_bits(dpos, dpos0 + s), "dpos"
    assert same_bits(dcls, dcls0 + s[0] if lead else dcls0), "dcls"
    assert same_bits(dtok, dx[:, lead:].reshape(B * Np, D).bfloat16()), "dtok"
