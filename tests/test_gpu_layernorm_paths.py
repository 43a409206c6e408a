"""LayerNorm forward / backward (csrc/layernorm.hip) against an fp64 reference on every dispatch path: all forward widths, all 14
backward instantiations with and without the LayerScale operands, row_map on both sides, the dy=None pass, in-place dx, the atomics
path of the C ABI, row counts past both grid caps, rows = 1 and the refused widths.

Every gate is a derived bound in units of u = 2**-24 with all scales taken from the fp64 reference (no tuned number); the factor 16
leaves room for rsqrtf, FMA contraction and the shuffle-tree order (a plain fp32 torch implementation stays within 3.3 u on these
inputs).  The measured maxima, in u, go to helpers.report and stand next to their gates.

Inputs: x = 2 randn + 0.5 with three hard rows (row 0 constant 3.25, row 1 = 3 + 1e-3 randn, row 2 = 100 + randn), w = 1 + 0.2 randn,
b = 0.1 randn, dy bf16, dres fp32.  The backward receives mean / rstd computed in fp64 and rounded to fp32 and the reference uses
the same rounded values, so the backward is judged on its own.  eps is the fp32 value the C ABI receives.

bf16 outputs (y, cast_out): "half a bf16 ulp plus the fp32 allowance a" is checked in its exact form -- the output must lie between
bf16(v - a) and bf16(v + a), the correct roundings of the two ends of the allowed fp32 interval (rounding is monotone).  That is never
looser than |err| <= half_ulp(v) + a.  (The shorthand 2**-9 |v| for half an ulp is its LOWER edge: half a bf16 ulp of v is between
2**-9 |v| and 2**-8 |v|, so a correctly rounded value misses `2**-9 |v|` whenever v sits low in its binade, e.g. 1.0038 -> 1.0.)

Column sums start from non-zero contents (+= semantics); the prefilled value is one more term of the sum, so its magnitude is part
of sum|term| in the any-order bound (rows + 8) u sum|term| (test_gpu_explain.py's convention).

Each gate was shown to bite on value-only edits of the kernels: rowscale indexed by the compact row in ln_bwd2 (caught by
test_bwd_row_map), c2 taken from s1 in the generic backward, rstd stored without eps, the partner row dropped from ln_bwd2's flush."""
import numpy as np
import pytest
import torch

from helpers import SENT, U, bf16_rne, bits, half_ulp_bf16, maxu, report

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-6))           # the C entry point takes eps as a float
K = 16.0                                # allowance factor of every fp32 gate, in u


def make_x(rows, D, g):
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    hard = [torch.full((D,), 3.25), 3 + 1e-3 * torch.randn(D, generator=g), 100 + torch.randn(D, generator=g)]
    for i in range(min(rows, 3)):
        x[i] = hard[i]
    return x


def make_wb(D, g):
    return 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


# ------------------------------------------------------------------------------------------------ forward
def fwd_ref(x, w, b):
    x, w, b = x.double(), w.double(), b.double()
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    rs = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + EPS)
    xh = xc * rs
    return dict(mu=mu[:, 0], rs=rs[:, 0], y=xh * w + b,
                s_mean=x.abs().mean(-1),
                s_rstd=(rs * (1 + rs * rs * (xc.abs() * (x.abs() + mu.abs())).mean(-1, keepdim=True)))[:, 0],
                s_y=w.abs() * (rs * (x.abs() + mu.abs()) + xh.abs()) + b.abs())


def check_fwd(tag, got, ref):
    y, mean, rstd = (t.cpu().double() for t in got)
    assert y.shape == ref["y"].shape and mean.shape == ref["mu"].shape and rstd.shape == ref["rs"].shape, f"{tag}: output shapes"
    m_u = maxu((mean - ref["mu"]).abs(), ref["s_mean"])
    r_u = maxu((rstd - ref["rs"]).abs(), ref["s_rstd"])
    a = K * U * ref["s_y"]
    lo, hi = bf16_rne(ref["y"] - a), bf16_rne(ref["y"] + a)
    y_u = maxu(((y - ref["y"]).abs() - half_ulp_bf16(ref["y"])).clamp_min(0), ref["s_y"])      # fp32 part of the error: beyond half a bf16 ulp
    report(tag, mean_u=m_u, rstd_u=r_u, y_u=y_u)
    assert m_u <= K, f"{tag}: mean off by {m_u:.2f} u (gate {K})"                               # measured max 1.72 u
    assert r_u <= K, f"{tag}: rstd off by {r_u:.2f} u (gate {K})"                               # measured max 1.02 u
    bad = (y < lo) | (y > hi)
    assert not bool(bad.any()), f"{tag}: y outside [bf16(v - 16u S), bf16(v + 16u S)] at {int(bad.sum())} places ({y_u:.2f} u beyond half a bf16 ulp)"   # measured max 0.85 u


@pytest.mark.parametrize("D", [64, 96, 130, 200, 322, 500, 512, 768, 1024])
def test_fwd_every_nj(D):
    """ln_fwd_kernel<1,2,3,4,6,8>; at D = 130 only lane 0 is active in the second column block; rows = 1 leaves three waves idle."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(100 + D)
    w, b = make_wb(D, g)
    for rows in (1, 3, 77):
        x = make_x(rows, D, g)
        check_fwd(f"ln_fwd D={D} rows={rows}", ops.layernorm_fwd(x.cuda(), w.cuda(), b.cuda()), fwd_ref(x, w, b))


def test_fwd_past_grid_cap():
    """16 397 rows: the grid is capped at 4096 workgroups of four rows, so the first 13 rows take a second trip."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(7)
    rows, D = 16397, 64
    x = make_x(rows, D, g)
    w, b = make_wb(D, g)
    check_fwd("ln_fwd rows=16397", ops.layernorm_fwd(x.cuda(), w.cuda(), b.cuda()), fwd_ref(x, w, b))


@pytest.mark.parametrize("kind", ["permutation", "duplicates", "shorter", "long"])
def test_fwd_row_map(kind):
    """x is read at row_map[r], y / mean / rstd are written at r and have len(row_map) rows."""
    from protopformer_amd import ops
    g = torch.Generator().manual_seed(11)
    D, nsrc = (64, 300) if kind == "long" else (200, 40)
    x = make_x(nsrc, D, g)
    w, b = make_wb(D, g)
    rm = {"permutation": lambda: torch.randperm(nsrc, generator=g),
          "duplicates": lambda: torch.tensor([5, 0, 39, 7, 7, 2, 1, 0, 0, 39, 38, 5, 1]),
          "shorter": lambda: torch.cat([torch.tensor([2, 0, 1]), 3 + torch.randperm(nsrc - 3, generator=g)[:6]]),      # the hard rows, out of order
          "long": lambda: torch.randint(0, nsrc, (16397,), generator=g)}[kind]()
    got = ops.layernorm_fwd(x.cuda(), w.cuda(), b.cuda(), row_map=rm.to(torch.int32).cuda())
    assert got[0].shape == (rm.numel(), D)
    check_fwd(f"ln_fwd row_map {kind}", got, fwd_ref(x[rm], w, b))


# ------------------------------------------------------------------------------------------------ backward
def make_bwd(rows, D, g, *, ls, nsrc=None, row_map=None, dres=True, dy=True, groups=None, zero_sums=False):
    """CPU operands of one backward call.  x / dres / branch / outputs have nsrc rows, dy / mean / rstd have `rows`."""
    nsrc = rows if nsrc is None else nsrc
    c = dict(rows=rows, D=D, nsrc=nsrc, row_map=row_map, ls=ls)
    c["x"] = make_x(nsrc, D, g)
    c["w"], _ = make_wb(D, g)
    c["dy"] = torch.randn(rows, D, generator=g).bfloat16() if dy else None
    c["dres"] = torch.randn(nsrc, D, generator=g) if dres else None
    src = row_map.long() if row_map is not None else torch.arange(rows)
    xs = c["x"][src].double()
    mu = xs.mean(-1, keepdim=True)
    c["mean"] = mu[:, 0].float()
    c["rstd"] = (1.0 / torch.sqrt(((xs - mu) ** 2).mean(-1) + EPS)).float()
    if groups is None:                          # the existing test's three groups, one of them zero
        c["rowscale"], c["rpg"] = torch.tensor([0.0, 1.0 / 0.9, 1.0]), (nsrc + 2) // 3
    else:
        c["rowscale"], c["rpg"] = groups
    c["colscale"] = (0.5 + torch.rand(D, generator=g)) if ls else None
    c["branch"] = torch.randn(nsrc, D, generator=g).bfloat16() if ls else None
    names = ("dw", "db", "dbn", "dcs") if ls else ("dw", "db", "dbn")
    c["init"] = {k: (torch.zeros(D) if zero_sums else torch.randn(D, generator=g) * 3) for k in names}
    return c


def bwd_ref(c):
    rows, D = c["rows"], c["D"]
    src = c["row_map"].long() if c["row_map"] is not None else torch.arange(rows)
    dres = c["dres"][src].double() if c["dres"] is not None else torch.zeros(rows, D, dtype=torch.float64)
    if c["dy"] is not None:
        rs = c["rstd"].double()[:, None]
        xh = (c["x"][src].double() - c["mean"].double()[:, None]) * rs
        dy = c["dy"].double()
        g = dy * c["w"].double()
        dx = dres + rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        s_dx = dres.abs() + rs * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
        tw, tb = dy * xh, dy
    else:
        dx, s_dx, tw, tb = dres, dres.abs(), None, None
    rsc = c["rowscale"].double()[src // c["rpg"]][:, None]
    cs = c["colscale"].double() if c["colscale"] is not None else torch.ones(D, dtype=torch.float64)
    r = dict(src=src, dx=dx, s_dx=s_dx, tw=tw, tb=tb, cast=dx * rsc * cs, a_cast=K * U * s_dx * (rsc * cs).abs())
    if c["branch"] is not None:
        br = c["branch"][src].double()
        r["tcs"], r["a_dcs"] = dx * rsc * br, (K * U * s_dx * (rsc * br).abs()).sum(0)
    return r


def run_bwd(c, *, atomics=False, inplace=False, fill=None):
    """One call on the GPU; returns the outputs on the CPU.  fill: dx_out / cast_out start from this value (row_map leaves rows untouched)."""
    from protopformer_amd import _lib, ops
    dev = lambda t: None if t is None else t.cuda()
    D, nsrc = c["D"], c["nsrc"]
    sums = {k: v.clone().cuda() for k, v in c["init"].items()}
    dres = dev(c["dres"])
    dx = dres if inplace else torch.full((nsrc, D), SENT if fill is None else fill, device="cuda")
    cast = torch.full((nsrc, D), SENT if fill is None else fill, dtype=torch.bfloat16, device="cuda")
    have_dy = c["dy"] is not None
    a = [dev(c["dy"]), dev(c["x"]) if have_dy else None, None if c["row_map"] is None else c["row_map"].to(torch.int32).cuda(),
         dev(c["w"]) if have_dy else None, dev(c["mean"]) if have_dy else None, dev(c["rstd"]) if have_dy else None]
    kw = dict(dres_in=dres, dx_out=dx, cast_out=cast, rowscale=dev(c["rowscale"]), rows_per_group=c["rpg"], colscale=dev(c["colscale"]),
              dbias_next=sums["dbn"], branch=dev(c["branch"]), dcolscale=sums.get("dcs"))
    if atomics:                                                       # partial == NULL, size 0: only the C ABI reaches it
        _lib.call("ppf_layernorm_bwd", a[0], a[1], a[2], a[3], a[4], a[5], dres, dx, sums["dw"], sums["db"], cast, kw["rowscale"], c["rpg"],
                  kw["colscale"], sums["dbn"], kw["branch"], kw["dcolscale"], c["rows"], D, None, 0)
    else:
        ops.layernorm_bwd(a[0], a[1], a[3], a[4], a[5], sums["dw"], sums["db"], row_map=a[2], **kw)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in sums.items()}
    out["dx"], out["cast"] = dx.cpu(), cast.cpu()
    return out


def colsum_gate(tag, name, got, init, terms, extra=0.0):
    """got = init + sum over rows of terms, any order: |err| <= (rows + 8) u (|init| + sum|term|) (+ a propagated allowance)."""
    n = terms.shape[0]
    ref, mass = init.double() + terms.sum(0), init.double().abs() + terms.abs().sum(0)
    err = (got.double() - ref).abs()
    bound = (n + 8) * U * mass + extra
    rel = maxu(err, bound / U)                          # fraction of the bound
    assert not bool((err > bound).any()), f"{tag}: {name} at {rel:.3f} of the any-order bound ({n} rows)"
    return rel


def check_bwd(tag, c, out, r=None):
    r = bwd_ref(c) if r is None else r
    src, rows = r["src"], c["rows"]
    vals = {}
    dx = out["dx"][src].double()
    vals["dx_u"] = maxu((dx - r["dx"]).abs(), r["s_dx"])
    assert vals["dx_u"] <= K, f"{tag}: dx off by {vals['dx_u']:.2f} u (gate {K})"                       # measured max 2.40 u
    cast = out["cast"][src].double()
    lo, hi = bf16_rne(r["cast"] - r["a_cast"]), bf16_rne(r["cast"] + r["a_cast"])
    bad = (cast < lo) | (cast > hi)
    vals["cast_u"] = maxu(((cast - r["cast"]).abs() - half_ulp_bf16(r["cast"])).clamp_min(0), r["a_cast"] / (K * U))
    assert not bool(bad.any()), f"{tag}: cast_out outside [bf16(v - a), bf16(v + a)] at {int(bad.sum())} places ({vals['cast_u']:.2f} u beyond half a bf16 ulp)"   # measured max 0.80 u
    if r["tw"] is not None:
        vals["dw_frac"] = colsum_gate(tag, "dw", out["dw"], c["init"]["dw"], r["tw"])               # measured max 0.19 of the bound
        vals["db_frac"] = colsum_gate(tag, "db", out["db"], c["init"]["db"], r["tb"])               # measured max 0.11
    else:
        assert torch.equal(bits(out["dw"]), bits(c["init"]["dw"])) and torch.equal(bits(out["db"]), bits(c["init"]["db"])), f"{tag}: dy=None touched dw / db"
    # the bias gradient of the branch GEMM sums the ROUNDED values: exact reference = fp64 column sum of the kernel's own cast_out
    err = (out["dbn"].double() - (c["init"]["dbn"].double() + cast.sum(0))).abs()
    bound = rows * U * (c["init"]["dbn"].double().abs() + cast.abs().sum(0))
    vals["dbn_frac"] = maxu(err, bound / U)                                                         # measured max 0.50 (rows = 2: one rounding)
    assert not bool((err > bound).any()), f"{tag}: dbias_next at {vals['dbn_frac']:.3f} of rows u sum|cast|"
    if "tcs" in r:
        vals["dcs_frac"] = colsum_gate(tag, "dcolscale", out["dcs"], c["init"]["dcs"], r["tcs"], extra=r["a_dcs"])     # measured max 0.09
    report(tag, **vals)
    return r


def assert_same_bits(tag, a, b):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{tag}: {k} differs between two runs"


V4, V2, GENERIC = [128, 256, 384, 512], [64, 192, 320, 448], [96, 200, 322, 500, 768, 1024]


@pytest.mark.parametrize("ls", [True, False], ids=["LS", "plain"])
@pytest.mark.parametrize("D", V4 + V2 + GENERIC)
def test_bwd_every_instantiation(D, ls):
    """ln_bwd2_kernel<4,{1..4}>, <2,{1,3,5,7}> and ln_bwd_kernel<{1,2,3,4,6,8}>, each with and without the LayerScale operands.
    rows = 1: the second half-wave of ln_bwd2 has no row; odd row counts end on a half-wave pair with one row."""
    g = torch.Generator().manual_seed(1000 + D + ls)
    for rows in (1, 2, 33, 77):
        c = make_bwd(rows, D, g, ls=ls)
        tag = f"ln_bwd D={D} rows={rows} {'LS' if ls else 'plain'}"
        out = run_bwd(c)
        check_bwd(tag, c, out)
        assert_same_bits(tag, out, run_bwd(c))                  # fixed-order column sums: bit-identical from run to run


@pytest.mark.parametrize("D", [64, 96])
def test_bwd_past_grid_cap(D):
    """32 801 rows: ln_bwd_grid caps at 1024 workgroups of 32 rows, so the first rows take a second trip.  The partial workspace has
    exactly ppf_layernorm_bwd_blocks(rows) * 4 * D floats: the kernel must fill what the reduce reads (NaN prefill) and write nothing past it."""
    from protopformer_amd import _lib
    rows = 32801
    g = torch.Generator().manual_seed(2000 + D)
    c = make_bwd(rows, D, g, ls=True)
    n = _lib.lib().ppf_layernorm_bwd_blocks(rows) * 4 * D
    guard = 4096
    part = torch.full((n + guard,), float("nan"), device="cuda")
    part[n:] = SENT
    sums = {k: v.clone().cuda() for k, v in c["init"].items()}
    dx = torch.empty(rows, D, device="cuda")
    cast = torch.empty(rows, D, dtype=torch.bfloat16, device="cuda")
    args = [c["dy"].cuda(), c["x"].cuda(), None, c["w"].cuda(), c["mean"].cuda(), c["rstd"].cuda(), c["dres"].cuda(), dx, sums["dw"], sums["db"], cast,
            c["rowscale"].cuda(), c["rpg"], c["colscale"].cuda(), sums["dbn"], c["branch"].cuda(), sums["dcs"], rows, D, part]
    with pytest.raises(RuntimeError):                                # one float short: refused on the host, nothing launched
        _lib.call("ppf_layernorm_bwd", *args, n * 4 - 4)
    _lib.call("ppf_layernorm_bwd", *args, n * 4)
    _lib.call("ppf_layernorm_bwd_reduce", part, rows, D, sums["dw"], sums["db"], sums["dbn"], sums["dcs"])
    torch.cuda.synchronize()
    assert torch.equal(bits(part[n:]), bits(torch.full((guard,), SENT))), "the kernel wrote past the partial workspace"
    out = {k: v.cpu() for k, v in sums.items()}
    out["dx"], out["cast"] = dx.cpu(), cast.cpu()
    check_bwd(f"ln_bwd D={D} rows={rows}", c, out)


@pytest.mark.parametrize("with_dres", [False, True], ids=["dres_none", "dres_by_source_row"])
@pytest.mark.parametrize("D", [192, 96])
def test_bwd_row_map(D, with_dres):
    """The final norm's scatter into the residual gradient: dy / mean / rstd by compact row; x / dres_in / dx_out / cast_out / branch
    and rowscale[src / rows_per_group] by source row.  Unmapped rows keep the sentinel bit for bit; the sums see mapped rows only."""
    g = torch.Generator().manual_seed(3000 + D + with_dres)
    rows, nsrc = 40, 120
    rm = torch.randperm(nsrc, generator=g)[:rows]                    # unordered, distinct
    c = make_bwd(rows, D, g, ls=True, nsrc=nsrc, row_map=rm, dres=with_dres, groups=(torch.tensor([0.5, 1.25, 2.0]), 40))
    assert len(set((rm // 40).tolist())) == 3 and set((torch.arange(rows) // 40).tolist()) == {0}     # source and compact groups differ
    out = run_bwd(c)
    tag = f"ln_bwd row_map D={D} {'dres' if with_dres else 'no dres'}"
    check_bwd(tag, c, out)
    rest = torch.ones(nsrc, dtype=torch.bool)
    rest[rm] = False
    assert torch.equal(bits(out["dx"][rest]), bits(torch.full((nsrc - rows, D), SENT))), f"{tag}: dx_out written at an unmapped row"
    assert torch.equal(bits(out["cast"][rest]), bits(torch.full((nsrc - rows, D), SENT, dtype=torch.bfloat16))), f"{tag}: cast_out written at an unmapped row"
    assert_same_bits(tag, out, run_bwd(c))


@pytest.mark.parametrize("D,ls", [(192, True), (384, False)])
def test_bwd_dy_none(D, ls):
    """The pure scale / cast / column-sum pass over dres_in: x, w, mean, rstd are NULL, dw / db keep their contents, dx_out is a copy."""
    g = torch.Generator().manual_seed(4000 + D)
    for rows in (1, 77):
        c = make_bwd(rows, D, g, ls=ls, dy=False)
        out = run_bwd(c)
        tag = f"ln_bwd dy=None D={D} rows={rows}"
        check_bwd(tag, c, out)
        assert torch.equal(bits(out["dx"]), bits(c["dres"])), f"{tag}: dx_out is not dres_in"
        assert_same_bits(tag, out, run_bwd(c))


@pytest.mark.parametrize("D", [128, 192, 96])
def test_bwd_in_place(D):
    """dx_out aliasing dres_in (every element is read and written by the same lane): bit-identical to the out-of-place call."""
    g = torch.Generator().manual_seed(5000 + D)
    c = make_bwd(77, D, g, ls=True)
    out = run_bwd(c)
    check_bwd(f"ln_bwd in place D={D}", c, out)
    assert_same_bits(f"ln_bwd in place D={D}", out, run_bwd(c, inplace=True))


@pytest.mark.parametrize("D", [128, 192, 96])
def test_bwd_atomics_path(D):
    """partial == NULL in the C ABI: one fp32 atomic per column per workgroup onto zeroed sums; any order, so no bit-identity."""
    g = torch.Generator().manual_seed(6000 + D)
    for rows in (1, 77, 200):
        c = make_bwd(rows, D, g, ls=True, zero_sums=True)
        check_bwd(f"ln_bwd atomics D={D} rows={rows}", c, run_bwd(c, atomics=True))


@pytest.mark.parametrize("D", [97, 600, 640, 800, 1026])
def test_refused_widths(D):
    """Odd D, ceil(D/128) in {5, 7} and D > 1024 are refused by the host-side argument checks of both entry points: RuntimeError, nothing
    launched, outputs untouched, and the next valid call works."""
    from protopformer_amd import _lib, ops
    g = torch.Generator().manual_seed(9)
    rows = 5
    x = torch.randn(rows, D, generator=g).cuda()
    w = torch.ones(D, device="cuda")
    b = torch.zeros(D, device="cuda")
    y = torch.full((rows, D), SENT, dtype=torch.bfloat16, device="cuda")
    mean, rstd = torch.full((rows,), SENT, device="cuda"), torch.full((rows,), SENT, device="cuda")
    with pytest.raises(RuntimeError):
        _lib.call("ppf_layernorm_fwd", x, None, w, b, y, mean, rstd, rows, D, EPS)
    dy = torch.randn(rows, D, generator=g).bfloat16().cuda()
    outs = [torch.full((rows, D), SENT, device="cuda"), torch.full((D,), SENT, device="cuda"), torch.full((D,), SENT, device="cuda"),
            torch.full((rows, D), SENT, dtype=torch.bfloat16, device="cuda"), torch.full((D,), SENT, device="cuda")]
    part = torch.full((_lib.lib().ppf_layernorm_bwd_blocks(rows) * 4 * D,), SENT, device="cuda")
    m0, r0 = torch.zeros(rows, device="cuda"), torch.ones(rows, device="cuda")
    for p, nbytes in ((part, part.numel() * 4), (None, 0)):
        with pytest.raises(RuntimeError):
            _lib.call("ppf_layernorm_bwd", dy, x, None, w, m0, r0, x, outs[0], outs[1], outs[2], outs[3], None, 1, None, outs[4], None, None, rows, D, p, nbytes)
    torch.cuda.synchronize()
    for t in [y, mean, rstd, part] + outs:
        assert torch.equal(bits(t), bits(torch.full(t.shape, SENT, dtype=t.dtype))), "a refused call wrote to an output"
    Dv = 96
    c = make_bwd(rows, Dv, g, ls=False)
    wv, bv = make_wb(Dv, g)
    check_fwd("ln_fwd after a refusal", ops.layernorm_fwd(c["x"].cuda(), wv.cuda(), bv.cuda()), fwd_ref(c["x"], wv, bv))
    check_bwd("ln_bwd after a refusal", c, run_bwd(c))
