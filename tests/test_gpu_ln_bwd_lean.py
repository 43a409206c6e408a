"""The register-lean form of ln_bwd2_kernel at D = 384 (csrc/layernorm.hip, test hook ppf_layernorm_test_bwd_path) against the parent form,
bit for bit, and against the fp64 reference of tests/test_gpu_layernorm_paths.py with that file's operands, bounds and checks (imported,
not restated).  Only where values live differs between the forms -- weights in LDS, dy kept packed, xhat and dx written over their inputs --
so dx_out, cast_out and the reduced column sums are equal on the deterministic `partial` path.

Row counts: 1 (the second half-wave has no row), 2, 7 (ends on a half-wave pair with one row), 263 (more than one workgroup, a ragged last
one) and 32 808 (past the 1024-workgroup grid cap: waves make a second trip).  Operand combinations at 263 rows: no dres_in, dx_out aliasing
dres_in, no cast_out (the call of block 0), dy = None (the scale / cast pass), a scattered row_map, rowscale in groups of 197 and of 82 rows.
The atomics path (partial = NULL) adds in any order, so there the lean form is held to fp64 only."""
import pytest
import torch

from helpers import SENT, bits, maxu, report
from test_gpu_layernorm_paths import K, bwd_ref, check_bwd, colsum_gate, make_bwd

pytestmark = pytest.mark.gpu

D = 384
PARENT, LEAN = 1, 2


def _run(c, path, *, atomics=False, inplace=False, cast=True):
    """One ppf_layernorm_bwd call (and its reduce) with the hook at `path`; the outputs on the CPU.  test_gpu_layernorm_paths.run_bwd with
    the hook around it and an optional cast_out."""
    from protopformer_amd import _lib, ops
    dev = lambda t: None if t is None else t.cuda()
    nsrc = c["nsrc"]
    sums = {k: v.clone().cuda() for k, v in c["init"].items()}
    dres = dev(c["dres"])
    dx = dres if inplace else torch.full((nsrc, D), SENT, device="cuda")
    cast_out = torch.full((nsrc, D), SENT, dtype=torch.bfloat16, device="cuda") if cast else None
    have_dy = c["dy"] is not None
    rm = None if c["row_map"] is None else c["row_map"].to(torch.int32).cuda()
    dy, x, w, mean, rstd = dev(c["dy"]), *(dev(c[k]) if have_dy else None for k in ("x", "w", "mean", "rstd"))
    rowscale, dbn = dev(c["rowscale"]), sums["dbn"] if cast else None
    try:
        _lib.call("ppf_layernorm_test_bwd_path", path)
        if atomics:                                                   # partial == NULL, size 0: only the C ABI reaches it
            _lib.call("ppf_layernorm_bwd", dy, x, rm, w, mean, rstd, dres, dx, sums["dw"], sums["db"], cast_out, rowscale, c["rpg"],
                      None, dbn, None, None, c["rows"], D, None, 0)
        else:
            ops.layernorm_bwd(dy, x, w, mean, rstd, sums["dw"], sums["db"], row_map=rm, dres_in=dres, dx_out=dx, cast_out=cast_out,
                              rowscale=rowscale, rows_per_group=c["rpg"], dbias_next=dbn)
        torch.cuda.synchronize()
    finally:
        _lib.call("ppf_layernorm_test_bwd_path", 0)
    out = {k: v.cpu() for k, v in sums.items()}
    out["dx"] = dx.cpu()
    if cast:
        out["cast"] = cast_out.cpu()
    return out


def _both(tag, c, **kw):
    """The parent form, then the lean form, in this process: equal bits everywhere, and the lean form within the fp64 gates."""
    parent, lean = _run(c, PARENT, **kw), _run(c, LEAN, **kw)
    for k in parent:
        assert torch.equal(bits(lean[k]), bits(parent[k])), f"{tag}: {k} differs between the lean and the parent form at {int((bits(lean[k]) != bits(parent[k])).sum())} places"
    return lean


CASES = {"dres_none": dict(dres=False),"rowscale_197": dict(groups=(torch.tensor([0.5, 1.25]), 197)),
         "rowscale_82": dict(groups=(torch.tensor([0.5, 0.0, 1.0 / 0.9, 2.0]), 82))}


@pytest.mark.parametrize("rows", [1, 2, 7, 263, 32808])
def test_lean_every_row_count(rows):
    g = torch.Generator().manual_seed(7000 + rows)
    c = make_bwd(rows, D, g, ls=False)
    tag = f"ln_bwd lean rows={rows}"
    check_bwd(tag, c, _both(tag, c))


@pytest.mark.parametrize("case", ["dres_none", "rowscale_197", "rowscale_82"])
def test_lean_operands(case):
    g = torch.Generator().manual_seed(7100 + len(case))
    c = make_bwd(263, D, g, ls=False, **CASES[case])
    tag = f"ln_bwd lean {case}"
    check_bwd(tag, c, _both(tag, c))


def test_lean_in_place():
    """dx_out aliasing dres_in: the same bits as the out-of-place call, in both forms."""
    g = torch.Generator().manual_seed(7200)
    c = make_bwd(263, D, g, ls=False)
    out = _both("ln_bwd lean out of place", c)
    check_bwd("ln_bwd lean in place", c, out)
    inplace = _both("ln_bwd lean in place", c, inplace=True)
    for k in out:
        assert torch.equal(bits(inplace[k]), bits(out[k])), f"in place: {k} differs from the out-of-place call"


def test_lean_no_cast_out():
    """The call of block 0: no cast_out, no dbias_next.  dx, dw and db under the gates of check_bwd; dbias_next keeps its contents."""
    g = torch.Generator().manual_seed(7300)
    c = make_bwd(263, D, g, ls=False)
    tag = "ln_bwd lean no cast_out"
    out = _both(tag, c, cast=False)
    r = bwd_ref(c)
    dx_u = maxu((out["dx"].double() - r["dx"]).abs(), r["s_dx"])
    assert dx_u <= K, f"{tag}: dx off by {dx_u:.2f} u (gate {K})"
    report(tag, dx_u=dx_u, dw_frac=colsum_gate(tag, "dw", out["dw"], c["init"]["dw"], r["tw"]),
           db_frac=colsum_gate(tag, "db", out["db"], c["init"]["db"], r["tb"]))
    assert torch.equal(bits(out["dbn"]), bits(c["init"]["dbn"])), f"{tag}: dbias_next touched"


def test_lean_dy_none():
    """The pure scale / cast / column-sum pass over dres_in: dw / db keep their contents (check_bwd), dx_out is a copy."""
    g = torch.Generator().manual_seed(7400)
    for rows in (1, 263):
        c = make_bwd(rows, D, g, ls=False, dy=False)
        tag = f"ln_bwd lean dy=None rows={rows}"
        out = _both(tag, c)
        check_bwd(tag, c, out)
        assert torch.equal(bits(out["dx"]), bits(c["dres"])), f"{tag}: dx_out is not dres_in"


@pytest.mark.parametrize("with_dres", [False, True], ids=["dres_none", "dres_by_source_row"])
def test_lean_row_map(with_dres):
    """The final norm: dy / mean / rstd by compact row, everything else and rowscale[src / 197] by a scattered source row; unmapped rows
    keep the sentinel."""
    g = torch.Generator().manual_seed(7500 + with_dres)
    rows, nsrc = 263, 788
    rm = torch.randperm(nsrc, generator=g)[:rows]
    c = make_bwd(rows, D, g, ls=False, nsrc=nsrc, row_map=rm, dres=with_dres, groups=(torch.tensor([0.5, 1.25, 2.0, 0.75]), 197))
    assert len(set((rm // 197).tolist())) == 4
    tag = f"ln_bwd lean row_map {'dres' if with_dres else 'no dres'}"
    out = _both(tag, c)
    check_bwd(tag, c, out)
    rest = torch.ones(nsrc, dtype=torch.bool)
    rest[rm] = False
    assert torch.equal(bits(out["dx"][rest]), bits(torch.full((nsrc - rows, D), SENT))), f"{tag}: dx_out written at an unmapped row"
    assert torch.equal(bits(out["cast"][rest]), bits(torch.full((nsrc - rows, D), SENT, dtype=torch.bfloat16))), f"{tag}: cast_out written at an unmapped row"


def test_lean_atomics_path():
    """partial == NULL: one fp32 atomic per column per workgroup onto zeroed sums, in any order: the lean form against fp64 only."""
    g = torch.Generator().manual_seed(7600)
    for rows in (1, 7, 263):
        c = make_bwd(rows, D, g, ls=False, zero_sums=True)
        check_bwd(f"ln_bwd lean atomics rows={rows}", c, _run(c, LEAN, atomics=True))


def test_bwd_path_hook_rejects_other_values():
    from protopformer_amd import _lib
    try:
        with pytest.raises(RuntimeError, match="ppf_layernorm_test_bwd_path"):
            _lib.call("ppf_layernorm_test_bwd_path", 3)
    finally:
        _lib.call("ppf_layernorm_test_bwd_path", 0)
