"""CPU-side checks of integrated gradients: ppf_ig_point, ppf_ig_accumulate and ppf_ig_finish are declared, exported and bound with one
parameter list each and answer their limits through the error channel before any device call; interpret.ig_rule gives the three
quadratures; the numpy referees (interpret.ig_point / ig_accumulate / ig_finish with device=False) are complete on a function whose
path integral is known and sum the cells as a loop over their pixels does; the order constants and the two tools' parsers give known
answers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_ig_point": "ppfflps", "ppf_ig_accumulate": "pfiilpls", "ppf_ig_finish": "pppfiiiiiipps"}


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("name", sorted(SPECS))
def test_declared_exported_and_bound(lib, name):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/ppf_hip.h"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == len(SPECS[name]) and _lib.SIGS[name] == SPECS[name]
    assert lib.ppf_abi_version() == 10 == _lib.EXPECTED_ABI          # additions: no existing entry point changed


def _fn(lib, name):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn


D = 4096                                                              # an aligned non-null address, never dereferenced on a rejected shape


def _point(lib, n=8, x=D):
    return _fn(lib, "ppf_ig_point")(x, None, 0.0, 0.5, n, D, None)


def _accumulate(lib, first=0, R=2, n=8, stride=8, g=D):
    return _fn(lib, "ppf_ig_accumulate")(g, 0.5, first, R, n, D, stride, None)


def _finish(lib, B=2, M=1, C=3, H=32, W=32, patch=16, acc=D):
    return _fn(lib, "ppf_ig_finish")(acc, D, None, 0.0, B, M, C, H, W, patch, D, D, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_point, dict(n=0), -1, "n=0"), (_point, dict(x=None), -3, "null pointer"),
    (_accumulate, dict(R=0), -1, "R=0"), (_accumulate, dict(n=0), -1, "n=0"), (_accumulate, dict(n=8, stride=7), -1, "acc_stride=7"),
    (_accumulate, dict(first=2), -3, "first=2"), (_accumulate, dict(g=None), -3, "null pointer"),
    (_finish, dict(M=9), -1, "M=9"), (_finish, dict(M=0), -1, "M=0"), (_finish, dict(H=40), -1, "patch=16 does not divide H=40"),
    (_finish, dict(W=24), -1, "W=24"), (_finish, dict(patch=0), -1, "patch=0"), (_finish, dict(H=132, W=132, patch=4), -1, "G=1089"),
    (_finish, dict(B=0), -1, "B=0"), (_finish, dict(acc=None), -3, "null pointer")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_ig_"), msg


# ------------------------------------------------------------------------------------------------ the quadrature
@pytest.mark.parametrize("S", [1, 2, 7])
def test_ig_rule_gives_the_three_quadratures(S):
    from protopformer_amd.interpret import ig_rule
    s = np.arange(S, dtype=np.float64)
    want = {"midpoint": ((s + 0.5) / S, np.full(S, 1.0 / S)), "endpoint": ((s + 1.0) / S, np.full(S, 1.0 / S)),
            "trapezoid": (np.arange(S + 1, dtype=np.float64) / S, np.array([0.5 / S] + [1.0 / S] * (S - 1) + [0.5 / S]))}
    for rule, (a64, w64) in want.items():
        a, w = ig_rule(S, rule)
        assert a.dtype == w.dtype == np.float32 and a.shape == w.shape == a64.shape
        assert np.array_equal(a, a64.astype(np.float32)) and np.array_equal(w, w64.astype(np.float32)), rule      # fp64, cast once
        assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23 * w.size, rule
        assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] <= 1
    assert np.array_equal(ig_rule(S)[0], ig_rule(S, "midpoint")[0])                                              # the default
    a, w = ig_rule(1, "endpoint")
    assert a.tolist() == [1.0] and w.tolist() == [1.0]                                                           # gradient x (x - baseline)


def test_ig_rule_refuses_bad_names_and_step_counts():
    from protopformer_amd.interpret import ig_rule
    for bad in ("simpson", "", None, "Midpoint"):
        with pytest.raises(ValueError, match="rule must be one of"):
            ig_rule(4, bad)
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="steps"):
            ig_rule(bad, "midpoint")


# ------------------------------------------------------------------------------------------------ the referees are complete where the integral is known
def _referee_ig(x, base, c, S, rule):
    """Integrated gradients of f(x) = sum c x^2 by the referees: gradient 2 c p at the path point p.  Returns (attr [1, 1, C, H, W],
    cell64, sum |w g (x - base)| in fp64)."""
    from protopformer_amd.interpret import ig_accumulate, ig_finish, ig_point, ig_rule
    alphas, weights = ig_rule(S, rule)
    acc, mass = None, 0.0
    b = np.broadcast_to(np.asarray(base, dtype=np.float32), x.shape)
    for s, (a, w) in enumerate(zip(alphas, weights)):
        p = ig_point(x, a, base, device=False)
        g = (np.float32(2) * c * p).astype(np.float32)
        acc = ig_accumulate(g, w, acc, first=s == 0, device=False)
        mass += float(np.abs(np.float64(w) * g.astype(np.float64) * (x.astype(np.float64) - b)).sum())
    attr, cell64 = ig_finish(acc[:, None], x, base, 4, device=False)
    return attr, cell64, mass


@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("rule", ["midpoint", "trapezoid"])
@pytest.mark.parametrize("tensor_baseline", [False, True], ids=["constant", "tensor"])
def test_referee_completeness_on_a_quadratic(S, rule, tensor_baseline):
    """Both rules integrate the linear gradient of f(x) = sum c x^2 exactly, so sum attr = f(x) - f(base) up to rounding.  The allowed
    error is (S + 4) * 2^-24 * sum |w g (x - base)|: the S roundings of the weighted sum and the few of the point, the gradient, the
    difference and the final product, each half an ulp of a term of that sum."""
    rng = np.random.default_rng(S + len(rule))
    x = rng.standard_normal((1, 3, 8, 12)).astype(np.float32)
    c = rng.uniform(0.5, 2.0, x.shape).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else -0.375
    attr, cell64, mass = _referee_ig(x, base, c, S, rule)
    b64 = np.broadcast_to(np.asarray(base, dtype=np.float32), x.shape).astype(np.float64)
    want = float((c.astype(np.float64) * (x.astype(np.float64) ** 2 - b64 ** 2)).sum())
    got = float(attr.astype(np.float64).sum())
    bound = (S + 4) * 2.0 ** -24 * mass
    print(f"{rule} S={S}: sum attr - (f(x) - f(base)) = {got - want:.3e}, bound {bound:.3e}")
    assert abs(got - want) <= bound
    assert abs(float(cell64.sum()) - got) <= 2.0 ** -52 * float(np.abs(attr).astype(np.float64).sum()) * attr.size       # the cells partition the image


def test_referee_endpoint_rule_with_one_step_is_gradient_times_input_bit_for_bit():
    from protopformer_amd.interpret import ig_point
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 3, 8, 12)).astype(np.float32)
    c = rng.uniform(0.5, 2.0, x.shape).astype(np.float32)
    attr, _, _ = _referee_ig(x, 0.0, c, 1, "endpoint")                                             # baseline 0: the end point is x itself
    assert np.array_equal(attr[:, 0].view(np.int32), (x * (np.float32(2) * c * x)).astype(np.float32).view(np.int32))
    for base in (-0.375, rng.standard_normal(x.shape).astype(np.float32)):                         # else: the gradient at the path's end point
        attr, _, _ = _referee_ig(x, base, c, 1, "endpoint")
        end = ig_point(x, 1.0, base, device=False)
        assert np.abs(end - x).max() <= 2.0 ** -22 * max(1.0, float(np.abs(x).max()))
        want = ((x - np.asarray(base, dtype=np.float32)) * (np.float32(2) * c * end)).astype(np.float32)
        assert np.array_equal(attr[:, 0].view(np.int32), want.view(np.int32))


def test_referee_point_and_accumulate_identities():
    from protopformer_amd.interpret import ig_accumulate, ig_point
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 3, 4, 4)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32)
    assert np.array_equal(ig_point(x, 0.0, base, device=False), base) and np.array_equal(ig_point(x, 0.0, 0.25, device=False), np.full_like(x, 0.25))
    assert np.array_equal(ig_point(x, 1.0, 0.0, device=False), x)
    third = ig_point(x, 1 / 3, base, device=False)
    assert third.dtype == np.float32 and np.array_equal(third, base + np.float32(1 / 3) * (x - base))
    first = ig_accumulate(x, 0.5, None, first=True, device=False)
    assert np.array_equal(first, np.float32(0.5) * x)
    x[1, 2, 3, 1] = np.nan
    nxt = ig_accumulate(x, 0.25, first, device=False)
    assert np.isnan(nxt[1, 2, 3, 1]) and np.isnan(nxt).sum() == 1 and np.array_equal(nxt[0], first[0] + np.float32(0.25) * x[0])


# ------------------------------------------------------------------------------------------------ the cell sums
@pytest.mark.parametrize("B,M,C,H,W,patch", [(2, 2, 3, 8, 8, 4), (1, 1, 3, 16, 16, 16), (2, 3, 1, 12, 18, 6)], ids=["2x2_grid", "one_cell", "non_square"])
def test_finish_referee_sums_each_cell_as_a_loop_over_its_pixels(B, M, C, H, W, patch):
    from protopformer_amd.interpret import ig_finish
    rng = np.random.default_rng(H + W)
    acc = rng.standard_normal((B, M, C, H, W)).astype(np.float32)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32)
    gh, gw = H // patch, W // patch
    for bl in (0.5, base):
        attr, cell64 = ig_finish(acc, x, bl, patch, device=False)
        assert attr.dtype == np.float32 and attr.shape == acc.shape and cell64.dtype == np.float64 and cell64.shape == (B, M, gh * gw)
        bb = np.broadcast_to(np.asarray(bl, dtype=np.float32), x.shape)
        assert np.array_equal(attr, (x - bb)[:, None] * acc)
        for b in range(B):
            for m in range(M):
                for g in range(gh * gw):
                    gy, gx = divmod(g, gw)
                    tot, mass = 0.0, 0.0
                    for c in range(C):
                        for py in range(patch):
                            for px in range(patch):
                                v = float(attr[b, m, c, gy * patch + py, gx * patch + px])
                                tot += v
                                mass += abs(v)
                    assert abs(cell64[b, m, g] - tot) <= C * patch * patch * 2.0 ** -53 * mass, (b, m, g)
    acc[0, 0, 0, 1, 1] = np.nan                                                                 # a NaN marks its own cell only
    _, cell64 = ig_finish(acc, x, 0.5, patch, device=False)
    assert np.isnan(cell64[0, 0, 0]) and np.isnan(cell64).sum() == 1
    for bad in (dict(patch=5), dict(patch=0)):
        with pytest.raises(ValueError, match="ig_finish"):
            ig_finish(acc, x, 0.5, bad["patch"], device=False)
    with pytest.raises(ValueError, match="ig_finish"):
        ig_finish(np.zeros((1, 9, 1, 4, 4), dtype=np.float32), np.zeros((1, 1, 4, 4), dtype=np.float32), 0.0, 4, device=False)


# ------------------------------------------------------------------------------------------------ constants, the result record, parsers
def test_order_constants():
    from protopformer_amd.interpret import EXTRA_ORDERS, GRADIENT_ORDERS, IG_DEFAULTS, ORDER_MODES
    assert ORDER_MODES == ("evidence", "attention", "random") and EXTRA_ORDERS == ("rise",) and GRADIENT_ORDERS == ("ig",)
    assert IG_DEFAULTS == dict(steps=32, rule="midpoint")


def test_result_record_on_the_host_and_the_cpu_refusal():
    import torch
    from protopformer_amd.interpret import IntegratedGradients, integrated_gradients
    assert IntegratedGradients.FIELDS == ("attribution", "cell", "total", "value", "value_base", "targets", "alphas", "weights")
    total = np.array([[1.5, -2.0]])
    r = IntegratedGradients(np.zeros((1, 2, 3, 4, 4), np.float32), np.zeros((1, 2, 1), np.float32), total, np.array([[3.0, 1.0]], np.float32),
                            np.array([[1.0, 2.5]], np.float32), np.array([[4, 7]], np.int32), np.array([0.5], np.float32), np.array([1.0], np.float32),
                            ("logit",), 1, "midpoint")
    assert r.on_host and r.cpu() is r and r.delta().dtype == np.float64 and r.delta().tolist() == [[-0.5, -0.5]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        integrated_gradients(None, torch.zeros(1, 3, 8, 8))


def test_faithfulness_parser_takes_the_ig_order():
    from protopformer_amd.faithfulness import get_args_parser
    a = get_args_parser().parse_args([])
    assert (a.orders, a.ig_steps, a.ig_rule, a.rise_masks, a.steps) == (["evidence", "attention", "random"], 32, "midpoint", 512, 14)      # defaults unchanged
    a = get_args_parser().parse_args(["--orders", "evidence", "ig", "--ig_steps", "4"])
    assert (a.orders, a.ig_steps, a.ig_rule) == (["evidence", "ig"], 4, "midpoint")
    assert get_args_parser().parse_args(["--ig_rule", "trapezoid"]).ig_rule == "trapezoid"
    for bad in (["--orders", "smoothgrad"], ["--ig_rule", "simpson"]):
        with pytest.raises(SystemExit):
            get_args_parser().parse_args(bad)


def test_attribute_parser_shares_the_model_and_data_flags_of_train():
    from protopformer_amd.attribute import get_args_parser
    from protopformer_amd.train import get_args_parser as train_parser
    own = {o: a for a in get_args_parser()._actions for o in a.option_strings}
    shared = [(o, a) for a in train_parser()._actions for o in a.option_strings]
    assert len(shared) > 40
    for o, a in shared:
        assert o in own and own[o].dest == a.dest, f"{o} of train.py is missing"
        assert own[o].default == (0 if a.dest == "seed" else a.default), o               # the tool's own default seed is 0
    a = get_args_parser().parse_args([])
    assert (a.resume, a.split, a.steps, a.rule, a.top_classes, a.against_label, a.max_images, a.save_maps) == ("", "test", 32, "midpoint", 1, False, 0, False)
    a = get_args_parser().parse_args(["--resume", "x.pth", "--split", "train", "--steps", "8", "--rule", "endpoint", "--top_classes", "3", "--against_label",
                                      "--max_images", "5", "--save-maps", "--output_dir", "o"])
    assert (a.resume, a.split, a.steps, a.rule, a.top_classes, a.against_label, a.max_images, a.save_maps, a.output_dir) == (
        "x.pth", "train", 8, "endpoint", 3, True, 5, True, "o")


def test_attribute_records_rank_the_cells_and_state_the_gap():
    from protopformer_amd.attribute import records, relative_gaps
    from protopformer_amd.interpret import IntegratedGradients
    cell = np.zeros((1, 1, 16), np.float32)
    cell[0, 0, [5, 9, 2]] = [3.0, 3.0, 7.0]
    cell[0, 0, 11] = np.nan
    h = IntegratedGradients(np.zeros((0, 1, 3, 8, 8), np.float32), cell, np.array([[13.5]]), np.array([[10.0]], np.float32), np.array([[-2.0]], np.float32),
                            np.array([[42]], np.int32), np.array([0.5], np.float32), np.array([1.0], np.float32), ("logit",), 1, "midpoint")
    (rec,) = records(h, [77], 4, 2, top_cells=4)
    col = rec["classes"][0]
    assert rec["image_id"] == 77 and (col["target"], col["value"], col["value_base"], col["total"], col["delta"]) == (42, 10.0, -2.0, 13.5, 1.5)
    assert [c["cell"] for c in col["cells"]] == [2, 5, 9, 0]                                     # score descending, ties to the smaller cell, NaN last
    assert col["cells"][1]["box"] == [2, 2, 4, 4] and col["cells"][0]["score"] == 7.0
    assert relative_gaps([rec]).tolist() == [0.125]
