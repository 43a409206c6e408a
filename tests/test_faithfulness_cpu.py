"""CPU-side checks of the faithfulness pass: ppf_cell_order, ppf_patch_perturb and ppf_class_prob are declared, exported and bound with
one parameter list each and answer their limits through the error channel before any device call; the numpy Philox reproduces the
published Random123 known answers; the numpy referees (interpret.cell_order_from_outputs / perturb_patches with device=False) keep the
contract's order and the deletion / insertion identities; the default counts, the area under a curve and the tool's parser give known
answers."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_cell_order": "ppppfppLiiiiiiippps", "ppf_patch_perturb": "pppiipfiiiiiips", "ppf_class_prob": "ppiips"}
MODES = ("evidence", "attention", "random")


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


def _order(lib, mode=0, B=2, P=20, C=10, T=9, G=16, M=1):
    return _fn(lib, "ppf_cell_order")(D, D, D, D, 0.5, D, D, 0, mode, B, P, C, T, G, M, D, D, D, None)


def _perturb(lib, S=4, insertion=0, B=2, M=1, Cc=3, H=64, W=64, G=16, x=D):
    return _fn(lib, "ppf_patch_perturb")(x, D, D, S, insertion, None, 0.0, B, M, Cc, H, W, G, D, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_order, dict(G=1025), -1, "G=1025"), (_order, dict(G=0), -1, "G=0"), (_order, dict(T=17), -1, "T=17"), (_order, dict(T=0), -1, "T=0"),
    (_order, dict(M=9), -1, "M=9"), (_order, dict(M=0), -1, "M=0"), (_order, dict(B=0), -1, "B=0"), (_order, dict(P=0), -1, "P=0"),
    (_order, dict(mode=3), -3, "mode=3"),
    (_perturb, dict(H=32, W=32, G=256), -1, "patch width 2"), (_perturb, dict(G=15), -1, "G=15"), (_perturb, dict(H=64, W=48), -1, "W=48"),
    (_perturb, dict(H=60, W=60), -1, "H=60"), (_perturb, dict(M=9), -1, "M=9"), (_perturb, dict(S=0), -1, "S=0"),
    (_perturb, dict(G=1600, H=160, W=160), -1, "G=1600"),
    (_perturb, dict(insertion=2), -3, "insertion=2"), (_perturb, dict(x=D + 4), -2, "16-byte")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_"), msg


def test_class_prob_limits(lib):
    fn = _fn(lib, "ppf_class_prob")
    assert fn(D, D, 0, 10, D, None) == -1 and "R=0" in lib.ppf_last_error().decode()
    assert fn(D, D, 4, 0, D, None) == -1 and "C=0" in lib.ppf_last_error().decode()
    assert fn(D, None, 4, 10, D, None) == -3


# ------------------------------------------------------------------------------------------------ the numpy Philox
def test_numpy_philox_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds."""
    from protopformer_amd.interpret import philox4x32_10
    kat = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert got.dtype == np.uint32 and " ".join(f"{v:08x}" for v in got) == want
    both = philox4x32_10(np.array([k[0] for k in kat[:2]], dtype=np.uint64), np.array([k[1] for k in kat[:2]], dtype=np.uint64))     # vectorised
    assert [" ".join(f"{v:08x}" for v in row) for row in both] == [kat[0][2], kat[1][2]]


# ------------------------------------------------------------------------------------------------ the order referee
def _case(B=2, P=12, C=4, T=5, G=16, M=3, seed=0):
    rng = np.random.default_rng(seed)
    return dict(act_full=(rng.integers(0, 64, (B, P, T)) / 8).astype(np.float32), idx=np.stack([np.sort(rng.permutation(G)[:T]) for _ in range(B)]).astype(np.int32),
                token_attn=(rng.integers(0, 8, (B, G)) / 64).astype(np.float32), weight=(rng.integers(-4, 5, (C, P)) / 4).astype(np.float32), scale=0.5,
                classes=rng.integers(0, C, (B, M)).astype(np.int32), grid_cells=G)


def _referee(c, mode, **kw):
    from protopformer_amd.interpret import cell_order_from_outputs
    return cell_order_from_outputs(device=False, mode=mode, **{**c, **kw})


def sorted_by_contract(score, tier):
    """The order the contract states, written out as a comparison sort (not lexsort): tier ascending, NaN last, score descending, cell."""
    import functools

    def cmp(i, j):
        a, b = (tier[i], np.isnan(score[i])), (tier[j], np.isnan(score[j]))
        if a != b:
            return -1 if a < b else 1
        if not a[1] and score[i] != score[j]:
            return -1 if score[i] > score[j] else 1
        return -1 if i < j else 1
    return sorted(range(len(score)), key=functools.cmp_to_key(cmp))


@pytest.mark.parametrize("mode", MODES)
def test_referee_rank_inverts_order_and_ties_go_to_the_smaller_cell(mode):
    c = _case()
    order, rank, score = _referee(c, mode, seed=3, image_ids=np.array([11, 5]))
    B, M, G = order.shape
    assert order.dtype == rank.dtype == np.int32 and score.dtype == np.float32
    for b in range(B):
        for m in range(M):
            assert sorted(order[b, m].tolist()) == list(range(G)) and (rank[b, m, order[b, m]] == np.arange(G)).all()
            tier = np.ones(G, dtype=int)
            tier[c["idx"][b]] = 0
            if mode != "evidence":
                tier[:] = 0
            assert order[b, m].tolist() == sorted_by_contract(score[b, m], tier)
            if mode == "evidence":
                T = c["idx"].shape[1]
                assert set(order[b, m, :T].tolist()) == set(c["idx"][b].tolist())                  # tier 0 precedes tier 1
                w = np.float32(c["scale"]) * c["weight"][c["classes"][b, m]]
                want = (w.astype(np.float64)[:, None] * c["act_full"][b].astype(np.float64)).sum(0)
                assert np.array_equal(score[b, m, c["idx"][b]], want.astype(np.float32))
                rest = np.setdiff1d(np.arange(G), c["idx"][b])
                assert np.array_equal(score[b, m, rest], c["token_attn"][b, rest])
            elif mode == "attention":
                assert np.array_equal(score[b, m], c["token_attn"][b])
            else:
                assert ((score[b, m] >= 0) & (score[b, m] < 1)).all() and len(set(score[b, m].tolist())) > G // 2
    if mode == "attention":
        assert (np.diff(score[0, 0, order[0, 0]]) <= 0).all() and (score[0, 0, order[0, 0]][:-1] == score[0, 0, order[0, 0]][1:]).any()   # ties exist


@pytest.mark.parametrize("mode", MODES)
def test_referee_all_equal_nan_and_invalid_classes(mode):
    c = _case()
    c["act_full"][:] = 1.0
    c["weight"][:] = 1.0
    c["token_attn"][:] = 0.25
    c["classes"][1] = (-1, 4, 2)
    order, rank, score = _referee(c, mode)
    assert (order[1, :2] == -1).all() and (rank[1, :2] == -1).all() and (score[1, :2] == 0).all() and (order[1, 2] >= 0).all()
    if mode == "attention":
        assert (order[0] == np.arange(16)).all()                                                   # all equal: ascending cells
    if mode == "evidence":
        res = c["idx"][0].tolist()
        assert order[0, 0].tolist() == res + [g for g in range(16) if g not in res]
    if mode == "random":
        return
    # NaN comes last in its tier, below -inf; +inf first
    c["token_attn"][0, :4] = (np.nan, -np.inf, np.inf, np.nan)
    c["act_full"][0, :, 0], c["act_full"][0, :, 1] = np.nan, -np.inf
    order, rank, score = _referee(c, mode)
    if mode == "attention":
        assert order[0, 0].tolist() == [2] + list(range(4, 16)) + [1, 0, 3]
    else:
        res = c["idx"][0].tolist()
        assert order[0, 0, :5].tolist() == res[2:] + [res[1], res[0]] and np.isnan(score[0, 0, res[0]]) and score[0, 0, res[1]] == -np.inf
        unres = [g for g in range(16) if g not in res]
        tail = order[0, 0, 5:].tolist()
        nans = [g for g in unres if np.isnan(c["token_attn"][0, g])]
        assert sorted(tail) == unres and tail[len(tail) - len(nans):] == nans


def test_referee_idx_outside_the_grid_and_repeated_cells():
    c = _case(T=5)
    c["idx"][0] = (3, 99, 3, -1, 7)                                                                 # cell 3 twice, two entries off the grid
    order, rank, score = _referee(c, "evidence")
    w = np.float32(0.5) * c["weight"][c["classes"][0, 0]]
    tot = (w.astype(np.float64)[:, None] * c["act_full"][0].astype(np.float64)).sum(0).astype(np.float32)
    assert score[0, 0, 3] == tot[0] and score[0, 0, 7] == tot[4]                                    # the smallest t wins
    assert set(order[0, 0, :2].tolist()) == {3, 7} and np.array_equal(np.delete(score[0, 0], [3, 7]), np.delete(c["token_attn"][0], [3, 7]))


def test_referee_random_order_is_keyed_by_image_id_alone():
    c = _case(B=2, M=1)
    a = _referee(c, "random", seed=9, image_ids=np.array([40, 41]))
    c2 = {**c, "classes": c["classes"][::-1].copy()}
    b = _referee(c2, "random", seed=9, image_ids=np.array([41, 40]))
    assert np.array_equal(a[0][0], b[0][1]) and np.array_equal(a[2][1], b[2][0])
    assert not np.array_equal(a[0][0], _referee(c, "random", seed=10, image_ids=np.array([40, 41]))[0][0])
    from protopformer_amd.interpret import philox4x32_10
    word = philox4x32_10(np.array([5, 0, 40, 0], dtype=np.uint64), np.array([9, 0], dtype=np.uint64))[0]
    assert a[2][0, 0, 5] == np.float32((int(word) >> 8) * 2.0 ** -24)


# ------------------------------------------------------------------------------------------------ counts, area, the perturbation referee
def test_default_counts():
    from protopformer_amd.interpret import default_counts
    assert default_counts(196).tolist() == list(range(0, 197, 14))
    for G in (1, 4, 9, 16, 64, 196, 576, 1024):
        for steps in (1, 14, 20):
            c = default_counts(G, steps)
            assert c.dtype == np.int32 and c[0] == 0 and c[-1] == G and (np.diff(c) > 0).all() and len(c) <= steps + 1
    assert default_counts(4).tolist() == [0, 1, 2, 3, 4]


def test_curve_auc_is_the_trapezoid_over_the_fraction():
    from protopformer_amd.interpret import Faithfulness, curve_auc
    assert curve_auc([1.0, 0.5, 0.0], [0, 8, 16], 16) == 0.5 and curve_auc([[1.0, 1.0], [0.0, 1.0]], [0, 4], 4).tolist() == [1.0, 0.5]
    f = Faithfulness({"deletion": np.array([[[1.0, 0.0, 0.0]]], dtype=np.float32)}, np.array([0, 4, 16], dtype=np.int32), np.zeros((1, 1), dtype=np.int32),
                     None, None, None, 16)
    assert f.cpu() is f and f.auc()["deletion"].tolist() == [[0.125]]


@pytest.mark.parametrize("size,G", [(64, 16), (32, 64), (24, 9)])
@pytest.mark.parametrize("tensor_baseline", [False, True])
def test_perturb_referee_identities(size, G, tensor_baseline):
    from protopformer_amd.interpret import perturb_patches
    rng = np.random.default_rng(G)
    B, M, side = 2, 2, int(G ** 0.5)
    x = rng.standard_normal((B, 3, size, size)).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32) if tensor_baseline else 0.25
    full = np.broadcast_to(np.float32(base), x.shape)
    rank = np.stack([np.stack([rng.permutation(G) for _ in range(M)]) for _ in range(B)]).astype(np.int32)
    rank[1, 1] = -1
    counts = [0, 1, 5, G]
    dele = perturb_patches(x, rank, counts, insertion=False, baseline=base, device=False)
    ins = perturb_patches(x, rank, counts, insertion=True, baseline=base, device=False)
    assert dele.shape == ins.shape == (4, B, M, 3, size, size) and dele.dtype == np.float32
    xm, bm = x[:, None].repeat(M, 1), full[:, None].repeat(M, 1)
    valid = (rank[:, :, 0] >= 0)
    assert np.array_equal(dele[0], xm) and np.array_equal(ins[3], xm)
    assert np.array_equal(dele[3][valid], bm[valid]) and np.array_equal(ins[0][valid], bm[valid])
    assert np.array_equal(dele[:, 1, 1], np.broadcast_to(x[1], dele[:, 1, 1].shape)) and np.array_equal(ins[:, 1, 1], dele[:, 1, 1])     # the -1 row copies x
    # at every count the two modes partition the pixels: where one shows x the other shows the baseline
    from_x_d, from_x_i = dele == xm[None], ins == xm[None]
    differs = (xm != bm)[None] & valid[None, :, :, None, None, None]
    assert ((from_x_d ^ from_x_i) | ~differs).all() and (np.where(from_x_d, ins, dele)[:, valid] == bm[None][:, valid]).all()
    # count 1 removes exactly the rank-0 cell
    p = size // side
    g0 = int(np.nonzero(rank[0, 0] == 0)[0][0])
    ys, xs = g0 // side * p, g0 % side * p
    want = x[0].copy()
    want[:, ys:ys + p, xs:xs + p] = full[0][:, ys:ys + p, xs:xs + p]
    assert np.array_equal(dele[1, 0, 0], want)


def test_perturb_referee_refuses_what_the_kernel_refuses():
    from protopformer_amd.interpret import perturb_patches
    with pytest.raises(ValueError, match="patch width"):
        perturb_patches(np.zeros((1, 3, 32, 32), dtype=np.float32), np.zeros((1, 1, 256), dtype=np.int32), [0, 1], device=False)


def test_counts_are_range_checked_on_the_host():
    from protopformer_amd.interpret import _device_counts
    assert _device_counts(None, 16, "cpu").tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16]
    for bad in ([0, 17], [3, 2], [0, 0, 4], [5], [-1, 4]):
        with pytest.raises(ValueError, match="strictly increasing"):
            _device_counts(bad, 16, "cpu")


# ------------------------------------------------------------------------------------------------ the tool's parser
def test_tool_parser_has_the_explain_tools_model_and_data_flags():
    from protopformer_amd.faithfulness import get_args_parser
    from protopformer_amd.train import get_args_parser as train_parser
    own = {o: a for a in get_args_parser()._actions for o in a.option_strings}
    shared = [(o, a) for a in train_parser()._actions for o in a.option_strings]
    assert len(shared) > 40
    for o, a in shared:
        assert o in own and own[o].dest == a.dest, f"{o} of train.py is missing"
        assert own[o].default == (0 if a.dest == "seed" else a.default), o               # the tool's own default seed is 0
    a = get_args_parser().parse_args([])
    assert (a.resume, a.split, a.steps, a.orders, a.modes, a.against_label, a.max_images, a.seed, a.per_image) == (
        "", "test", 14, ["evidence", "attention", "random"], ["deletion", "insertion"], False, 0, 0, False)
    a = get_args_parser().parse_args(["--resume", "x.pth", "--split", "train", "--steps", "7", "--orders", "evidence", "random", "--modes", "deletion",
                                      "--against_label", "--max_images", "5", "--seed", "3", "--per-image", "--output_dir", "o"])
    assert (a.resume, a.split, a.steps, a.orders, a.modes, a.against_label, a.max_images, a.seed, a.per_image, a.output_dir) == (
        "x.pth", "train", 7, ["evidence", "random"], ["deletion"], True, 5, 3, True, "o")


def test_summary_states_the_differences_to_the_random_order():
    from protopformer_amd.faithfulness import summarize
    res = dict(images=3, counts=[0, 8, 16], grid_cells=16, orders={
        "evidence": {"deletion": dict(curve=[0.9, 0.2, 0.1], auc=0.35), "insertion": dict(curve=[0.1, 0.8, 0.9], auc=0.65)},
        "random": {"deletion": dict(curve=[0.9, 0.5, 0.1], auc=0.5), "insertion": dict(curve=[0.1, 0.5, 0.9], auc=0.5)}})
    s = summarize(res)
    assert s["images"] == 3 and s["counts"] == [0, 8, 16] and s["orders"]["evidence"]["deletion"]["auc"] == 0.35
    assert s["vs_random"]["evidence"] == dict(deletion_auc_minus_random=pytest.approx(-0.15), insertion_auc_minus_random=pytest.approx(0.15), informative=True)
    assert "random" not in s["vs_random"]
