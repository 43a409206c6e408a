"""CPU-side checks of the local analysis: ppf_explain_topk is declared, exported and bound with one parameter list; its limits answer
through the error channel before any device call; the numpy referee (interpret.explain_from_outputs(device=False)) reproduces the
fixtures' logits and keeps the contract's order; Explanation.report and the tool's parser give known answers."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from helpers import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
NAME = "ppf_explain_topk"


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


def test_declared_exported_and_bound(lib):
    from protopformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b" + NAME + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, f"{NAME} is not declared in include/ppf_hip.h"
    assert hasattr(lib, NAME), f"{NAME} is not exported by the built library"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == 26 and _lib.SIGS[NAME] == "pppippfippiiiiiiipppppppps"
    assert lib.ppf_abi_version() == 10 == _lib.EXPECTED_ABI          # an addition: no existing entry point changed


def _call(lib, B=4, P=20, C=10, M=1, K=10, G=16, T=9, ppc=2, sign=1):
    """The entry point with its real argument types and pointers that are never dereferenced on a rejected shape."""
    from protopformer_amd import _lib
    fn = getattr(lib, NAME)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[NAME]]
    d = 4096                                                          # an aligned non-null address
    return fn(d, d, d, T, d, d, 0.5, ppc, d, None, sign, B, P, C, M, K, G, d, d, d, d, d, d, d, d, None)


@pytest.mark.parametrize("kw,word", [(dict(K=65), "K=65"), (dict(K=0), "K=0"), (dict(M=9), "M=9"), (dict(M=0), "M=0"), (dict(M=3, C=2), "M=3"),
                                     (dict(ppc=3), "ppc=3"), (dict(B=0), "B=0"), (dict(G=0), "G=0"), (dict(T=0), "T=0")])
def test_limits_answer_without_a_device(lib, kw, word):
    rc = _call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert rc == -1, f"{kw}: rc={rc} {msg}"                           # PPF_ERR_SHAPE
    assert NAME in msg and word in msg, msg


def test_bad_sign_is_an_argument_error(lib):
    assert _call(lib, sign=0) == -3 and "sign=0" in lib.ppf_last_error().decode()


# ------------------------------------------------------------------------------------------------ the referee on the fixtures
def _fixture_acts(z):
    d = z["eval/distances"].astype(np.float32)
    return np.log((d + np.float32(1)) / (d + np.float32(1e-4))).reshape(d.shape[0], d.shape[1], -1).max(-1).astype(np.float32)


@pytest.mark.parametrize("fixture", ["micro_deit.npz", "micro_cait.npz"])
def test_referee_evidence_adds_up_to_the_fixture_logits(fixture):
    from protopformer_amd.interpret import explain_from_outputs
    z = load_npz(fixture)
    act, W, coe = _fixture_acts(z), z["sd/last_layer.weight"].astype(np.float32), float(z["meta/global_coe"])
    (B, P), C = act.shape, W.shape[0]
    ref = z["eval/logits_local"].astype(np.float64)
    assert np.abs(act.astype(np.float64) @ W.T.astype(np.float64) - ref).max() < 2e-6     # the activations are the reference's
    for lo in range(0, C, 5):
        cls = np.tile(np.arange(lo, lo + 5, dtype=np.int32), (B, 1))
        r = explain_from_outputs(act, W, 1.0 - coe, P // C, z["eval/logits"], P, classes=cls, device=False)
        assert np.array_equal(r["classes"], cls) and np.array_equal(r["class_logits"], z["eval/logits"][:, lo:lo + 5])
        assert (np.sort(r["prototypes"], axis=-1) == np.arange(P)).all()                    # K = P: every prototype listed once
        mass = np.abs(r["contributions"].astype(np.float64)).sum(-1)
        err = np.abs(r["evidence"].astype(np.float64).sum(-1) - (1.0 - coe) * ref[:, lo:lo + 5])
        bound = 1.01 * P * 2.0 ** -24 * mass
        print(fixture, lo, "max err", err.max(), "min bound", bound.min())
        assert (err <= bound).all(), (err.max(), bound.min())
        # the class's own prototypes carry weight 1, all others -0.5: the own evidence is positive, the rest negative
        assert (r["evidence"][..., 0] > 0).all() and (r["evidence"][..., 1] < 0).all()


def _toy(act, weight, **kw):
    from protopformer_amd.interpret import explain_from_outputs
    act, weight = np.asarray(act, dtype=np.float32), np.asarray(weight, dtype=np.float32)
    logits = kw.pop("logits", np.zeros((act.shape[0], weight.shape[0]), dtype=np.float32))
    return explain_from_outputs(act, weight, kw.pop("scale", 1.0), kw.pop("ppc", 1), logits, kw.pop("topk"), device=False, **kw)


def test_referee_order_ties_sign_and_padding():
    inf = np.float32(np.inf)
    act = [[2.0, 3.0, 2.0, 1.0, 2.0, 0.5]]
    w = [[1.0, 1.0, 1.0, -4.0, 1.0, 1.0]]
    cls = np.zeros((1, 1), dtype=np.int32)
    r = _toy(act, w, topk=4, classes=cls)
    assert r["prototypes"].tolist() == [[[1, 0, 2, 4]]]                                    # duplicates resolve by prototype id
    assert r["contributions"].tolist() == [[[3.0, 2.0, 2.0, 2.0]]] and r["activations"].tolist() == [[[3.0, 2.0, 2.0, 2.0]]]
    assert r["cells"].tolist() == [[[-1, -1, -1, -1]]] and r["maps"] is None               # the global form
    r = _toy(act, w, topk=4, classes=cls, sign=-1)
    assert r["prototypes"].tolist() == [[[3, 5, 0, 2]]]                                    # key reversed, ties still by smaller id
    assert r["contributions"].tolist() == [[[-4.0, 0.5, 2.0, 2.0]]]
    assert r["evidence"].tolist() == [[[2.0, 3.5]]]                                        # ppc = 1: prototype 0 is class 0's own
    # NaN and inf are left out of the list and stay in the sums; K > P pads with -1 / -inf
    act2 = [[np.nan, 3.0, np.inf, 1.0]]
    r = _toy(act2, [[1.0, 1.0, 1.0, 1.0]], topk=6, classes=cls)
    assert r["prototypes"].tolist() == [[[1, 3, -1, -1, -1, -1]]]
    assert r["contributions"][0, 0, :2].tolist() == [3.0, 1.0] and (r["contributions"][0, 0, 2:] == -inf).all() and (r["activations"][0, 0, 2:] == -inf).all()
    assert np.isnan(r["evidence"][0, 0, 0]) and r["evidence"][0, 0, 1] == inf
    # classes: picked by logit with ties by smaller id and NaN never picked; out-of-range classes give an unfilled row
    r = _toy(act, np.ones((4, 6)), topk=2, top_classes=4, logits=np.array([[1.0, np.nan, 5.0, 1.0]], dtype=np.float32))
    assert r["classes"].tolist() == [[2, 0, 3, -1]] and r["class_logits"].tolist() == [[5.0, 1.0, 1.0, float("-inf")]]
    assert r["prototypes"][0, 3].tolist() == [-1, -1] and r["evidence"][0, 3].tolist() == [0.0, 0.0]
    r = _toy(act, np.ones((4, 6)), topk=2, classes=np.array([[-1, 4, 3]], dtype=np.int32))
    assert r["classes"].tolist() == [[-1, -1, 3]] and r["prototypes"].tolist() == [[[-1, -1], [-1, -1], [1, 0]]]


def test_referee_cells_and_maps():
    act = np.array([[1.0, 4.0, 2.0]], dtype=np.float32)
    full = np.arange(6, dtype=np.float32).reshape(1, 3, 2) + 1
    r = _toy(act, [[1.0, 1.0, 1.0]], topk=4, classes=np.zeros((1, 1), dtype=np.int32), argmax=np.array([[1, 2, 0]], dtype=np.int32),
             idx=np.array([[3, 0]], dtype=np.int32), act_full=full, grid_cells=4, maps=True)
    assert r["prototypes"].tolist() == [[[1, 2, 0, -1]]] and r["cells"].tolist() == [[[-1, 3, 0, -1]]]      # argmax == T: no cell
    assert r["maps"][0, 0].tolist() == [[4.0, 0, 0, 3.0], [6.0, 0, 0, 5.0], [2.0, 0, 0, 1.0], [0, 0, 0, 0]]


# ------------------------------------------------------------------------------------------------ the report
def _hand_made():
    from protopformer_amd.interpret import Explanation
    inf = np.float32(-np.inf)
    local = dict(classes=np.array([[3, -1]], dtype=np.int32), class_logits=np.array([[2.5, inf]], dtype=np.float32),
                 prototypes=np.array([[[6, 7, -1], [-1, -1, -1]]], dtype=np.int32),
                 contributions=np.array([[[1.5, 0.25, inf], [inf, inf, inf]]], dtype=np.float32),
                 activations=np.array([[[3.0, 0.5, inf], [inf, inf, inf]]], dtype=np.float32),
                 cells=np.array([[[15, -1, -1], [-1, -1, -1]]], dtype=np.int32), weights=np.array([[[1.0, 1.0, 0.0], [0.0, 0.0, 0.0]]], dtype=np.float32),
                 evidence=np.array([[[1.75, -0.5], [0.0, 0.0]]], dtype=np.float32), boxes=np.zeros((1, 2, 3, 4), dtype=np.int32) + np.array([1, 9, 2, 8], dtype=np.int32))
    glob = dict(classes=local["classes"], class_logits=local["class_logits"], prototypes=np.array([[[3, -1, -1], [-1, -1, -1]]], dtype=np.int32),
                contributions=np.array([[[1.0, inf, inf], [inf, inf, inf]]], dtype=np.float32),
                activations=np.array([[[2.0, inf, inf], [inf, inf, inf]]], dtype=np.float32), cells=np.full((1, 2, 3), -1, dtype=np.int32),
                weights=np.ones((1, 2, 3), dtype=np.float32), evidence=np.array([[[1.0, 0.25], [0.0, 0.0]]], dtype=np.float32))
    return Explanation(local, glob, {"local": 2, "global": 1}, {"local": 0.5, "global": 0.5}, side=14, patch_size=16, img_size=224)


def test_report_on_a_hand_made_explanation():
    ex = _hand_made()
    assert ex.cpu() is ex and ex.prototypes is ex.local["prototypes"] and ex.global_["maps"] is None
    bank = {"local_filled": np.array([0] * 6 + [2, 0]), "local_image_ids": np.full((8, 2), -1), "local_values": np.full((8, 2), -np.inf),
            "local_grid_pos": np.full((8, 2), -1), "global_filled": np.array([0, 0, 0, 1]), "global_image_ids": np.array([[-1, -1]] * 3 + [[11, -1]]),
            "global_values": np.array([[-np.inf, -np.inf]] * 3 + [[9.0, -np.inf]]), "global_grid_pos": np.full((4, 2), -1)}
    bank["local_image_ids"][6], bank["local_values"][6], bank["local_grid_pos"][6] = (40, 41), (5.0, 4.0), (0, 195)
    recs = ex.report(bank=bank)
    assert json.loads(json.dumps(recs)) == recs and len(recs) == 1
    rec = recs[0]
    assert rec["image"] == 0 and rec["against"] is False and [c["class"] for c in rec["classes"]] == [3]      # the class -1 slot is dropped
    c = rec["classes"][0]
    assert c["logit"] == 2.5 and c["local"]["evidence_own"] == 1.75 and c["local"]["evidence_other"] == -0.5 and c["global"]["scale"] == 0.5
    lp = c["local"]["prototypes"]
    assert [e["prototype"] for e in lp] == [6, 7] and [e["rank"] for e in lp] == [0, 1]                         # the unfilled slot is dropped
    assert lp[0] == dict(rank=0, prototype=6, prototype_class=3, weight=1.0, activation=3.0, contribution=1.5, cell=15, patch_box=[16, 16, 32, 32],
                         activation_box=[1, 9, 2, 8], nearest=[dict(rank=0, image_id=40, activation=5.0, grid_pos=0),
                                                               dict(rank=1, image_id=41, activation=4.0, grid_pos=195)])
    assert lp[1]["cell"] is None and lp[1]["patch_box"] is None and lp[1]["nearest"] == []
    gp = c["global"]["prototypes"]
    assert len(gp) == 1 and set(gp[0]) == {"rank", "prototype", "prototype_class", "weight", "activation", "contribution", "nearest"}
    assert gp[0]["prototype_class"] == 3 and gp[0]["nearest"] == [dict(rank=0, image_id=11, activation=9.0, grid_pos=-1)]
    assert ex.report(index=0) == ex.report(index=[0]) == ex.report()
    assert "nearest" not in ex.report()[0]["classes"][0]["local"]["prototypes"][0]
    with pytest.raises(IndexError):
        ex.report(index=1)


def test_class_lists_are_range_checked_on_the_host():
    import torch

    from protopformer_amd.interpret import _explain_classes
    assert _explain_classes([1, 2], 2, 10, "cpu").tolist() == [[1], [2]] and _explain_classes([[1, 2]], 1, 10, "cpu").dtype == torch.int32
    for bad in ([1, 10], [-1, 0]):
        with pytest.raises(ValueError, match=r"\[0, 10\)"):
            _explain_classes(bad, 2, 10, "cpu")
    with pytest.raises(ValueError, match="batch of 3"):
        _explain_classes([1, 2], 3, 10, "cpu")
    with pytest.raises(ValueError, match="integers"):
        _explain_classes([0.5, 1.0], 2, 10, "cpu")


# ------------------------------------------------------------------------------------------------ the tool's parser
def test_tool_parser_has_the_bank_tools_model_and_data_flags():
    from protopformer_amd.bank import get_args_parser as bank_parser
    from protopformer_amd.explain import get_args_parser
    from protopformer_amd.train import get_args_parser as train_parser
    shared = {a.dest for a in train_parser()._actions} | {"split", "topk"}
    bank, own = {a.dest: a for a in bank_parser()._actions}, {a.dest: a for a in get_args_parser()._actions}
    assert len(shared) > 40
    for dest in shared:
        assert dest in own, f"--{dest} of the bank tool is missing"
        assert own[dest].default == bank[dest].default and own[dest].option_strings == bank[dest].option_strings, dest
    a = get_args_parser().parse_args([])
    assert (a.resume, a.split, a.topk, a.top_classes, a.against, a.max_images, a.bank, a.render) == ("", "train", 10, 1, False, 0, "", False)
    a = get_args_parser().parse_args(["--resume", "x.pth", "--split", "test", "--topk", "3", "--top_classes", "5", "--against", "--max_images", "7",
                                      "--bank", "b.npz", "--render", "--output_dir", "o", "--prototype_shape", "400", "64", "1", "1"])
    assert (a.resume, a.split, a.topk, a.top_classes, a.against, a.max_images, a.bank, a.render, a.output_dir) == ("x.pth", "test", 3, 5, True, 7,
                                                                                                                    "b.npz", True, "o")
    assert a.prototype_shape == [400, 64, 1, 1]
