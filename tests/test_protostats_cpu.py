"""Prototype statistics without a GPU: everything protostats.py derives from the integer tables (AUROC, percentile, overlap, the keep
decision), the bin rule of the numpy referee against Python-float arithmetic, the argument validation of ppf_proto_stats_update (it
runs before any device call), the tool's parser, and Explanation.report with and without `stats`."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from protopformer_amd import protostats as S


# ------------------------------------------------------------------------------------------------ auroc
def brute_auroc_counts(own, other):
    """2 * (pairs own > other) + (pairs in the same bin), and 2 * n_own * n_other, by expanding the counts into binned values."""
    a = np.repeat(np.arange(own.size), own)
    b = np.repeat(np.arange(other.size), other)
    num = sum(2 * int((x > b).sum()) + int((x == b).sum()) for x in a)
    return num, 2 * a.size * b.size


def test_auroc_against_pairwise_count():
    rng = np.random.default_rng(0)
    hist = rng.integers(0, 6, size=(12, 2, 9))
    hist[rng.random(hist.shape) < 0.4] = 0
    hist[3, 0] = 0                                    # no own-class image
    hist[4, 1] = 0                                    # no other-class image
    hist[5] = 0
    hist[5, :, 6] = (7, 11)                           # all mass in one bin
    num, den = S.auroc_counts(hist)
    au = S.auroc(hist)
    for p in range(hist.shape[0]):
        want = brute_auroc_counts(hist[p, 0], hist[p, 1])
        assert (int(num[p]), int(den[p])) == want, p
        if want[1] == 0:
            assert np.isnan(au[p])
        else:
            assert au[p] == want[0] / want[1]
    assert np.isnan(au[3]) and np.isnan(au[4]) and au[5] == 0.5
    sep = np.zeros((2, 2, 8), dtype=np.int32)
    sep[0, 0, 7], sep[0, 1, 0] = 3, 5                 # own above other: 1; the other way round: 0
    sep[1, 0, 0], sep[1, 1, 7] = 3, 5
    assert S.auroc(sep).tolist() == [1.0, 0.0]


def test_auroc_counts_do_not_overflow_int32():
    hist = np.zeros((1, 2, 8), dtype=np.int32)
    hist[0, 0, 5], hist[0, 1, 2] = 60000, 70000
    num, den = S.auroc_counts(hist)
    assert int(num[0]) == int(den[0]) == 2 * 60000 * 70000


# ------------------------------------------------------------------------------------------------ percentile, overlap, mean / median
def test_percentile_hand_computed():
    hist = np.zeros((2, 2, 8), dtype=np.int32)
    hist[0, 0] = (0, 1, 0, 2, 0, 0, 0, 1)             # own
    hist[0, 1] = (4, 0, 0, 2, 0, 0, 0, 0)             # other
    t = dict(hist=hist, lo=np.float32(0), hi=np.float32(8))        # bin k = [k, k + 1)
    assert S.percentile(t, 0, 3.5, "own") == (1 + 0.5 * 2) / 4
    assert S.percentile(t, 0, 3.5, "other") == (4 + 0.5 * 2) / 6
    assert S.percentile(t, 0, 3.5) == (5 + 0.5 * 4) / 10
    assert S.percentile(t, 0, -1.0) == 0.5 * 4 / 10 and S.percentile(t, 0, 100.0, "own") == (3 + 0.5) / 4
    assert S.percentile(t, 0, 2.0, "own") == 1 / 4                 # an empty bin: only what lies below
    assert math.isnan(S.percentile(t, 0, float("nan"))) and math.isnan(S.percentile(t, 1, 3.5))
    with pytest.raises(ValueError, match="which"):
        S.percentile(t, 0, 1.0, "both")


def test_overlap_hand_computed():
    coloc = np.array([[4, 2, 0], [2, 8, 8], [0, 3, 0],            # class 0: prototype 2 has a zero diagonal
                      [5, 5, 5], [5, 5, 5], [5, 5, 5]], dtype=np.int32)
    ov = S.overlap(coloc, np.array([9, 5]))
    assert ov[0].tolist() == [1.0, 0.5, 0.0] and ov[1].tolist() == [0.25, 1.0, 1.0]
    assert np.isnan(ov[2]).all() and (ov[3:] == 1.0).all()
    with pytest.raises(ValueError, match="images"):
        S.overlap(coloc, np.array([9, 5, 1]))


def test_mean_and_median_bin_centres():
    hist = np.zeros((1, 2, 8), dtype=np.int32)
    hist[0, 0] = (1, 0, 0, 2, 0, 0, 0, 1)
    mean, med = S.mean_median(hist, 0.0, 16.0)                     # centres 1, 3, ..., 15
    assert mean[0, 0] == (1 + 2 * 7 + 15) / 4 and med[0, 0] == 7.0
    assert np.isnan(mean[0, 1]) and np.isnan(med[0, 1])


# ------------------------------------------------------------------------------------------------ keep_mask
def _hist_with_auroc(values, bins=8):
    """hist [P, 2, bins] whose AUROCs are exactly the given k / 8 fractions (None: no own-class image, NaN)."""
    hist = np.zeros((len(values), 2, bins), dtype=np.int32)
    for p, v in enumerate(values):
        hist[p, 1, 3] = 8                                          # 8 other-class images in bin 3
        if v is None:
            continue
        k = int(round(v * 8))
        hist[p, 0, 6], hist[p, 0, 0] = k, 8 - k                    # k own-class images above, 8 - k below
    return hist


def _stats(au_local, coloc, au_global, ppc, ppc_g):
    return {"local": dict(hist=_hist_with_auroc(au_local), coloc=np.asarray(coloc, dtype=np.int32), images=np.zeros(len(au_local) // ppc, np.int32)),
            "global": dict(hist=_hist_with_auroc(au_global), coloc=None, images=np.zeros(len(au_global) // ppc_g, np.int32))}


def _diag(P, ppc, n=8):
    c = np.zeros((P, ppc), dtype=np.int32)
    c[np.arange(P), np.arange(P) % ppc] = n
    return c


def test_keep_mask_rules():
    au = [0.75, 0.75, 1.0, 0.25,  0.25, 0.125, None, 0.25,  1.0, 0.875, 0.75, 0.625]
    assert np.array_equal(S.auroc(_hist_with_auroc(au))[[0, 2, 5]], [0.75, 1.0, 0.125])
    coloc = _diag(12, 4)
    coloc[0, 1] = 8                     # class 0: prototype 1 sits on prototype 0's cell in all of 0's images (the direction 0 -> 1 only)
    coloc[9, 0] = 8                     # class 2: 9 -> 8 at 1.0 (9 is visited after 8), 11 -> 10 below the bound
    coloc[11, 2] = 7
    st = _stats(au, coloc, [0.75, 0.25, None, 0.25], 4, 2)
    keep, why = S.keep_decisions(st, min_auroc=0.5, max_overlap=0.9, min_keep=1)
    # class 0: 2 (best), then 0 before 1 (tie to the smaller id), 1 dropped for the overlap although only ov[0][1] reaches it, 3 below 0.5
    # class 1: every AUROC below the threshold: the floor keeps the best one, the smaller id of the two 0.25s
    # class 2: 9 overlaps the kept 8; 11's 7/8 stays below 0.9
    assert keep["local"].tolist() == [True, False, True, False,  True, False, False, False,  True, False, True, True]
    assert "overlap" in why["local"][1] and "prototype 0" in why["local"][1] and "AUROC" in why["local"][3] and "undefined" in why["local"][6]
    assert set(why["local"]) == {1, 3, 5, 6, 7, 9}
    # the global branch: AUROC and the floor only (class 1: a known AUROC below the threshold ranks before an undefined one)
    assert keep["global"].tolist() == [True, False, False, True] and S.keep_mask(st)["global"].tolist() == keep["global"].tolist()
    assert S.keep_mask(st, min_keep=2)["local"].tolist() == [True, False, True, False,  True, False, False, True,  True, True, True, True]
    assert S.keep_mask(st, max_overlap=0.8)["local"][8:].tolist() == [True, False, True, False]
    assert S.keep_mask(st, min_auroc=0.8)["local"].tolist() == [False, False, True, False,  True, False, False, False,  True, False, False, False]


def test_keep_mask_global_ignores_overlap():
    """The same tables offered as either branch: the local one honours the co-location, the global one does not look at it."""
    au = [1.0, 0.875]
    coloc = np.full((2, 2), 8, dtype=np.int32)
    st = _stats(au, coloc, au, 2, 2)
    st["global"]["coloc"] = coloc
    keep = S.keep_mask(st)
    assert keep["local"].tolist() == [True, False] and keep["global"].tolist() == [True, True]


def test_keep_mask_same_under_permuted_order():
    """The decision is a function of the tables: classes offered in another order give the same decision per class, and a repeated call
    on tables rebuilt from shuffled samples gives the same mask."""
    rng = np.random.default_rng(3)
    P, ppc, C, N, T = 12, 3, 4, 60, 5
    act = (rng.integers(0, 70, size=(N, P)) / 8.0).astype(np.float32)
    argmax, idx = rng.integers(0, T, size=(N, P)), np.stack([rng.permutation(16)[:T] for _ in range(N)])
    labels = rng.integers(0, C, size=N)
    def tables(order):
        t = S.stats_from_outputs(act[order], argmax[order], idx[order], labels[order], ppc, 16, 0.0, 8.0)
        return {"local": t, "global": dict(t, coloc=None)}
    a, b = tables(np.arange(N)), tables(rng.permutation(N))
    assert all(np.array_equal(a["local"][k], b["local"][k]) for k in S.TABLES)
    ka, kb = S.keep_mask(a, 0.4, 0.5), S.keep_mask(b, 0.4, 0.5)
    assert np.array_equal(ka["local"], kb["local"]) and np.array_equal(ka["global"], kb["global"])
    perm = rng.permutation(C)                                      # the classes in another order
    rows = (perm[:, None] * ppc + np.arange(ppc)[None, :]).reshape(-1)
    c = {"local": dict(hist=a["local"]["hist"][rows], coloc=a["local"]["coloc"][rows], images=a["local"]["images"][perm]),
         "global": dict(hist=a["local"]["hist"][rows], coloc=None, images=a["local"]["images"][perm])}
    kc = S.keep_mask(c, 0.4, 0.5)
    assert np.array_equal(kc["local"], ka["local"][rows]) and np.array_equal(kc["global"], ka["global"][rows])


# ------------------------------------------------------------------------------------------------ the referee's bin rule
def py_bin(a, bins, lo, inv_width):
    """The rule in Python floats: every fp32 rounding explicit (a double product of two fp32 values rounds to fp32 as the fp32 product)."""
    if math.isnan(a):
        return None
    with np.errstate(over="ignore"):
        d = float(np.float32(float(a) - float(lo))) if math.isfinite(a) else a
        t = float(np.float32(d * float(inv_width))) if math.isfinite(d) else d
    if t < 0:
        return 0
    if t >= bins:
        return bins - 1
    return int(t)


@pytest.mark.parametrize("bins,lo,hi", [(16, 0.0, 8.0), (64, 0.0, math.log(1.0 / 1e-4)), (8, -1.5, 2.25), (128, 0.25, 7.0)])
def test_referee_bin_rule(bins, lo, hi):
    lo32, hi32 = np.float32(lo), np.float32(hi)
    w = S.inv_width_of(bins, lo, hi)
    assert w == np.float32(np.float32(bins) / np.float32(hi32 - lo32))
    edges = (lo32 + np.arange(bins + 1, dtype=np.float32) * np.float32((hi32 - lo32) / bins)).astype(np.float32)
    vals = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf)),
                           np.array([lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), -0.0, 0.0, np.inf, -np.inf, np.nan, 1e38, -1e38], dtype=np.float32)])
    b, nan = S.bin_index(vals, bins, lo, w)
    for v, got, isnan in zip(vals, b, nan):
        want = py_bin(float(v), bins, float(lo32), float(w))
        assert bool(isnan) == (want is None), v
        if want is not None:
            assert int(got) == want, (float(v), int(got), want)
    known = dict(zip(["lo", "hi", "below", "-0", "+inf", "-inf"], S.bin_index(np.array([lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), -0.0, np.inf,
                                                                                       -np.inf], dtype=np.float32), bins, lo, w)[0].tolist()))
    assert (known["lo"], known["hi"], known["below"], known["+inf"], known["-inf"]) == (0, bins - 1, 0, bins - 1, 0)
    if lo == 0.0:
        assert known["-0"] == 0
        if hi == 8.0:                                              # width 1/2: every multiple of 1/8 is exact, edges at the multiples of 1/2
            q = np.arange(0, 65, dtype=np.float32) / 8
            assert S.bin_index(q, bins, lo, w)[0].tolist() == [min(int(v * 2), bins - 1) for v in q.tolist()]


def test_referee_tables_known_answer():
    act = np.array([[0.0, 7.9, np.nan, 3.0], [9.0, -1.0, 2.0, np.nan], [1.0, 1.0, 1.0, 1.0], [5.0, 5.0, 5.0, 5.0]], dtype=np.float32)
    labels = np.array([0, 1, 2, -1])                               # classes 0, 1 of ppc = 2; labels 2 and -1 are bad
    argmax = np.array([[0, 0, 1, 1], [2, 1, 1, 3], [0, 0, 0, 0], [0, 0, 0, 0]])
    idx = np.array([[4, 6, 7], [1, 2, 3], [0, 1, 2], [0, 1, 2]])
    t = S.stats_from_outputs(act, argmax, idx, labels, 2, 8, 0.0, 8.0)
    assert t["images"].tolist() == [1, 1] and t["bad"].tolist() == [2]
    hist = np.zeros((4, 2, 8), dtype=np.int32)
    hist[0, 0, 0] = hist[1, 0, 7] = hist[3, 1, 3] = 1              # sample 0 (class 0): own for prototypes 0, 1
    hist[0, 1, 7] = hist[1, 1, 0] = hist[2, 0, 2] = 1              # sample 1 (class 1): own for prototypes 2, 3; 9.0 and -1.0 clamp
    assert np.array_equal(t["hist"], hist)
    assert t["nan_count"].tolist() == [[0, 0], [0, 0], [0, 1], [1, 0]]
    # sample 0: prototypes 0, 1 both at cell 4; sample 1: prototype 2 at cell 2, prototype 3's argmax = T is invalid
    assert t["coloc"].tolist() == [[1, 1], [1, 1], [1, 0], [0, 0]]
    g = S.stats_from_outputs(act, None, None, labels, 2, 8, 0.0, 8.0)
    assert g["coloc"] is None and np.array_equal(g["hist"], hist)
    with pytest.raises(ValueError, match="limits"):
        S.stats_from_outputs(act, argmax, idx, labels, 3, 8, 0.0, 8.0)


# ------------------------------------------------------------------------------------------------ the entry point's validation
@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


def test_entry_point_rejects_bad_shapes_before_any_device_call(lib):
    from protopformer_amd import _lib
    assert _lib.SIGS["ppf_proto_stats_update"] == "pppipiiiiffppppps"
    fn = lib.ppf_proto_stats_update
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS["ppf_proto_stats_update"]]
    good = dict(T=9, ppc=5, B=37, P=130, NB=16, lo=0.0, w=2.0)
    def call(**kw):
        a = dict(good, **kw)
        return fn(None, None, None, a["T"], None, a["ppc"], a["B"], a["P"], a["NB"], a["lo"], a["w"], None, None, None, None, None, None)
    for kw, word in ((dict(ppc=65), b"ppc=65"), (dict(ppc=0), b"ppc=0"), (dict(NB=7), b"NB=7"), (dict(NB=129), b"NB=129"), (dict(P=131), b"P=131"),
                     (dict(P=0), b"P=0"), (dict(B=1025), b"B=1025"), (dict(B=0), b"B=0"), (dict(lo=float("inf")), b"lo=inf"),
                     (dict(lo=float("nan")), b"lo=nan"), (dict(w=0.0), b"inv_width=0"), (dict(w=-1.0), b"inv_width=-1"),
                     (dict(w=float("inf")), b"inv_width=inf")):
        assert call(**kw) == _lib.DEFINES["PPF_ERR_SHAPE"], kw
        assert b"ppf_proto_stats_update" in lib.ppf_last_error() and word in lib.ppf_last_error(), (kw, lib.ppf_last_error())
    assert call() == _lib.DEFINES["PPF_ERR_ARG"] and b"null pointer" in lib.ppf_last_error()      # the shape passes, the pointers do not


# ------------------------------------------------------------------------------------------------ the object, the tool, explain
def _cpu_ppnet(activation="log"):
    from protopformer_amd.protopformer import construct_PPNet
    return construct_PPNet("deit_tiny_patch16_224", pretrained=False, prototype_shape=(20, 32, 1, 1), num_classes=10, reserve_layers=[11],
                           reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=3, add_on_layers_type="regular",
                           prototype_activation_function=activation)


def test_prototype_stats_ranges_and_state():
    lin = _cpu_ppnet("linear")
    with pytest.raises(ValueError, match="range"):
        S.PrototypeStats(lin)
    assert (S.PrototypeStats(lin, range=(-30.0, 0.0)).lo, S.PrototypeStats(lin, range=(-30.0, 0.0)).hi) == (np.float32(-30), np.float32(0))
    m = _cpu_ppnet()
    st = S.PrototypeStats(m, bins=16)
    assert st.lo == 0 and st.hi == np.float32(math.log(1.0 / 1e-4)) and st.inv_width == np.float32(np.float32(16) / st.hi)
    for bad in (7, 129):
        with pytest.raises(ValueError, match="bins"):
            S.PrototypeStats(m, bins=bad)
    with pytest.raises(ValueError, match="range"):
        S.PrototypeStats(m, range=(1.0, 1.0))
    # tables made elsewhere, held on the CPU: result() splits the one buffer by shape
    st.state["local"]["hist"][3, 1, 5] = 4
    st.state["global"]["images"][9] = 2
    st.state["local"]["coloc"][19, 1] = 6
    r = st.result()
    assert r["local"]["hist"].shape == (20, 2, 16) and r["local"]["coloc"].shape == (20, 2) and r["global"]["hist"].shape == (30, 2, 16)
    assert r["global"]["coloc"] is None and r["local"]["images"].shape == (10,) and r["global"]["nan_count"].shape == (30, 2)
    assert r["local"]["hist"][3, 1, 5] == 4 and r["global"]["images"][9] == 2 and r["local"]["coloc"][19, 1] == 6
    assert sum(int(v.sum()) for b in r.values() for k, v in b.items() if k in S.TABLES and v is not None) == 12
    other = S.PrototypeStats(m, bins=16)
    other.load_state_dict(copy.deepcopy(st.state_dict()))
    assert torch.equal(other.buf, st.buf)
    with pytest.raises(ValueError, match="bins=16"):
        S.PrototypeStats(m, bins=32).load_state_dict(st.state_dict())
    with pytest.raises(ValueError, match="range"):
        S.PrototypeStats(m, bins=16, range=(0.0, 9.0)).load_state_dict(st.state_dict())


def test_save_load_and_report(tmp_path):
    rng = np.random.default_rng(5)
    act = (rng.integers(0, 70, size=(40, 6)) / 8.0).astype(np.float32)
    labels = rng.integers(0, 3, size=40)
    loc = S.stats_from_outputs(act, rng.integers(0, 4, size=(40, 6)), np.tile(np.arange(4), (40, 1)), labels, 2, 16, 0.0, 8.0)
    glo = S.stats_from_outputs(act[:, :3], None, None, labels, 1, 16, 0.0, 8.0)
    result = {"local": dict(loc, lo=np.float32(0), hi=np.float32(8)), "global": dict(glo, lo=np.float32(0), hi=np.float32(8))}
    S.save_stats(str(tmp_path / "s.npz"), result)
    back = S.load_stats(str(tmp_path / "s.npz"))
    for br in S.BRANCHES:
        for k in S.TABLES:
            assert (back[br][k] is None and result[br][k] is None) or np.array_equal(back[br][k], result[br][k]), (br, k)
        assert back[br]["lo"] == 0 and back[br]["hi"] == 8
    doc = S.stats_report(back)
    assert doc["bins"] == 16 and doc["range"] == [0.0, 8.0] and doc["images"] == {"local": 40, "global": 40} and len(doc["prototypes"]) == 9
    assert sum(p["own_images"] + p["other_images"] for p in doc["prototypes"]) == 40 * 9
    first = doc["prototypes"][0]
    assert first["branch"] == "local" and first["auroc"] == float(S.auroc(loc["hist"])[0]) and "overlaps" in first
    assert "overlaps" not in doc["prototypes"][-1] and doc["prototypes"][-1]["class"] == 2
    import json
    json.dumps(doc)


def test_tool_parser_accepts_the_training_flags():
    a = S.get_args_parser().parse_args(["--base_architecture", "deit_tiny_patch16_224", "--no-pretrained", "--prototype_shape", "400", "64", "1", "1",
                                        "--reserve_layers", "11", "--reserve_token_nums", "81", "--use_global", "true", "--global_proto_per_class", "1",
                                        "--data_set", "CUB2011U", "--data_path", "/data", "--output_dir", "out", "--batch_size", "4", "--bins", "32",
                                        "--range", "0", "9.5", "--max_images", "10", "--split", "test", "--prune", "--min_auroc", "0.6",
                                        "--max_overlap", "0.8", "--min_keep", "2", "--save-pruned", "p.pth"])
    assert (a.bins, a.range, a.max_images, a.split, a.prune, a.min_auroc, a.max_overlap, a.min_keep, a.save_pruned) == \
        (32, [0.0, 9.5], 10, "test", True, 0.6, 0.8, 2, "p.pth")
    assert a.prototype_shape == [400, 64, 1, 1] and a.data_set == "CUB2011U"
    d = S.get_args_parser().parse_args([])
    assert (d.bins, d.range, d.split, d.prune, d.min_auroc, d.max_overlap, d.min_keep) == (64, None, "train", False, 0.5, 0.9, 1)
    from protopformer_amd.explain import get_args_parser
    assert get_args_parser().parse_args([]).stats == "" and get_args_parser().parse_args(["--stats", "s.npz"]).stats == "s.npz"


def _hand_explanation():
    from protopformer_amd.interpret import Explanation
    def branch(P0):
        return dict(classes=np.array([[1]], dtype=np.int32), class_logits=np.array([[2.5]], dtype=np.float32),
                    prototypes=np.array([[[P0, 0, -1]]], dtype=np.int32), contributions=np.array([[[1.5, 0.5, -np.inf]]], dtype=np.float32),
                    activations=np.array([[[3.5, 1.0, -np.inf]]], dtype=np.float32), cells=np.array([[[5, -1, -1]]], dtype=np.int32),
                    evidence=np.array([[[1.5, 0.5]]], dtype=np.float32), weights=np.array([[[1.0, -0.5, 0.0]]], dtype=np.float32))
    return Explanation(branch(2), branch(1), {"local": 2, "global": 1}, {"local": 0.7, "global": 0.3}, 4, 16, 64)


def test_explanation_report_with_and_without_stats():
    ex = _hand_explanation()
    plain = ex.report()
    assert plain == ex.report(None, None, None) == ex.report(stats=None)
    want_local = [dict(rank=0, prototype=2, prototype_class=1, weight=1.0, activation=3.5, contribution=1.5, cell=5, patch_box=[16, 16, 32, 32]),
                  dict(rank=1, prototype=0, prototype_class=0, weight=-0.5, activation=1.0, contribution=0.5, cell=None, patch_box=None)]
    assert plain[0]["classes"][0]["local"]["prototypes"] == want_local            # what it returned before the argument existed
    assert list(plain[0]["classes"][0]["global"]["prototypes"][0]) == ["rank", "prototype", "prototype_class", "weight", "activation", "contribution"]
    hist = np.zeros((4, 2, 8), dtype=np.int32)
    hist[2, 0] = (0, 1, 0, 2, 0, 0, 0, 1)
    hist[2, 1] = (4, 0, 0, 2, 0, 0, 0, 0)
    tables = dict(hist=hist, lo=np.float32(0), hi=np.float32(8))
    full = ex.report(stats={"local": tables, "global": tables})
    e = full[0]["classes"][0]["local"]["prototypes"]
    assert e[0]["percentile_all"] == (5 + 0.5 * 4) / 10 and e[0]["percentile_own"] == (1 + 0.5 * 2) / 4
    assert math.isnan(e[1]["percentile_all"]) and math.isnan(e[1]["percentile_own"])           # prototype 0 recorded nothing
    for rec in full:                                                                             # only the two keys are new
        for c in rec["classes"]:
            for br in ("local", "global"):
                for p in c[br]["prototypes"]:
                    del p["percentile_all"], p["percentile_own"]
    assert full == plain
