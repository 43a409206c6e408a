"""CPU-side checks of the foreground-focus pass: ppf_act_focus, ppf_focus_box_terms, ppf_reserve_focus and ppf_evidence_focus are declared,
exported and bound with one parameter list each (the ABI version unchanged) and answer their limits through the error channel before
any device call; interpret.scaled_boxes against hand-computed boxes; the numpy referees (device=False) against brute-force loops on
tiny inputs; the summary's arithmetic; the tool's parser and its box reading on a miniature CUB tree."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ppf_hip.h")
SPECS = {"ppf_act_focus": "ppiiiipppppps", "ppf_focus_box_terms": "ppiiips", "ppf_reserve_focus": "pppiiiipps",
         "ppf_evidence_focus": "pppipfippiiiiiipps"}


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
    assert len(re.findall(r"\b" + name + r"\s*\(", src)) == 1, f"{name} is declared more than once"
    assert hasattr(lib, name), f"{name} is not exported by the built library"
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert nargs == len(SPECS[name]) and _lib.SIGS[name] == SPECS[name]
    assert lib.ppf_abi_version() == _lib.EXPECTED_ABI == 10              # additions: no existing entry point changed


def _fn(lib, name):
    from protopformer_amd import _lib
    fn = getattr(lib, name)
    fn.restype = ctypes.c_int
    fn.argtypes = [_lib._CT[c] for c in _lib.SIGS[name]]
    return fn


D = 4096                                                              # an aligned non-null address, never dereferenced on a rejected call


def _focus(lib, grids=D, obj=D, M=6, g=14, S=224, per=3, hit=D):
    return _fn(lib, "ppf_act_focus")(grids, obj, M, g, S, per, D, D, hit, D, D, None, None)


def _terms(lib, box=D, M=6, per=3, S=224, terms=D):
    return _fn(lib, "ppf_focus_box_terms")(box, D, M, per, S, terms, None)


def _reserve(lib, idx=D, ta=None, B=2, T=9, g=14, patch=16, attn=None):
    return _fn(lib, "ppf_reserve_focus")(idx, D, ta, B, T, g, patch, D, attn, None)


def _evidence(lib, act=D, B=2, P=20, C=10, M=1, T=9, ppc=2, g=14, patch=16, ev=D):
    return _fn(lib, "ppf_evidence_focus")(act, None, D, T, D, 0.5, ppc, D, D, g, patch, B, P, C, M, ev, D, None)


@pytest.mark.parametrize("call,kw,rc,word", [
    (_focus, dict(M=0), -1, "M=0"), (_focus, dict(g=65), -1, "g=65"), (_focus, dict(S=1025), -1, "S=1025"), (_focus, dict(g=64, S=1024), -1, "LDS"),
    (_focus, dict(per=4), -1, "maps_per_img=4"), (_focus, dict(per=0), -1, "maps_per_img=0"), (_focus, dict(grids=None), -3, "null"),
    (_focus, dict(obj=None), -3, "null"), (_focus, dict(hit=None), -3, "null"),
    (_terms, dict(M=0), -1, "M=0"), (_terms, dict(S=0), -1, "S=0"), (_terms, dict(S=32769), -1, "S=32769"), (_terms, dict(per=4), -1, "maps_per_img=4"),
    (_terms, dict(box=None), -3, "null"), (_terms, dict(terms=None), -3, "null"),
    (_reserve, dict(B=0), -1, "B=0"), (_reserve, dict(T=0), -1, "T=0"), (_reserve, dict(g=4096, patch=16), -1, "g=4096"), (_reserve, dict(patch=0), -1, "patch=0"),
    (_reserve, dict(T=1 << 20, g=2, patch=16384), -1, "overflow"), (_reserve, dict(idx=None), -3, "null"), (_reserve, dict(ta=D), -3, "token_attn"),
    (_reserve, dict(attn=D), -3, "token_attn"),
    (_evidence, dict(M=9), -1, "M=9"), (_evidence, dict(M=0), -1, "M=0"), (_evidence, dict(B=0), -1, "B=0"), (_evidence, dict(T=0), -1, "T=0"),
    (_evidence, dict(ppc=3), -1, "ppc=3"), (_evidence, dict(g=0), -1, "g=0"), (_evidence, dict(act=None), -3, "null"), (_evidence, dict(ev=None), -3, "null")])
def test_limits_answer_without_a_device(lib, call, kw, rc, word):
    got = call(lib, **kw)
    msg = lib.ppf_last_error().decode()
    assert got == rc, f"{kw}: rc={got} {msg}"
    assert word in msg and msg.startswith("ppf_"), msg


# ------------------------------------------------------------------------------------------------ scaled_boxes
def test_scaled_boxes_against_hand_computed_boxes():
    from protopformer_amd.interpret import scaled_boxes
    boxes = {1: (10, 20, 60, 80), 2: (0, 0, 100, 50), 3: (95, 45, 130, 70), 4: (37, 11, 38, 12), 5: (0, 0, 1, 1), 6: (149, 299, 150, 300),
             7: (33, 10, 66, 20)}
    sizes = {1: (100, 200), 2: (100, 50), 3: (100, 50), 4: (300, 150), 5: (500, 333), 6: (150, 300), 7: (99, 30)}
    got = scaled_boxes([1, 2, 3, 4, 5, 6, 7], boxes, sizes, 224)
    assert got.dtype == np.int32 and got.shape == (7, 4)
    # rows are (Y0, Y1, X0, X1).  1: x 10..60 of 100 -> floor(22.4) = 22 .. ceil(134.4) = 135; y 20..80 of 200 -> floor(22.4) = 22 .. ceil(89.6) = 90
    assert got[0].tolist() == [22, 90, 22, 135]
    assert got[1].tolist() == [0, 224, 0, 224]                        # touching the file's border on all sides: the whole view
    assert got[2].tolist() == [201, 224, 212, 224]                    # exceeding it: floor(224*45/50) = 201, floor(224*95/100) = 212, the ends cut to S
    assert got[3].tolist() == [16, 18, 27, 29]                        # one pixel of a larger file: floor(16.43) .. ceil(17.92), floor(27.63) .. ceil(28.37)
    assert got[4].tolist() == [0, 1, 0, 1]                            # one pixel of a file larger than the view: ceil(0.67) = 1, ceil(0.448) = 1
    assert got[5].tolist() == [223, 224, 222, 224]                    # the last pixel: floor(223.25) .. 224, floor(222.5) .. 224
    assert got[6].tolist() == [74, 150, 74, 150]                      # non-square 99 x 30: floor(74.67) .. ceil(149.33) both ways
    assert scaled_boxes([], boxes, sizes, 224).shape == (0, 4)
    # the order of the ids is the order of the rows
    assert scaled_boxes([4, 1], boxes, sizes, 224).tolist() == [got[3].tolist(), got[0].tolist()]


def test_scaled_box_is_never_empty_and_covers_the_source():
    from protopformer_amd.interpret import scaled_boxes
    rng = np.random.default_rng(0)
    for S in (1, 7, 64, 224):
        for n in range(200):
            w, h = int(rng.integers(1, 700)), int(rng.integers(1, 700))
            x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
            x1, y1 = int(rng.integers(x0 + 1, w + 3)), int(rng.integers(y0 + 1, h + 3))        # may exceed the border by up to two pixels
            Y0, Y1, X0, X1 = scaled_boxes([0], {0: (x0, y0, x1, y1)}, {0: (w, h)}, S)[0].tolist()
            assert 0 <= X0 < X1 <= S and 0 <= Y0 < Y1 <= S, (S, w, h, x0, y0, x1, y1)
            assert X0 <= S * x0 / w and (X1 >= S * min(x1, w) / w) and Y0 <= S * y0 / h and (Y1 >= S * min(y1, h) / h)


# ------------------------------------------------------------------------------------------------ the referees against loops
def test_act_focus_referee_agrees_with_a_loop():
    from protopformer_amd.interpret import act_focus, resize_cubic
    rng = np.random.default_rng(1)
    g, S = 3, 7
    grids = rng.standard_normal((6, g, g)).astype(np.float32)
    grids[1] = -np.abs(grids[1])                                     # all negative (the cubic kernel overshoots: not all <= 0 after up-sampling)
    grids[2, 1, 1] = np.nan
    grids[3] = np.nan
    grids[4, 0, 0], grids[4, 2, 2] = np.inf, -np.inf
    grids[5] = 2.5
    obj = np.array([[1, 5, 2, 6], [-3, 99, -3, 99], [3, 3, 0, 7]], dtype=np.int32)         # interior; larger than the image; empty
    r = act_focus(grids, S, obj, device=False)
    assert r["inside"].dtype == r["total"].dtype == np.float64 and r["peak_yx"].dtype == r["hit"].dtype == r["nonfinite"].dtype == np.int32
    for m in range(6):
        with np.errstate(invalid="ignore"):
            up = resize_cubic(grids[m], S)
        y0, y1, x0, x1 = np.clip(obj[m // 2], 0, S)
        best, at, ti, tt, bad = -np.inf, None, 0.0, 0.0, 0
        for y in range(S):
            for x in range(S):
                v = float(up[y, x])
                if v > best:
                    best, at = v, (y, x)
                if not math.isfinite(v):
                    bad += 1
                    continue
                tt += max(v, 0.0)
                if y0 <= y < y1 and x0 <= x < x1:
                    ti += max(v, 0.0)
        if at is None:
            at = next(((y, x) for y in range(S) for x in range(S) if up[y, x] == -np.inf), (0, 0))
        assert tuple(r["peak_yx"][m]) == at and (r["peak_val"][m] == np.float32(best)), m
        assert r["hit"][m] == int(y0 <= at[0] < y1 and x0 <= at[1] < x1) and r["nonfinite"][m] == bad
        assert abs(r["inside"][m] - ti) <= 49 * 2.0 ** -52 * ti and abs(r["total"][m] - tt) <= 49 * 2.0 ** -52 * tt
    assert r["nonfinite"][3] == 49 and tuple(r["peak_yx"][3]) == (0, 0) and r["peak_val"][3] == -np.inf and r["total"][3] == 0
    assert r["inside"][2] == r["total"][2] and r["inside"][4] == r["inside"][5] == 0                      # the whole image; the empty box
    assert r["hit"][5] == 0
    with pytest.raises(ValueError, match="do not divide"):
        act_focus(grids[:5], S, obj, device=False)


def test_box_terms_referee_agrees_with_a_pixel_count():
    from protopformer_amd.interpret import focus_box_terms
    S = 12
    box = np.array([[0, 1, 0, 1], [2, 9, 3, 11], [0, 12, 0, 12], [5, 5, 0, 12], [-4, 6, -2, 20], [8, 12, 8, 12]], dtype=np.int32)
    obj = np.array([[1, 8, 2, 10], [4, 20, -5, 9], [7, 3, 1, 2]], dtype=np.int32)
    got = focus_box_terms(box, obj, S, device=False)
    assert got.dtype == np.int32 and got.shape == (6, 4)
    for m in range(6):
        a, o = np.zeros((S, S), dtype=bool), np.zeros((S, S), dtype=bool)
        for mask, b in ((a, box[m]), (o, obj[m // 2])):
            for y in range(S):
                for x in range(S):
                    mask[y, x] = b[0] <= y < b[1] and b[2] <= x < b[3]
        assert got[m].tolist() == [int((a & o).sum()), int(a.sum()), int(o.sum()), int((a | o).sum())], m


def test_reserve_referee_agrees_with_a_pixel_count():
    from protopformer_amd.interpret import reserve_focus
    g, patch = 4, 3
    S = g * patch
    idx = np.array([[0, 5, 5, 15, -1, 16], [3, 6, 9, 12, 1, 2], [7, 7, 7, 7, 7, 7]], dtype=np.int32)          # out of range; duplicates
    obj = np.array([[2, 10, 1, 8], [0, 12, 0, 12], [5, 5, 0, 12]], dtype=np.int32)
    rng = np.random.default_rng(2)
    ta = rng.random((3, g * g)).astype(np.float32)
    ta[0, 3], ta[0, 6], ta[1, 0] = np.nan, np.inf, -np.inf
    out, attn = reserve_focus(idx, obj, g, patch, ta, device=False)
    assert out.dtype == np.int32 and attn.dtype == np.float64
    for b in range(3):
        inside = lambda y, x: obj[b, 0] <= y < obj[b, 1] and obj[b, 2] <= x < obj[b, 3]
        pix = cen = valid = 0
        for c in idx[b]:
            if not 0 <= c < g * g:
                continue
            valid += 1
            cy, cx = divmod(int(c), g)
            pix += sum(inside(y, x) for y in range(cy * patch, (cy + 1) * patch) for x in range(cx * patch, (cx + 1) * patch))
            cen += inside(cy * patch + patch // 2, cx * patch + patch // 2)
        cells = [c for c in range(g * g) if inside((c // g) * patch + patch // 2, (c % g) * patch + patch // 2)]
        assert out[b].tolist() == [pix, cen, len(cells), valid], b
        fin = lambda v: float(v) if math.isfinite(v) else 0.0
        assert abs(attn[b, 0] - math.fsum(fin(ta[b, c]) for c in cells)) <= 16 * 2.0 ** -52 * attn[b, 1]
        assert abs(attn[b, 1] - math.fsum(fin(v) for v in ta[b])) <= 16 * 2.0 ** -52 * attn[b, 1]
    assert out[1].tolist() == [6 * patch * patch, 6, 16, 6] and out[2].tolist() == [0, 0, 0, 6]
    assert reserve_focus(idx, obj, g, patch, device=False)[1] is None


def test_evidence_referee_agrees_with_a_loop():
    from protopformer_amd.interpret import evidence_focus
    rng = np.random.default_rng(3)
    B, C, ppc, T, g, patch = 3, 4, 2, 5, 3, 4
    P = C * ppc
    act = rng.random((B, P)).astype(np.float32) * 4
    act[2, 3] = np.nan
    w = np.where(np.arange(P)[None, :] // ppc == np.arange(C)[:, None], 1.0, -0.5).astype(np.float32) + rng.standard_normal((C, P)).astype(np.float32) * 0.01
    idx = np.array([[0, 2, 4, 6, 8], [1, 3, 5, 7, 9], [8, 4, 0, -1, 2]], dtype=np.int32)               # a cell outside the grid (9, -1)
    argmax = rng.integers(0, T, (B, P)).astype(np.int32)
    argmax[0, 0], argmax[0, 1], argmax[1, 4] = -1, T, 4                                                # out of range twice; -> cell 9: not located
    obj = np.array([[0, 8, 0, 8], [0, 12, 0, 12], [4, 12, 0, 4]], dtype=np.int32)
    cls = np.array([[1, -1], [3, 0], [1, 4]], dtype=np.int32)
    scale = 0.3
    ev, cnt = evidence_focus(act, w, scale, ppc, cls, obj, g, patch, idx, argmax, device=False)
    assert ev.dtype == np.float64 and cnt.dtype == np.int32 and ev.shape == cnt.shape == (B, 2, 4)
    for b in range(B):
        for m in range(2):
            c = int(cls[b, m])
            sums, n = [0.0] * 4, [0] * 4
            if 0 <= c < C:
                for p in range(P):
                    ctr = np.float32(act[b, p] * np.float32(np.float32(scale) * w[c, p]))
                    t, inside = int(argmax[b, p]), False
                    if 0 <= t < T and 0 <= idx[b, t] < g * g:
                        cy, cx = divmod(int(idx[b, t]), g)
                        py, px = cy * patch + patch // 2, cx * patch + patch // 2
                        inside = obj[b, 0] <= py < obj[b, 1] and obj[b, 2] <= px < obj[b, 3]
                    k = (0 if p // ppc == c else 2) + (0 if inside else 1)
                    sums[k] += float(ctr)
                    n[k] += 1
            assert cnt[b, m].tolist() == n and sum(n) == (P if 0 <= c < C else 0), (b, m)
            for k in range(4):
                assert (math.isnan(sums[k]) and math.isnan(ev[b, m, k])) or abs(ev[b, m, k] - sums[k]) <= P * 2.0 ** -52 * 4.0, (b, m, k)
    assert np.isnan(ev[2, 0]).sum() == 1 and not ev[0, 1].any() and not ev[2, 1].any()                 # the NaN stays in its sum; classes -1 and C: zeros
    # argmax None (k = 1): every prototype sits at idx[b][0]
    ev1, cnt1 = evidence_focus(act, w, scale, ppc, cls[:, :1], obj, g, patch, idx[:, :1], None, device=False)
    assert cnt1[0, 0].tolist() == [ppc, 0, P - ppc, 0] and cnt1[2, 0].tolist() == [0, ppc, 0, P - ppc]   # cell 0 inside obj 0; cell 8 outside obj 2


# ------------------------------------------------------------------------------------------------ the summary
def _rows(seed=4, N=7, K=2):
    rng = np.random.default_rng(seed)
    total = rng.random((N, K)) * 3
    total[2, 1] = 0.0
    inside = total * rng.random((N, K))
    nonfinite = np.zeros((N, K), dtype=np.int32)
    nonfinite[4, 0] = 3
    terms = np.zeros((N, K, 4), dtype=np.int32)
    terms[..., 1], terms[..., 2] = rng.integers(1, 30, (N, K)), rng.integers(0, 40, (N, 1))
    terms[..., 0] = np.minimum(terms[..., 1], terms[..., 2]) // 2
    terms[..., 3] = terms[..., 1] + terms[..., 2] - terms[..., 0]
    reserve = np.stack([rng.integers(0, 36, N), rng.integers(0, 4, N), rng.integers(0, 9, N), np.full(N, 9)], axis=1).astype(np.int32)
    reserve[3, 2] = reserve[3, 1] = 0                                   # no grid cell has its centre in this image's box
    reserve[5, 3] = reserve[5, 0] = reserve[5, 1] = 0                   # no valid reserved cell
    ev = rng.random((N, 4)) * np.array([1, 1, -1, -1])
    ev[1, :2] = 0.0                                                      # no own evidence
    obj = np.array([[0, int(a), 0, int(b)] for a, b in rng.integers(0, 9, (N, 2))], dtype=np.int32)
    return dict(image_ids=np.array([11, 3, 8, 5, 9, 2, 7]), protos=rng.integers(0, 6, (N, K)).astype(np.int32), classes=rng.integers(0, 3, N).astype(np.int32),
                hit=rng.integers(0, 2, (N, K)).astype(np.int32), inside=inside, total=total, nonfinite=nonfinite, terms=terms, reserve=reserve,
                attn=np.stack([rng.random(N), 1 + rng.random(N)], axis=1), ev=ev, cnt=np.ones((N, 4), dtype=np.int32), global_ev=rng.random(N),
                obj=obj, labels=rng.integers(0, 3, N).astype(np.int64), peak_val=total.astype(np.float32), peak_yx=np.zeros((N, K, 2), dtype=np.int32),
                box=np.zeros((N, K, 4), dtype=np.int32))


TOL = 16 * 2.0 ** -52        # an fp64 mean of at most 14 values below 1, summed in another order than numpy's: n * 2^-52, rounded up


def test_summary_counts_zero_denominators_and_ignores_row_order():
    from protopformer_amd.interpret import focus_summary
    rows = _rows()
    s = focus_summary(rows, 8, 2)
    N, K = 7, 2
    o = s["overall"]
    assert s["images"] == N and s["rows"] == N * K
    pm = o["prototype_maps"]
    assert pm["rows"] == 14 and pm["energy_rows"] == 13 and pm["zero_total_rows"] == 1 and pm["nonfinite_rows"] == 1
    assert pm["pointing"] == int(rows["hit"].sum()) / 14
    live = rows["total"] > 0
    assert abs(pm["energy"] - (rows["inside"][live] / rows["total"][live]).mean()) <= TOL
    assert abs(pm["iou"] - (rows["terms"][..., 0] / rows["terms"][..., 3]).mean()) <= TOL
    assert abs(pm["box_inside"] - (rows["terms"][..., 0] / rows["terms"][..., 1]).mean()) <= TOL
    assert abs(pm["chance"] - (rows["terms"][..., 2] / 64.0).mean()) <= TOL
    rv = o["reservation"]
    assert rv["images"] == 7 and rv["images_without_object_cells"] == int((rows["reserve"][:, 2] == 0).sum()) >= 1
    ok = rows["reserve"][:, 3] > 0
    assert abs(rv["reserved_on_object"] - (rows["reserve"][ok, 0] / (rows["reserve"][ok, 3] * 4.0)).mean()) <= TOL and ok.sum() == 6
    have = rows["reserve"][:, 2] > 0
    assert abs(rv["object_recall"] - (rows["reserve"][have, 1] / rows["reserve"][have, 2]).mean()) <= TOL
    assert abs(rv["attention_on_object"] - (rows["attn"][:, 0] / rows["attn"][:, 1]).mean()) <= TOL
    assert abs(rv["chance"] - (rows["obj"][:, 1] * rows["obj"][:, 3] / 64.0).mean()) <= TOL
    e = o["evidence"]
    assert e["own_images"] == 6 and e["other_images"] == 0 and e["other_inside"] is None        # negative evidence is not "> 0": counted out
    own = rows["ev"][:, 0] + rows["ev"][:, 1]
    assert abs(e["own_inside"] - (rows["ev"][own > 0, 0] / own[own > 0]).mean()) <= TOL and e["global_branch_share"] is not None
    # per class (by label) and per prototype partition the rows
    assert sorted(s["per_class"]) == sorted(set(rows["labels"].tolist()))
    assert sum(v["prototype_maps"]["rows"] for v in s["per_class"].values()) == 14 and sum(v["reservation"]["images"] for v in s["per_class"].values()) == 7
    assert sorted(s["per_prototype"]) == sorted(set(rows["protos"].reshape(-1).tolist())) and sum(v["rows"] for v in s["per_prototype"].values()) == 14
    assert focus_summary(rows, 8, 2, per_prototype=False)["per_prototype"] is None
    # any order of the rows, and so any batching, gives the same record, bit for bit
    for seed in (0, 1):
        perm = np.random.default_rng(seed).permutation(N)
        assert focus_summary({k: v[perm] for k, v in rows.items()}, 8, 2) == s
    # without labels the class is the predicted one; without the global branch its share is None
    t = focus_summary(dict(rows, labels=None, global_ev=None, attn=None), 8, 2)
    assert sorted(t["per_class"]) == sorted(set(rows["classes"].tolist())) and t["overall"]["evidence"]["global_branch_share"] is None
    assert t["overall"]["reservation"]["attention_on_object"] is None
    empty = focus_summary({k: (v[:0] if v is not None else None) for k, v in rows.items()}, 8, 2)
    assert empty["images"] == 0 and empty["overall"]["prototype_maps"]["pointing"] is None and empty["per_class"] == {}


def test_focus_from_outputs_host_pipeline_on_synthetic_outputs():
    """The referee pipeline end to end on the host, both selections; K and the shapes of every field."""
    import torch
    from protopformer_amd.interpret import FOCUS_FIELDS, focus_from_outputs
    rng = np.random.default_rng(5)
    B, C, ppc, k, g, S = 3, 4, 3, 4, 4, 16
    P, G = C * ppc, g * g
    ta = rng.random((B, G)).astype(np.float32)
    idx = np.sort(np.argsort(-ta, axis=1)[:, :k], axis=1).astype(np.int32)
    act_full = rng.random((B, P, k)).astype(np.float32)
    outs = dict(token_attn=ta, idx=idx, act_full=act_full, logits=rng.standard_normal((B, C)).astype(np.float32), act_max=act_full.max(-1),
                argmax=act_full.argmax(-1).astype(np.int32), logits_global=rng.standard_normal((B, C)).astype(np.float32))
    w = np.where(np.arange(P)[None, :] // ppc == np.arange(C)[:, None], 1.0, -0.5).astype(np.float32)
    obj = np.array([[0, 16, 0, 16], [4, 12, 4, 12], [9, 9, 0, 16]], dtype=np.int32)
    labels = np.array([2, 0, 3])
    for mode, K in (("own", ppc), ("top", 2)):
        f = focus_from_outputs(outs, obj, w, 0.5, ppc, k, S, labels, mode, 2, 95, 0.5, device=False)
        assert f.on_host and f.cpu() is f and (f.grid_side, f.patch, f.img_size, f.mode) == (g, 4, S, mode)
        shapes = dict(protos=(B, K), classes=(B,), peak_val=(B, K), peak_yx=(B, K, 2), hit=(B, K), inside=(B, K), total=(B, K), nonfinite=(B, K),
                      box=(B, K, 4), terms=(B, K, 4), reserve=(B, 4), attn=(B, 2), ev=(B, 4), cnt=(B, 4), global_ev=(B,), obj=(B, 4), labels=(B,))
        assert set(shapes) == set(FOCUS_FIELDS)
        for name, shape in shapes.items():
            assert isinstance(getattr(f, name), np.ndarray) and getattr(f, name).shape == shape, (mode, name)
        pred = outs["logits"].argmax(1)
        assert f.classes.tolist() == pred.tolist() and (f.hit[0] == 1).all() and (f.hit[2] == 0).all() and (f.inside[0] == f.total[0]).all()
        if mode == "own":
            assert f.protos.tolist() == [[c * ppc + j for j in range(ppc)] for c in labels]
        else:
            for b in range(B):
                own = np.arange(pred[b] * ppc, pred[b] * ppc + ppc)
                assert f.protos[b].tolist() == own[np.argsort(-outs["act_max"][b, own], kind="stable")][:2].tolist()
        assert (f.cnt.sum(1) == P).all() and (f.reserve[:, 3] == k).all() and f.reserve[0].tolist() == [k * 16, k, G, k]
        local = torch.from_numpy(outs["act_max"]).double() @ (torch.from_numpy(w).double() * float(np.float32(0.5))).t()
        assert np.allclose(f.ev.sum(1), local.numpy()[np.arange(B), pred], rtol=1e-6, atol=1e-5)                  # the four sums are the branch's share of the logit
        assert np.allclose(f.global_ev, 0.5 * outs["logits_global"][np.arange(B), pred].astype(np.float64), rtol=0, atol=0)
    with pytest.raises(ValueError, match="labels are needed"):
        focus_from_outputs(outs, obj, w, 0.5, ppc, k, S, None, "own", device=False)
    with pytest.raises(ValueError, match="'own' or 'top'"):
        focus_from_outputs(outs, obj, w, 0.5, ppc, k, S, labels, "all", device=False)


# ------------------------------------------------------------------------------------------------ the tool
def test_tool_parser_has_the_model_and_data_flags_of_train():
    from protopformer_amd.focus import get_args_parser
    from protopformer_amd.train import get_args_parser as train_parser
    own = {o: a for a in get_args_parser()._actions for o in a.option_strings}
    shared = [(o, a) for a in train_parser()._actions for o in a.option_strings]
    assert len(shared) > 40
    for o, a in shared:
        assert o in own and own[o].dest == a.dest, f"{o} of train.py is missing"
        assert own[o].default == (0 if a.dest == "seed" else a.default), o
    a = get_args_parser().parse_args([])
    assert (a.resume, a.split, a.protos, a.protos_per_image, a.percentile, a.max_images, a.boxes, a.per_image) == ("", "test", "own", 3, 95, 0, "", False)
    a = get_args_parser().parse_args(["--resume", "x.pth", "--split", "train", "--protos", "top", "--protos_per_image", "2", "--percentile", "90",
                                      "--max_images", "5", "--boxes", "b.json", "--per-image", "--output_dir", "o"])
    assert (a.resume, a.split, a.protos, a.protos_per_image, a.percentile, a.max_images, a.boxes, a.per_image, a.output_dir) == (
        "x.pth", "train", "top", 2, 90.0, 5, "b.json", True, "o")
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--protos", "all"])


def test_tool_module_imports_nothing_gpu_related():
    import subprocess
    code = "import sys; import protopformer_amd.focus as f; f.get_args_parser; sys.exit(int('torch' in sys.modules))"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def test_boxes_of_the_miniature_cub_tree(tmp_path):
    import mini_trees
    from protopformer_amd import data as D
    from protopformer_amd.focus import cub_boxes, image_files, read_boxes
    from protopformer_amd.interpret import scaled_boxes
    tree = str(tmp_path / "data")
    meta = mini_trees.build_cub(tree)
    for path in (tree, meta):                                          # --data_path may name either directory
        boxes = cub_boxes(path)
        assert len(boxes) == 25 and boxes[7] == (17, 12, 17 + 74, 12 + 47) and boxes[1] == (11, 6, 11 + 62, 6 + 41)
    ds = D.Cub2011(tree, train=False, transform=None, return_id=True)
    files = image_files(ds)
    assert sorted(files) == sorted(i for i, _, t in mini_trees.CUB_ROWS if t == 0 and i not in mini_trees.CUB_NO_LABEL)
    sizes = {i: mini_trees.cub_size(i) for i in files}
    from PIL import Image
    for i, p in files.items():
        with Image.open(p) as im:
            assert im.size == sizes[i]
    ids = sorted(files)
    got = scaled_boxes(ids, boxes, sizes, 224)
    for row, i in zip(got.tolist(), ids):
        w, h = sizes[i]
        x0, y0, x1, y1 = 10 + i, 5 + i, 10 + i + 60 + 2 * i, 5 + i + 40 + i
        assert row == [224 * y0 // h, min(224, -(-224 * y1 // h)), 224 * x0 // w, min(224, -(-224 * x1 // w))], i
        assert 0 <= row[0] < row[1] <= 224 and 0 <= row[2] < row[3] <= 224
    # a --boxes file for any other set
    path = str(tmp_path / "boxes.json")
    json.dump({"0": [1, 2, 30, 40], "5": [0, 0, 7, 9]}, open(path, "w"))
    assert read_boxes(path) == {0: (1, 2, 30, 40), 5: (0, 0, 7, 9)}
    json.dump({"0": [1, 2, 30]}, open(path, "w"))
    with pytest.raises(ValueError, match="four integers"):
        read_boxes(path)


def test_tool_record_is_plain_json():
    from protopformer_amd.focus import get_args_parser, summarize
    from protopformer_amd.interpret import focus_summary
    res = focus_summary(_rows(), 8, 2)
    res["settings"] = dict(protos="own", protos_per_image=3, percentile=95, img_size=8, patch=2)
    doc = json.loads(json.dumps(summarize(res, get_args_parser().parse_args(["--data_set", "CUB2011U"])), allow_nan=False))
    assert doc["images"] == 7 and doc["rows"] == 14 and doc["settings"]["split"] == "test" and doc["settings"]["boxes"] == "bounding_boxes.txt"
    assert all(isinstance(k, str) for k in doc["per_class"]) and all(isinstance(k, str) for k in doc["per_prototype"])
    assert doc["overall"]["evidence"]["other_inside"] is None and set(doc["overall"]) == {"prototype_maps", "reservation", "evidence"}
