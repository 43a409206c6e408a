"""Part interventions without a GPU: the numpy referee of ppf_synth_edit (every op, the 0 and -1 rules, and that a rendered PARTS_OFF row
differs from the unedited frame only inside the part's square), the view rule on the world the GPU tests use, the part_mass referee
against math.fsum with its NaN / inf / -0 rules, the arithmetic of part_agreement_from_rows against hand-worked cases, and the parser."""
import math

import numpy as np
import pytest

from protopformer_amd import data as D
from protopformer_amd import interpret as I

WORLD = dict(classes=4, parts=4, distractors=3, n_train=32, n_test=12, seed=5, noise=8, grid=4)


@pytest.fixture(scope="module")
def world():
    spec = D.PartsWorldSpec(height=80, width=96, **WORLD)
    ids = spec.test_id_base + np.arange(spec.n_test, dtype=np.int64)
    scene = D.partsworld_scene_from_ids(spec, ids)
    frames, maps = D.partsworld_render(spec, scene, ids, partmap=True)
    return spec, ids, scene, frames, maps


def _part(row, k, field=0):
    return row[D.SYNTH_PART0 + D.SYNTH_PRIM_WORDS * k + field]


# ------------------------------------------------------------------------------------------------ the referee of ppf_synth_edit
def test_edit_referee_every_op(world):
    spec, ids, scene, _, _ = world
    K, Dn, nodes = spec.parts, spec.distractors, (spec.grid + 1) ** 2
    b = 0                                                                      # image 0 shows all four parts
    vis = [k for k in range(K) if _part(scene[b], k)]
    assert vis == [0, 1, 2, 3]
    attr1 = int(_part(scene[b], 1, 4))
    edits = [(D.EDIT_COPY, 0), (D.EDIT_PARTS_OFF, 0b0101), (D.EDIT_DISTRACTORS_OFF, (1 << Dn) - 1), (D.EDIT_BACKGROUND, 0x808080),
             (D.EDIT_PART_ATTR, 1 | ((attr1 + 5) % 24) << 8), (D.EDIT_PART_ATTR, 1 | attr1 << 8), (D.EDIT_PARTS_OFF, 0)]
    e = np.tile(np.array(edits, dtype=np.int32)[None], (len(ids), 1, 1))
    out, changed = D.partsworld_edit(spec, scene, e)
    assert out.shape == (len(ids), len(edits), D.SYNTH_WORDS) and out.dtype == np.int32 and changed.shape == (len(ids), len(edits))
    row = scene[b]
    assert np.array_equal(out[b, 0], row) and changed[b, 0] == 0
    want = row.copy(); want[D.SYNTH_PART0] = 0; want[D.SYNTH_PART0 + 10] = 0
    assert np.array_equal(out[b, 1], want) and changed[b, 1] == 1
    want = row.copy(); want[D.SYNTH_DIST0:D.SYNTH_DIST0 + 5 * Dn:5] = 0
    assert np.array_equal(out[b, 2], want) and changed[b, 2] == int(row[D.SYNTH_DIST0:D.SYNTH_DIST0 + 5 * Dn:5].any())
    want = row.copy(); want[D.SYNTH_NODE0:D.SYNTH_NODE0 + nodes] = 0x808080
    assert np.array_equal(out[b, 3], want) and changed[b, 3] == 1 and (out[b, 3][D.SYNTH_NODE0 + nodes:] == 0).all()
    want = row.copy(); want[D.SYNTH_PART0 + 5 + 4] = (attr1 + 5) % 24
    assert np.array_equal(out[b, 4], want) and changed[b, 4] == 1
    assert np.array_equal(out[b, 5], row) and changed[b, 5] == 0               # an attribute set to its own value
    assert np.array_equal(out[b, 6], row) and changed[b, 6] == 0               # an empty mask
    # an edit list is applied to the same row, edit by edit: nothing of edit 1 is in edit 2
    assert _part(out[b, 2], 0) == 1


def test_edit_referee_changed_is_zero_for_what_is_not_drawn(world):
    spec, ids, scene, _, _ = world
    b = 4                                                                      # one visible part
    vis = [k for k in range(4) if _part(scene[b], k)]
    assert len(vis) == 1
    hidden = [k for k in range(4) if k not in vis]
    edits = [(D.EDIT_PARTS_OFF, 1 << k) for k in hidden] + [(D.EDIT_PART_ATTR, k | ((int(_part(scene[b], k, 4)) + 1) % 24) << 8) for k in hidden]
    edits += [(D.EDIT_PARTS_OFF, sum(1 << k for k in hidden)), (D.EDIT_PARTS_OFF, 0xF)]
    out, changed = D.partsworld_edit(spec, scene[b:b + 1], np.array(edits, dtype=np.int32)[None])
    assert changed[0].tolist() == [0] * 7 + [1]
    assert _part(out[0, 3], hidden[0], 4) == (int(_part(scene[b], hidden[0], 4)) + 1) % 24      # written all the same


def test_edit_referee_invalid_edits_copy_the_row(world):
    spec, ids, scene, _, _ = world
    bad = [(5, 0), (-1, 0), (99, 3), (D.EDIT_PARTS_OFF, 1 << 4), (D.EDIT_PARTS_OFF, -1), (D.EDIT_DISTRACTORS_OFF, 1 << 3), (D.EDIT_PART_ATTR, 4 | 1 << 8),
           (D.EDIT_PART_ATTR, 0 | 24 << 8), (D.EDIT_PART_ATTR, -3), (D.EDIT_BACKGROUND, 0x1000000), (D.EDIT_BACKGROUND, -1)]
    out, changed = D.partsworld_edit(spec, scene[:2], np.tile(np.array(bad, dtype=np.int32)[None], (2, 1, 1)))
    assert (changed == -1).all()
    assert np.array_equal(out, np.repeat(scene[:2, None], len(bad), axis=1))
    with pytest.raises(ValueError, match="edits"):
        D.partsworld_edit(spec, scene[:2], np.zeros((3, 1, 2), dtype=np.int32))


def test_rendering_a_hidden_part_touches_its_square_only(world):
    spec, ids, scene, frames, maps = world
    for b, k in ((0, 0), (0, 3), (5, 2)):
        assert _part(scene[b], k) == 1
        out, changed = D.partsworld_edit(spec, scene[b:b + 1], np.array([[[D.EDIT_PARTS_OFF, 1 << k]]], dtype=np.int32))
        assert changed[0, 0] == 1
        f, m = D.partsworld_render(spec, out[0], ids[b:b + 1], partmap=True)
        cx, cy, r = (int(_part(scene[b], k, j)) for j in (1, 2, 3))
        ys, xs = np.mgrid[0:spec.height, 0:spec.width]
        outside = (np.abs(xs - cx) > r) | (np.abs(ys - cy) > r)
        assert np.array_equal(f[0][outside], frames[b][outside]) and not np.array_equal(f[0], frames[b])      # noise included
        assert (maps[b] == 3 + k).any() and not (m[0] == 3 + k).any()
        before, after = np.bincount(maps[b].reshape(-1), minlength=7), np.bincount(m[0].reshape(-1), minlength=7)
        assert all(after[c] >= before[c] for c in range(7) if c != 3 + k)


# ------------------------------------------------------------------------------------------------ the view rule
def test_view_rule_on_the_gpu_tests_world(world):
    spec, ids, scene, frames, maps = world
    S, K = 64, spec.parts
    src = D.partsworld_view_src(np.arange(S), 80, S)
    assert src[0] == 0 and src[-1] == 79 and (np.diff(src) >= 1).all() and src.dtype == np.int64
    assert D.partsworld_view_src(0, 1, 7) == 0 and D.partsworld_view_src(6, 1, 7) == 0 and D.partsworld_view_src(3, 7, 7) == 3
    view = D.partsworld_view_partmap(maps, S)
    assert view.shape == (12, S, S) and view.dtype == np.uint8
    assert view[3, 10, 20] == maps[3, (21 * 80) // 128, (41 * 96) // 128]
    visible = np.array([[int(_part(scene[b], k)) for k in range(K)] for b in range(12)])
    assert visible.sum(1).tolist() == [4, 3, 3, 3, 1, 4, 3, 3, 3, 3, 4, 4]
    counts = np.array([[int((view[b] == 3 + k).sum()) for k in range(K)] for b in range(12)])
    assert ((counts > 0) == (visible == 1)).all()                              # every visible part is in the view, no invisible one is
    on = scene[:, D.SYNTH_DIST0:D.SYNTH_DIST0 + 5 * spec.distractors:5]
    assert [b for b in range(12) if not (view[b] == 1).any()] == [9, 11] and not (maps[9] == 1).any() and not (maps[11] == 1).any()
    assert on[9].sum() == 0 and on[11].sum() == 2
    out, changed = D.partsworld_edit(spec, scene[[9, 11]], np.tile(np.array([[[D.EDIT_DISTRACTORS_OFF, 7]]], dtype=np.int32), (2, 1, 1)))
    assert changed[:, 0].tolist() == [0, 1]                                    # image 11: both under the body, so the pixels are equal
    assert np.array_equal(D.partsworld_render(spec, out[1], ids[11:12])[0], frames[11])


# ------------------------------------------------------------------------------------------------ the referee of ppf_part_mass
def _fsum_bins(score, codes, nb):
    pos, neg, cnt = np.zeros(nb), np.zeros(nb), np.zeros(nb, dtype=np.int64)
    for c in range(nb):
        v = [float(x) for x in score[codes == c] if math.isfinite(x)]
        pos[c], neg[c], cnt[c] = math.fsum(x for x in v if x > 0), math.fsum(-x for x in v if x < 0), int((codes == c).sum())
    return pos, neg, cnt


def test_part_mass_referee_against_fsum(world):
    spec, ids, scene, frames, maps = world
    rng = np.random.default_rng(0)
    S, K, M = 20, spec.parts, 2
    score = (rng.standard_normal((3 * M, S, S)) * np.exp(rng.uniform(-8, 8, (3 * M, S, S)))).astype(np.float32)
    score[1, 0, :4] = [np.nan, np.inf, -np.inf, -0.0]
    pos, neg, count, bad = I.part_mass(score, maps[:3], M, K, device=False)
    assert pos.shape == (6, 3 + K) and pos.dtype == np.float64 and count.dtype == np.int32 and bad.tolist() == [0, 3, 0, 0, 0, 0]
    view = D.partsworld_view_partmap(maps[:3], S)
    for r in range(6):
        p, n, c = _fsum_bins(score[r], view[r // M], 3 + K)
        assert np.array_equal(count[r], c) and count[r].sum() == S * S
        total = np.abs(np.where(np.isfinite(score[r]), score[r], 0).astype(np.float64))
        for b in range(3 + K):
            bound = c[b] * 2.0 ** -53 * total[view[r // M] == b].sum()
            assert abs(pos[r, b] - p[b]) <= bound and abs(neg[r, b] - n[b]) <= bound
    assert (pos >= 0).all() and (neg >= 0).all() and not np.signbit(pos).any() and not np.signbit(neg).any()


def test_part_mass_referee_rules():
    maps = np.zeros((1, 4, 4), dtype=np.uint8)
    maps[0, 0, 0], maps[0, 3, 3], maps[0, 1, 1] = 3, 4, 9                      # code 9 > 2 + K for K = 2
    score = np.full((1, 4, 4), np.nan, dtype=np.float32)
    pos, neg, count, bad = I.part_mass(score, maps, 1, 2, device=False)
    assert not pos.any() and not neg.any() and bad.tolist() == [16] and count[0].tolist() == [13, 0, 0, 1, 1]
    score = np.ones((1, 4, 4), dtype=np.float32)
    score[0, 0, 0], score[0, 3, 3], score[0, 1, 1] = -2.5, -0.0, 7.0
    pos, neg, count, bad = I.part_mass(score, maps, 1, 2, device=False)
    assert pos[0].tolist() == [13.0, 0, 0, 0, 0] and neg[0].tolist() == [0, 0, 0, 2.5, 0] and bad.tolist() == [1] and count[0].sum() == 15
    with pytest.raises(ValueError, match="rows_per_img"):
        I.part_mass(np.zeros((3, 4, 4), dtype=np.float32), maps, 2, 2, device=False)


# ------------------------------------------------------------------------------------------------ part_agreement_from_rows
def test_spearman_hand_worked():
    assert I.spearman([1, 2, 3, 4], [10, 20, 30, 40]) == pytest.approx(1.0, abs=1e-15)
    assert I.spearman([1, 2, 3, 4], [4, 3, 2, 1]) == pytest.approx(-1.0, abs=1e-15)
    assert I._avg_ranks([10, 20, 20, 30]).tolist() == [1.0, 2.5, 2.5, 4.0]
    # ranks (1, 2.5, 2.5, 4) against (1, 2, 3, 4): cov = 4.5, var = 4.5 and 5
    assert I.spearman([10, 20, 20, 30], [1, 2, 3, 4]) == pytest.approx(4.5 / math.sqrt(4.5 * 5.0), abs=1e-15)
    assert I.spearman([1, 3, 2], [1, 2, 3]) == pytest.approx(0.5, abs=1e-15)
    assert I.spearman([5, 5, 5], [1, 2, 3]) is None and I.spearman([1, 2, 3], [0, 0, 0]) is None and I.spearman([1], [2]) is None


def _rows(N=5, K=3, seed=1):
    rng = np.random.default_rng(seed)
    E, nb = K + 5, 3 + K
    visible = np.ones((N, K), dtype=np.int32)
    visible[1, 1:] = 0                                                         # image 1 shows one part: undefined
    changed = np.ones((N, E), dtype=np.int32)
    changed[:, 0] = 0
    changed[:, 1:K + 1] = visible
    value = rng.uniform(0.1, 0.9, (N, E)).astype(np.float32)
    labels = np.arange(N) % 4
    pred = np.tile(labels[:, None], (1, E)).astype(np.int32)
    pred[:, K + 4] = (labels + 1) % 4
    pred[2, K + 4] = labels[2]
    pred[3, K + 2] = (labels[3] + 2) % 4

    def order():
        return dict(pos=rng.uniform(0, 5, (N, nb)), neg=rng.uniform(0, 1, (N, nb)), count=np.tile(np.array([[60, 4, 24] + [4] * K]), (N, 1)).astype(np.int32),
                    nonfinite=np.zeros(N, dtype=np.int32), deleted=rng.uniform(0, 1, (N, K)).astype(np.float32))
    return dict(image_ids=np.array([7, 3, 11, 5, 9][:N], dtype=np.int64), labels=labels, value=value, pred=pred, changed=changed, visible=visible,
                class_parts=np.array([[c, 0, 0][:K] for c in range(4)]), view=10, oracle=rng.uniform(0, 1, (N, K)).astype(np.float32),
                reverse=rng.uniform(0, 1, (N, K)).astype(np.float32), orders=dict(a=order(), b=order()))


def test_agreement_arithmetic():
    rows = _rows()
    K, N = 3, 5
    out = I.part_agreement_from_rows(rows)
    assert out["images"] == N and out["parts"] == K and set(out["per_order"]) == {"a", "b"}
    m, v = out["model"], rows["value"].astype(np.float64)
    assert m["discriminative_parts"] == [0] and m["importance_images"] == [5, 4, 4]
    by_id = np.argsort(rows["image_ids"])
    assert m["importance"][0] == pytest.approx(float(np.mean((v[:, 0] - v[:, 1])[by_id])), abs=1e-15)
    keep = [i for i in by_id if i != 1]
    assert m["importance"][1] == pytest.approx(float(np.mean((v[:, 0] - v[:, 2])[keep])), abs=1e-15)
    assert m["parts_share"] == pytest.approx(float(np.mean(((v[:, 0] - v[:, K + 1]) / v[:, 0])[by_id])), abs=1e-15)
    assert m["distractor_effect"] == pytest.approx(float(np.mean(np.abs(v[:, 0] - v[:, K + 2])[by_id])), abs=1e-15)
    assert m["distractor_changes_prediction"] == pytest.approx(0.2) and m["background_changes_prediction"] == 0.0
    assert m["counterfactual_images"] == 5 and m["counterfactual_follows"] == pytest.approx(0.8)
    a = out["per_order"]["a"]
    assert a["undefined"] == 1 and a["defined"] == 4
    f = rows["orders"]["a"]
    signed, imp = f["pos"][:, 3:] - f["neg"][:, 3:], v[:, :1] - v[:, 1:K + 1]
    rho = [I.spearman(signed[i], imp[i]) for i in by_id if i != 1]
    assert a["single_deletion"] == pytest.approx(float(np.mean(rho)), abs=1e-15)
    match = [int(np.argmax(signed[i][:1 if i == 1 else K]) == np.argmax(imp[i][:1 if i == 1 else K])) for i in by_id]
    assert a["top_part_match"] == pytest.approx(float(np.mean(match)), abs=1e-15)
    assert a["area_share"] == dict(parts=0.12, body=0.24, distractors=0.04, background=0.6)
    assert sum(a["mass_share"].values()) == pytest.approx(1.0, abs=1e-12) and a["distractor_mass"] == a["mass_share"]["distractors"]
    # the areas: V + 1 values over j / V
    def area(dv):
        per = []
        for i in by_id:
            V = 1 if i == 1 else K
            c = np.concatenate([[v[i, 0]], dv[i, :V].astype(np.float64)])
            per.append(((c[1:] + c[:-1]) / 2).sum() / V)
        return float(np.mean(per))
    pd = a["part_deletion"]
    assert pd["order"] == pytest.approx(area(f["deleted"]), abs=1e-15) and pd["oracle"] == pytest.approx(area(rows["oracle"]), abs=1e-15)
    assert pd["normalised"] == pytest.approx((pd["reverse"] - pd["order"]) / (pd["reverse"] - pd["oracle"]), abs=1e-15)


def test_agreement_normalisation_is_null_when_oracle_equals_reverse():
    rows = _rows()
    rows["reverse"] = rows["oracle"].copy()
    out = I.part_agreement_from_rows(rows)
    assert out["per_order"]["a"]["part_deletion"]["normalised"] is None and out["per_order"]["a"]["part_deletion"]["order"] is not None


def test_agreement_does_not_depend_on_the_row_order():
    rows = _rows()
    perm = np.array([3, 0, 4, 2, 1])
    shuffled = {k: (v[perm] if isinstance(v, np.ndarray) and k != "class_parts" else v) for k, v in rows.items()}
    shuffled["orders"] = {o: {k: v[perm] for k, v in f.items()} for o, f in rows["orders"].items()}
    assert I.part_agreement_from_rows(shuffled) == I.part_agreement_from_rows(rows)


def test_ties_go_to_the_smaller_part():
    assert I._descending([1.0, 3.0, 3.0, 2.0], np.array([True, True, True, True])).tolist() == [1, 2, 3, 0]
    assert I._descending([1.0, 3.0, 3.0, 2.0], np.array([True, False, True, True])).tolist() == [2, 3, 0]


def test_standard_edits():
    spec = D.PartsWorldSpec(**WORLD)
    e = I.standard_edits(spec)
    assert len(e) == spec.parts + 4 and e[0] == (0, 0) and e[1:5] == [(1, 1), (1, 2), (1, 4), (1, 8)] and e[5:] == [(1, 15), (2, 7), (3, 0x808080)]


# ------------------------------------------------------------------------------------------------ the tool's parser
def test_parser_builds_without_a_gpu_and_refuses_other_sets():
    from protopformer_amd import partcheck as tool
    args = tool.get_args_parser().parse_args(["--data_set", "PartsWorld", "--output_dir", "x", "--orders", "evidence", "ig", "--per-image", "--value", "logit"])
    assert args.orders == ["evidence", "ig"] and args.per_image and args.value == "logit" and args.pass_images == 16 and args.split == "test"
    assert tool.check_args(args) is args
    assert tool.get_args_parser().parse_args(["--output_dir", "x"]).orders == ["evidence", "attention", "random"]
    other = tool.get_args_parser().parse_args(["--data_set", "CUB2011U", "--output_dir", "x"])
    with pytest.raises(ValueError, match="CUB2011U"):
        tool.check_args(other)
    with pytest.raises(ValueError, match="CUB2011U"):
        tool.main(other)
    with pytest.raises(SystemExit):
        tool.get_args_parser().parse_args(["--orders", "shap"])
