"""PartsWorld without a GPU: the class table, the invariants of the scene table (true by construction: no case is left out), the pixels
of the numpy referee, the plumbing from the train parser to the annotation, and the argument checks of ppf_synth_scene / ppf_synth_render,
which run before any device call."""
import ctypes
import json

import numpy as np
import pytest

from protopformer_amd import data as D

SPECIAL_IDS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3]
FRAMES = [(32, 32), (37, 48), (256, 256)]


def _spec(H=64, W=64, **kw):
    kw = dict(dict(classes=200, parts=8, distractors=8, n_train=64, n_test=32, seed=3, noise=8, grid=4), **kw)
    return D.PartsWorldSpec(height=H, width=W, **kw)


def _prims(scene, at, n):
    """[B, n, 5] = (on, cx, cy, r, attribute) of the parts (at = SYNTH_PART0) or the distractors (at = SYNTH_DIST0)."""
    return scene[:, at:at + D.SYNTH_PRIM_WORDS * n].reshape(len(scene), n, D.SYNTH_PRIM_WORDS).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the class table
@pytest.mark.parametrize("C,K", [(2, 1), (24, 1), (25, 2), (1024, 3)])
def test_class_rows_are_pairwise_distinct(C, K):
    spec = _spec(classes=C, parts=K)
    t = D.partsworld_class_table(spec)
    assert t.shape == (C, K) and t.dtype == np.int32 and t.min() >= 0 and t.max() < D.SYNTH_ATTRS
    assert len({tuple(r) for r in t.tolist()}) == C
    assert np.array_equal(t, D.partsworld_class_table(_spec(32, 48, classes=C, parts=K, seed=99, noise=0)))     # the spec's C and K alone


def test_too_many_classes_are_refused_by_name():
    with pytest.raises(ValueError, match=r"C > A\^K"):
        _spec(classes=25, parts=1)


def test_the_table_is_part_of_the_annotation():
    ds = D.PartsWorld(_spec(classes=30, parts=2), train=False)
    a = ds.annotation()
    assert np.array_equal(a.class_parts, D.partsworld_class_table(ds.spec)) and a.n_parts == 2
    parts = _prims(a.scene, D.SYNTH_PART0, 2)
    assert np.array_equal(parts[:, :, 4], a.class_parts[a.scene[:, 0]])


# ------------------------------------------------------------------------------------------------ the scene
@pytest.fixture(scope="module", params=FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def scenes(request):
    H, W = request.param
    spec = _spec(H, W)
    rng = np.random.default_rng(11)
    ids = np.concatenate([np.array(SPECIAL_IDS, dtype=np.int64), np.arange(2, 1000), rng.integers(0, 1 << 62, 2000 - 998 - len(SPECIAL_IDS))])
    assert len(ids) == 2000
    return spec, ids, D.partsworld_scene_from_ids(spec, ids)


def test_scene_invariants(scenes):
    spec, ids, scene = scenes
    H, W, K = spec.height, spec.width, spec.parts
    assert scene.shape == (2000, D.SYNTH_WORDS) and scene.dtype == np.int32
    assert np.array_equal(scene[:, 0], ids % spec.classes)
    x0, y0, x1, y1 = (scene[:, D.SYNTH_BOX + i].astype(np.int64) for i in range(4))
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x1 <= W).all() and (y1 <= H).all() and (x1 > x0).all() and (y1 > y0).all()
    p = _prims(scene, D.SYNTH_PART0, K)
    on, cx, cy, r = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    assert set(np.unique(on)) <= {0, 1} and (on.sum(axis=1) >= 1).all()
    assert 0 < on.mean() < 1                                                   # and some parts are hidden
    # every part (visible or not) lies inside the box: each shape lies inside the square of its radius
    assert (cx - r >= x0[:, None]).all() and (cx + r < x1[:, None]).all() and (cy - r >= y0[:, None]).all() and (cy + r < y1[:, None]).all()
    assert (r >= 3).all()
    for a in range(K):                                                        # pairwise disjoint: the squares are
        for b in range(a):
            gap_x = np.abs(cx[:, a] - cx[:, b]) - r[:, a] - r[:, b]
            gap_y = np.abs(cy[:, a] - cy[:, b]) - r[:, a] - r[:, b]
            assert ((gap_x > 0) | (gap_y > 0)).all(), (a, b)
    d = _prims(scene, D.SYNTH_DIST0, spec.distractors)
    assert (d[..., 1] - d[..., 3] >= 0).all() and (d[..., 1] + d[..., 3] < W).all() and (d[..., 2] - d[..., 3] >= 0).all() and (d[..., 2] + d[..., 3] < H).all()
    assert (d[..., 4] >= 0).all() and (d[..., 4] < D.SYNTH_ATTRS).all() and 0 < d[..., 0].mean() < 1
    assert (scene[:, D.SYNTH_NODE0 + (spec.grid + 1) ** 2:] == 0).all()


def test_scene_is_a_function_of_the_id(scenes):
    spec, ids, scene = scenes
    pick = np.array([7, 0, 1999, 3, 4])
    assert np.array_equal(D.partsworld_scene_from_ids(spec, ids[pick]), scene[pick])
    other = D.partsworld_scene_from_ids(D.PartsWorldSpec.from_dict(dict(spec.to_dict(), seed=spec.seed + 1)), ids[:50])
    assert not np.array_equal(other[:, 1:], scene[:50, 1:]) and np.array_equal(other[:, 0], scene[:50, 0])
    # the id's high word reaches the draws
    assert not np.array_equal(D.partsworld_scene_from_ids(spec, [5])[0, 1:], D.partsworld_scene_from_ids(spec, [5 + (1 << 32)])[0, 1:])


# ------------------------------------------------------------------------------------------------ the pixels
@pytest.fixture(scope="module", params=[(37, 48), (64, 64)], ids=lambda f: f"{f[0]}x{f[1]}")
def rendered(request):
    H, W = request.param
    spec = _spec(H, W, noise=0, classes=200)
    ids = np.array(SPECIAL_IDS + list(range(30, 41)), dtype=np.int64)
    scene = D.partsworld_scene_from_ids(spec, ids)
    frames, maps = D.partsworld_render(spec, scene, ids, partmap=True)
    return spec, ids, scene, frames, maps


def test_partmap_and_part_colours(rendered):
    spec, ids, scene, frames, maps = rendered
    H, W, K = spec.height, spec.width, spec.parts
    assert frames.shape == (len(ids), H, W, 3) and frames.dtype == np.uint8 and maps.shape == (len(ids), H, W) and maps.dtype == np.uint8
    parts = _prims(scene, D.SYNTH_PART0, K)
    ys, xs = np.mgrid[0:H, 0:W]
    seen_shapes = set()
    for b in range(len(ids)):
        x0, y0, x1, y1 = scene[b, D.SYNTH_BOX:D.SYNTH_BOX + 4]
        outside = ~((xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1))
        assert (maps[b][outside] < 3).all() and (maps[b][~outside] >= 2).all()
        for k, (on, cx, cy, r, attr) in enumerate(parts[b]):
            own = maps[b] == 3 + k
            if not on:
                assert not own.any()
                continue
            assert maps[b, cy, cx] == 3 + k
            assert (frames[b][own] == D.SYNTH_PALETTE[attr % D.SYNTH_COLOURS]).all()
            assert np.array_equal(own, D._synth_inside(attr // D.SYNTH_COLOURS, xs - cx, ys - cy, r))       # nothing covers a part
            seen_shapes.add(int(attr) // D.SYNTH_COLOURS)
        assert (frames[b][maps[b] == 2] == D.SYNTH_BODY).all()
    assert seen_shapes == {0, 1, 2, 3}
    assert (maps == 1).any() and (maps == 0).any()


def test_an_image_alone_equals_the_image_in_a_batch(rendered):
    spec, ids, scene, frames, maps = rendered
    noisy = D.PartsWorldSpec.from_dict(dict(spec.to_dict(), noise=32))
    whole = D.partsworld_render(noisy, scene, ids)
    assert not np.array_equal(whole, frames) and np.abs(whole.astype(int) - frames).max() <= 32
    for b in (0, 3, len(ids) - 1):
        one_f, one_m = D.partsworld_render(noisy, scene[b:b + 1], ids[b:b + 1], partmap=True)
        assert np.array_equal(one_f[0], whole[b]) and np.array_equal(one_m[0], maps[b])
    back = D.partsworld_render(noisy, scene[::-1], ids[::-1])
    assert np.array_equal(back[::-1], whole)


# ------------------------------------------------------------------------------------------------ the plumbing
def test_spec_json_round_trip():
    spec = _spec(37, 48, test_id_base=1 << 33)
    again = D.PartsWorldSpec.from_json(spec.to_json())
    assert again == spec and again.to_dict() == spec.to_dict() and json.loads(spec.to_json())["test_id_base"] == 1 << 33
    d = D.PartsWorldSpec()
    assert (d.classes, d.parts, d.distractors, d.height, d.width, d.n_train, d.n_test, d.test_id_base, d.seed) == (20, 4, 3, 256, 256, 4096, 1024, 1 << 32, 0)
    with pytest.raises(ValueError, match="unknown settings"):
        D.PartsWorldSpec.from_dict(dict(spec.to_dict(), colour=3))
    for bad, word in ((dict(width=40), "multiple of 16"), (dict(height=16), "height"), (dict(parts=9), "parts"), (dict(distractors=9), "distractors"),
                      (dict(noise=33), "noise"), (dict(grid=0), "grid"), (dict(test_id_base=3), "test_id_base")):
        with pytest.raises(ValueError, match=word):
            D.PartsWorldSpec.from_dict(dict(spec.to_dict(), **bad))


def test_parser_and_build_dataset(tmp_path):
    from protopformer_amd.train import get_args_parser
    args = get_args_parser().parse_args(["--data_set", "PartsWorld", "--input_size", "64"])
    assert args.data_set == "PartsWorld" and not hasattr(args, "partsworld")
    ds, nb = D.build_dataset(True, args)                                       # the defaults
    assert isinstance(ds, D.PartsWorld) and nb == 20 and len(ds) == 4096 and ds.spec == D.PartsWorldSpec()
    spec = _spec(classes=4, parts=2, n_train=32, n_test=16)
    path = tmp_path / "world.json"
    path.write_text(spec.to_json())
    args.data_path = str(path)                                                 # a settings file
    ds, nb = D.build_dataset(False, args)
    assert nb == 4 and ds.spec == spec and len(ds) == 16 and not ds.train
    args.partsworld = _spec(classes=5, parts=1, n_train=10, n_test=5)          # a Python caller's spec wins
    ds, nb = D.build_dataset(True, args)
    assert nb == 5 and len(ds) == 10 and ds.ids.tolist() == list(range(10))
    img, label = ds[7]
    assert isinstance(img, np.ndarray) and img.shape == (64, 64, 3) and img.dtype == np.uint8 and label == 7 % 5
    ds.return_id, ds.transform = True, None
    img, label, img_id = ds[3]
    assert img.size == (64, 64) and img_id == 3 and np.array_equal(np.asarray(img), ds.original(3)) and ds.image_size(3) == (64, 64)


def test_annotation_agrees_with_the_scene_and_labels_are_balanced():
    spec = _spec(37, 48, classes=7, parts=3, n_train=100, n_test=30)
    for train in (True, False):
        ds = D.PartsWorld(spec, train=train)
        base = 0 if train else 1 << 32
        assert ds.ids.tolist() == list(range(base, base + len(ds))) and np.array_equal(ds.labels, ds.ids % 7)
        counts = np.bincount(ds.labels, minlength=7)
        assert counts.max() - counts.min() <= 1
        a = ds.annotation()
        scene = D.partsworld_scene_from_ids(spec, ds.ids)
        assert np.array_equal(a.scene, scene) and sorted(a.id_to_bbox) == ds.ids.tolist() and a.part_names == {"1": "part 1", "2": "part 2", "3": "part 3"}
        parts = _prims(scene, D.SYNTH_PART0, 3)
        for i, row, p in zip(ds.ids.tolist(), scene, parts):
            assert a.id_to_bbox[i] == tuple(row[1:5].tolist()) and a.image_sizes[i] == (48, 37)
            assert a.id_to_part_loc[i] == [[k + 1, int(q[1]), int(q[2])] for k, q in enumerate(p) if q[0]] and len(a.id_to_part_loc[i]) >= 1
    from protopformer_amd.interpret import scaled_boxes, scaled_parts                   # the callers' own readers take it
    ids = ds.ids[:5].tolist()
    assert scaled_boxes(ids, a.id_to_bbox, a.image_sizes, 64).shape == (5, 4)
    labels, masks = scaled_parts(ids, a, a.image_sizes, 64, a.n_parts)
    assert masks.shape == (5, 3) and all(0 <= pid0 < 3 and 0 <= x < 64 and 0 <= y < 64 for image in labels for pid0, x, y in image)


def test_bank_index_names_the_rendered_images():
    from protopformer_amd.bank import image_index
    ds = D.PartsWorld(_spec(classes=4, parts=1, n_train=8, n_test=4), train=False)
    index = image_index(ds)
    assert index[(1 << 32) + 1] == (f"partsworld:{(1 << 32) + 1}", 1) and len(index) == 4


# ------------------------------------------------------------------------------------------------ the error channel
@pytest.fixture(scope="module")
def lib():
    from protopformer_amd import _lib
    from protopformer_amd.build import build
    build(verbose=False)
    return _lib.lib()


OK = dict(B=2, C=20, K=4, D=3, H=64, W=64, g=4, noise=8)
REFUSED = [(dict(W=40), "W=40", "multiple of 16"), (dict(H=16), "H=16", "outside"), (dict(H=2000), "H=2000", "outside"), (dict(W=16), "W=16", "outside"),
           (dict(W=1040), "W=1040", "outside"), (dict(K=9), "K=9", "parts"), (dict(D=9), "D=9", "distractors"), (dict(C=25, K=1), "C=25", "A^K"),
           (dict(B=0), "B=0", ">= 1")]


@pytest.mark.parametrize("change,name,word", REFUSED, ids=[r[1] for r in REFUSED])
def test_refused_arguments_without_a_gpu(lib, change, name, word):
    a = dict(OK, **change)
    calls = (("scene", lambda: lib.ppf_synth_scene(None, None, a["B"], a["C"], a["K"], a["D"], a["H"], a["W"], a["g"], a["noise"], 0, None)),
             ("render", lambda: lib.ppf_synth_render(None, None, None, None, a["B"], a["H"], a["W"], a["C"], a["K"], a["D"], a["g"], a["noise"], 0, None)))
    for fn, call in calls:
        rc = call()
        msg = lib.ppf_last_error().decode()
        assert rc == -1 and name in msg and word in msg and msg.startswith("ppf_synth_" + fn), (fn, rc, msg)


@pytest.mark.parametrize("out,partmap", [(8, 0), (4096, 4100)], ids=["out", "partmap"])
def test_refused_alignment_without_a_gpu(lib, out, partmap):
    a = OK
    rc = lib.ppf_synth_render(ctypes.c_void_p(out), ctypes.c_void_p(partmap), None, None, a["B"], a["H"], a["W"], a["C"], a["K"], a["D"], a["g"], a["noise"],
                              0, None)
    assert rc == -1 and "16-byte aligned" in lib.ppf_last_error().decode()
    assert lib.ppf_synth_render(ctypes.c_void_p(4096), None, None, None, a["B"], a["H"], a["W"], a["C"], a["K"], a["D"], a["g"], a["noise"], 0, None) == -3
    assert "null pointer" in lib.ppf_last_error().decode()


def test_wrappers_refuse_what_the_c_side_cannot_see():
    import torch
    from protopformer_amd import ops
    spec = _spec()
    with pytest.raises(ValueError, match="ids must be"):
        ops.synth_scene(spec, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="ids must be"):
        ops.synth_render(spec, torch.zeros((3, D.SYNTH_WORDS), dtype=torch.int32), torch.zeros((3, 1), dtype=torch.int64))
    with pytest.raises(ValueError, match=">= 0"):
        D.partsworld_scene_from_ids(spec, [-1])
    assert ops.SYNTH_WORDS == D.SYNTH_WORDS
