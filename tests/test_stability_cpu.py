"""Host side of the stability score (interpret.stability_from_outputs, the arithmetic of PartMeter.result, the interp_eval parser):
no GPU needed."""
import types

import numpy as np
import pytest
import torch

from protopformer_amd import interpret as I


def hot(cells, g=4):
    """(len(cells), g, g) maps with one hot cell each."""
    m = np.zeros((len(cells), g, g), dtype=np.float32)
    for p, (y, x) in enumerate(cells):
        m[p, y, x] = 5.0
    return m


def test_stability_by_hand():
    """1 class, 2 images, 2 prototypes, 4 x 4 maps up-sampled to 64 x 64 (one cell = 16 pixels, the peak of a single hot cell lies inside
    it), boxes of half-width 8, one part at pixel (8, 8) = inside cell (0, 0).
    Prototype 0 sits on cell (0, 0) in every pass: its row is (1,) clean and noisy in both images -> stable fraction 1.0.
    Prototype 1 sits on cell (0, 0) in the clean pass; the noise leaves it there in image 0 and moves it across the part to cell (3, 3)
    in image 1 (row (1,) -> (0,)) -> stable fraction 0.5.  Score = (1.0 + 0.5) / 2."""
    acts = np.stack([hot([(0, 0), (0, 0)]), hot([(0, 0), (0, 0)])])
    acts_noisy = np.stack([hot([(0, 0), (0, 0)]), hot([(0, 0), (3, 3)])])
    attn = np.zeros((2, 16), dtype=np.float32)                       # k = 16 = every token: no expansion
    parts = types.SimpleNamespace(id_to_part_loc={7: [[1, 8.0, 8.0]], 9: [[1, 8.0, 8.0]]})
    sizes = {7: (64, 64), 9: (64, 64)}
    targets, ids = np.array([0, 0]), np.array([7, 9])
    # the tables themselves, so that the fractions below are not right for a wrong reason
    clean = I._host_tables(acts, ids, parts, sizes, 64, 8, 1)[0]
    noisy = I._host_tables(acts_noisy, ids, parts, sizes, 64, 8, 1)[0]
    assert clean.reshape(2, 2).tolist() == [[1, 1], [1, 1]] and noisy.reshape(2, 2).tolist() == [[1, 1], [1, 0]]
    score, fraction = I.stability_from_outputs(attn, acts, attn, acts_noisy, targets, ids, parts, sizes, 16, 64, num_classes=1, half_size=8, n_parts=1)
    assert fraction == [1.0, 0.5] and score == 0.75
    # a class without an image is skipped, not counted as unstable
    score3, fraction3 = I.stability_from_outputs(attn, acts, attn, acts_noisy, targets + 1, ids, parts, sizes, 16, 64, num_classes=3, half_size=8,
                                                 n_parts=1)
    assert fraction3 == [1.0, 0.5] and score3 == 0.75


def test_stability_compares_whole_rows():
    """Rows that differ in one of several parts are different rows."""
    clean = np.array([[[1, 0, 1]], [[1, 0, 1]], [[0, 0, 0]]])
    noisy = np.array([[[1, 0, 1]], [[1, 1, 1]], [[0, 0, 0]]])
    score, fraction = I.stability_from_tables(clean, noisy, np.array([0, 0, 2]), 3)
    assert fraction == [0.5, 1.0] and score == 0.75
    assert I.stability_from_tables(clean[:0], noisy[:0], np.zeros(0, dtype=np.int64), 3) == (0.0, [])


def counts():
    """3 classes x 2 prototypes x 3 parts; class 1 has no image."""
    hits = np.zeros((3, 2, 3), dtype=np.int32)
    visible = np.zeros((3, 3), dtype=np.int32)
    hits[0] = [[4, 0, 1], [3, 0, 0]]; visible[0] = [5, 0, 2]          # 4/5 = 0.8 -> consistent; 3/5 -> not; part 1 never visible: 0 / 1
    hits[2] = [[0, 0, 0], [2, 1, 7]]; visible[2] = [3, 1, 9]          # nothing; 1/1 -> consistent
    stable = np.array([[5, 2], [0, 0], [0, 9]], dtype=np.int32)
    images = np.array([5, 0, 9], dtype=np.int32)
    return hits, visible, stable, images


def test_part_meter_scores_arithmetic():
    hits, visible, stable, images = counts()
    r = I.part_meter_scores(hits, visible, stable, images, part_thresh=0.8)
    assert r["effects"] == [1, 0, 0, 1] and r["consistency"] == 0.5
    assert r["max_parts"] == [4 / 5, 3 / 5, 0.0, 1.0]
    assert r["stable_fraction"] == [1.0, 2 / 5, 0.0, 1.0] and r["stability"] == np.mean([1.0, 2 / 5, 0.0, 1.0])
    assert r["images"] == [5, 0, 9]
    # the same numbers as consistency_from_tables on per-image tables with these sums
    tables = np.zeros((5, 2, 3)); masks = np.zeros((5, 3))
    masks[:, 0] = 1; masks[:2, 2] = 1
    tables[:4, 0, 0] = 1; tables[0, 0, 2] = 1; tables[:3, 1, 0] = 1
    e, m = I.consistency_from_tables(tables, masks, 0.8)
    assert e == r["effects"][:2] and m == r["max_parts"][:2]
    assert I.part_meter_scores(hits, visible, stable, images, part_thresh=0.81)["effects"] == [0, 0, 0, 1]
    none = I.part_meter_scores(hits, visible, stable, images, with_stability=False)
    assert none["stability"] is None and none["stable_fraction"] is None and none["consistency"] == 0.5
    empty = I.part_meter_scores(hits * 0, visible * 0, stable * 0, images * 0)
    assert empty["consistency"] == 0.0 and empty["stability"] == 0.0 and empty["effects"] == []


def test_part_meter_result_on_cpu_accumulators():
    """PartMeter holds its five arrays in one int32 buffer; filled by hand on the CPU, result() is part_meter_scores of them."""
    hits, visible, stable, images = counts()
    m = I.PartMeter(3, 2, 3, "cpu")
    assert m.result()["stability"] is None and m.result()["effects"] == []
    m.hits.copy_(torch.from_numpy(hits)); m.visible.copy_(torch.from_numpy(visible)); m.images.copy_(torch.from_numpy(images))
    r = m.result()
    assert r["stability"] is None and r["stable_fraction"] is None and r["effects"] == [1, 0, 0, 1]
    m.stable.copy_(torch.from_numpy(stable)); m.noisy = True
    assert m.result() == I.part_meter_scores(hits, visible, stable, images)
    m.bad += 2
    with pytest.raises(ValueError, match=r"2 labels lie outside \[0, 3\)"):
        m.result()
    m.reset()
    assert int(m.buf.abs().sum()) == 0 and m.noisy is None and m.result()["images"] == [0, 0, 0]


REFERENCE_FLAGS = dict(gpuid=(str, "0"), data_path=(str, None), imgclass=(int, [15]), out_dir=(str, None), batch_size=(int, None),
                       check_test=(None, False), data_set=(str, "CUB2011U"), base_architecture=(str, "vgg16"), input_size=(int, 224),
                       prototype_shape=(int, [2000, 64, 1, 1]), prototype_activation_function=(str, "log"), add_on_layers_type=(str, "regular"),
                       reserve_layers=(int, []), reserve_token_nums=(int, []), use_global=(None, False), use_ppc_loss=(None, False),
                       ppc_cov_thresh=(float, 1.0), ppc_mean_thresh=(float, 2.0), global_coe=(float, 0.5), global_proto_per_class=(int, 5),
                       resume=(str, None))


def test_interp_eval_parser_has_the_reference_flags_and_ours():
    from protopformer_amd import interp_eval
    p = interp_eval.get_args_parser()
    actions = {a.dest: a for a in p._actions}
    d = p.parse_args([])
    for name, (typ, default) in REFERENCE_FLAGS.items():
        assert "--" + name in actions[name].option_strings, name
        assert getattr(d, name) == default, name
        if typ is not None:
            assert actions[name].type is typ, name
    assert actions["imgclass"].nargs == 1 and actions["prototype_shape"].nargs == "+" and actions["reserve_layers"].nargs == "+"
    assert (d.no_stability, d.noise_std, d.noise_seed, d.host) == (False, 0.2, 0, False)
    a = p.parse_args("--no-stability --noise_std 0.1 --noise_seed 7 --host --use_global True --check_test no --prototype_shape 20 32 1 1 "
                     "--reserve_token_nums 81 --batch_size 64".split())
    assert (a.no_stability, a.noise_std, a.noise_seed, a.host, a.use_global, a.check_test) == (True, 0.1, 7, True, True, False)
    assert a.prototype_shape == [20, 32, 1, 1] and a.reserve_token_nums == [81] and a.batch_size == 64
    with pytest.raises(SystemExit):
        p.parse_args(["--use_global", "maybe"])
    doc = interp_eval.report(dict(consistency=0.5, stability=None, effects=[1, 0], max_parts=[1.0, 0.2], stable_fraction=None), 12, a)
    assert doc["images"] == 12 and doc["noise_std"] == 0.1 and doc["noise_seed"] == 7 and doc["path"] == "host" and not doc["stability_computed"]
    src = open(interp_eval.__file__).read().split("def str2bool")[0]                 # the module level: nothing GPU-related is imported there
    assert "import torch" not in src and "from ." not in src


def test_cub_dirs_accepts_either_directory(tmp_path):
    from protopformer_amd.interp_eval import cub_dirs
    inner = tmp_path / "CUB_200_2011"
    inner.mkdir()
    assert cub_dirs(str(tmp_path)) == (str(tmp_path), str(inner)) == cub_dirs(str(inner))
