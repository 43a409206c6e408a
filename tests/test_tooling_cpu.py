"""protopformer_amd.tooling: what the command-line tools set up alike -- the "stop after N images" iteration with and without image
ids, the one host read, and the model built from the training flags; with them PPNet.eval_mode and the source rules of the forward's
named record.  No GPU: list "loaders", CPU tensors and CPU construction only."""
import pytest
import torch

from protopformer_amd import tooling as T


def _loader(width):
    """Three batches of 4 images; `width` elements per batch tuple: (x,), or (x, y, ids) with ids a list as a collate may leave it."""
    x = torch.arange(12.0).reshape(12, 1)
    full = [(x[i:i + 4], x[i:i + 4, 0].long() * 10, list(range(100 + i, 104 + i))) for i in range(0, 12, 4)]
    return [b[:width] for b in full]


@pytest.mark.parametrize("width", [3, 1])
@pytest.mark.parametrize("max_images, sizes", [(0, [4, 4, 4]), (None, [4, 4, 4]), (3, [3]), (4, [4]), (6, [4, 2]), (100, [4, 4, 4])])
def test_take_images_counts_truncates_every_element_and_stops(width, max_images, sizes):
    loader = _loader(width)
    pulled = []

    def counting():
        for b in loader:
            pulled.append(1)
            yield b

    got = list(T.take_images(counting(), max_images))
    assert [len(b) for b in got] == [width] * len(sizes)
    assert [b[0].shape[0] for b in got] == sizes
    n = sum(sizes)
    assert torch.equal(torch.cat([b[0] for b in got]), torch.arange(float(n)).reshape(n, 1))
    for b in got:                                                   # every element of a batch is cut to the same images
        if width == 3:
            assert b[1].tolist() == [int(v) * 10 for v in b[0][:, 0]] and list(b[2]) == [100 + int(v) for v in b[0][:, 0]]
    assert len(pulled) == len(sizes)                                # nothing is pulled after the batch that reaches the count


def test_regroup_over_take_images():
    x = torch.arange(14.0).reshape(14, 1)
    loader = [(x[i:i + 4], None) for i in range(0, 14, 4)]                 # composed as spatial_alignment composes it
    passes = [p for p, in T.regroup(((v.float(),) for v, in T.take_images(((b[0],) for b in loader), 10)), 3)]
    assert [p.shape[0] for p in passes] == [3, 3, 3, 1]
    assert torch.equal(torch.cat(passes), x[:10]) and all(p.dtype == torch.float32 and p.is_contiguous() for p in passes)


@pytest.mark.parametrize("width", [3, 2])
@pytest.mark.parametrize("max_images, sizes", [(0, [4, 4, 4]), (6, [4, 2]), (3, [3])])
def test_batches_with_ids_takes_or_counts_the_ids(width, max_images, sizes):
    loader = _loader(width)
    pulled = []

    def counting():
        for b in loader:
            pulled.append(1)
            yield b

    got = list(T.batches_with_ids(counting(), max_images))
    n = sum(sizes)
    assert all(len(b) == 3 for b in got) and [b[0].shape[0] for b in got] == sizes and len(pulled) == len(sizes)
    assert torch.equal(torch.cat([b[0] for b in got]), torch.arange(float(n)).reshape(n, 1))
    assert torch.cat([b[1] for b in got]).tolist() == [10 * i for i in range(n)]                 # the last batch is cut in every element
    ids = torch.cat([b[2] for b in got])
    assert all(b[2].dtype == torch.int64 and b[2].shape == (b[0].shape[0],) for b in got)
    assert ids.tolist() == [(100 if width == 3 else 0) + i for i in range(n)]                    # the loader's ids, else the running index


def test_read_once_keeps_dtype_shape_and_bits_in_one_transfer(monkeypatch):
    import numpy as np
    f32 = torch.tensor([[1.5, float("nan"), -0.0], [3.0e38, -1.0e-40, 2.0]])
    named = {"u8": torch.arange(7, dtype=torch.uint8) + 250, "f32": f32, "i64": torch.tensor([-1, 2 ** 40 + 3, -2 ** 62]), "none": None,
             "i32": torch.tensor([-5, 4, 3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32), "f64": torch.tensor([1.0 / 3.0], dtype=torch.float64),
             "empty": torch.zeros((0, 4)), "u8b": torch.tensor([9], dtype=torch.uint8)}
    want = {k: None if v is None else v.numpy().copy() for k, v in named.items()}
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    got = T.read_once(named)
    monkeypatch.undo()
    assert len(calls) == 1, f"{len(calls)} device-to-host transfers"
    assert list(got) == list(named) and got["none"] is None
    for k, w in want.items():
        if w is not None:
            assert isinstance(got[k], np.ndarray) and got[k].dtype == w.dtype and got[k].shape == w.shape, k
            assert got[k].tobytes() == w.tobytes(), f"{k}: the bits changed"
    assert got["empty"].size == 0 and np.signbit(got["f32"][0, 2]) and np.isnan(got["f32"][0, 1])
    for k in got:                                                   # independent copies: writing one array changes no other
        if got[k] is not None and got[k].size:
            got[k].reshape(-1).view(np.uint8)[:] ^= 0xFF
            assert all(got[j].tobytes() == want[j].tobytes() for j in got if j != k and want[j] is not None)
            got[k].reshape(-1).view(np.uint8)[:] ^= 0xFF
    assert T.read_once({"a": None}) == {"a": None}


def test_eval_mode_restores_the_mode_it_found():
    from protopformer_amd.protopformer import PPNet

    class Net(torch.nn.Module):
        eval_mode = PPNet.eval_mode

        def __init__(self):
            super().__init__()
            self.drop = torch.nn.Dropout(0.5)

    m = Net()
    for start in (True, False):
        m.train(start)
        with m.eval_mode() as inside:
            assert inside is m and not m.training and not m.drop.training
        assert m.training is start and m.drop.training is start
        with pytest.raises(KeyError):
            with m.eval_mode():
                assert not m.training
                raise KeyError("body")
        assert m.training is start and m.drop.training is start


def test_forward_outputs_travel_by_name_not_by_side_channel():
    """The source rules of the record: no stashed activations, one assignment of the test-facing arg-max and no reader outside tests/, one
    place that switches the training flag by hand, no indexing of _branches by number."""
    import glob
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "protopformer_amd", "*.py")) + glob.glob(os.path.join(root, "scripts", "**", "*.py"), recursive=True))
    assert len(files) > 20
    argmax, switching = [], set()
    for path in files:
        with open(path) as f:
            text = f.read()
        assert "_last_act_max" not in text, path
        assert not re.search(r"_branches\([^)]*\)\s*\[", text), path
        func = None
        for line in text.splitlines():
            func = (re.match(r"\s*def (\w+)", line) or [None, func])[1]
            argmax += [(path, line)] * line.count("_last_argmax")
            if "was_training" in line:
                switching.add((os.path.basename(path), func))
    assert len(argmax) == 1 and re.search(r"self\._last_argmax = ", argmax[0][1]) and argmax[0][0].endswith("protopformer.py"), argmax
    assert switching == {("protopformer.py", "eval_mode")}, switching


def _args(*argv):
    from protopformer_amd.train import get_args_parser
    return get_args_parser().parse_args(list(argv))


def test_model_from_args_is_the_call_the_tools_spelled_out():
    from protopformer_amd.protopformer import construct_PPNet
    # the parser's defaults, and the three flags without which no PPNet is built (use_global with one reserve layer)
    args = _args("--no-pretrained", "--base_architecture", "deit_tiny_patch16_224", "--use_global", "true", "--reserve_layers", "11",
                 "--reserve_token_nums", "81")
    ref = construct_PPNet(base_architecture=args.base_architecture, pretrained=not args.no_pretrained, img_size=args.img_size,
                          prototype_shape=args.prototype_shape, num_classes=200, reserve_layers=args.reserve_layers,
                          reserve_token_nums=args.reserve_token_nums, use_global=args.use_global, use_ppc_loss=args.use_ppc_loss,
                          ppc_cov_thresh=args.ppc_cov_thresh, ppc_mean_thresh=args.ppc_mean_thresh, global_coe=args.global_coe,
                          global_proto_per_class=args.global_proto_per_class,
                          prototype_activation_function=args.prototype_activation_function, add_on_layers_type=args.add_on_layers_type)
    got = T.model_from_args(args, 200)
    shapes = lambda m: {k: tuple(v.shape) for k, v in m.state_dict().items()}      # noqa: E731
    assert shapes(got) == shapes(ref) and list(got.state_dict()) == list(ref.state_dict())
    assert got.img_size == ref.img_size == 224 and got.num_classes == 200


def test_model_from_args_overrides(monkeypatch):
    """interp_eval's case: its parser has --input_size and neither --img_size nor --no-pretrained."""
    import protopformer_amd.protopformer as PP
    seen = {}
    monkeypatch.setattr(PP, "construct_PPNet", lambda **kw: seen.update(kw) or "model")
    args = _args("--no-pretrained", "--use_global", "true", "--reserve_layers", "11", "--reserve_token_nums", "81")
    assert T.model_from_args(args, 7) == "model"
    assert seen["pretrained"] is False and seen["img_size"] == 224 and seen["num_classes"] == 7 and seen["use_global"] is True
    assert seen["reserve_layers"] == [11] and seen["reserve_token_nums"] == [81] and len(seen) == 15
    T.model_from_args(args, 7, img_size=96, pretrained=True)
    assert seen["pretrained"] is True and seen["img_size"] == 96
    del args.img_size, args.no_pretrained
    T.model_from_args(args, 7, img_size=64, pretrained=True)
    assert seen["img_size"] == 64


def test_regroup_carries_every_field_across_batch_borders():
    """Three fields, 7 images in loader batches of 2, passes of 3: the batch size does not divide the pass, a pass takes rows of two
    batches, the last one is short."""
    x, y, ids = torch.arange(21.0).reshape(7, 3), torch.arange(7) * 10, torch.arange(7) + 100
    loader = [(x[i:i + 2], y[i:i + 2], ids[i:i + 2]) for i in range(0, 7, 2)]
    passes = list(T.regroup(loader, 3))
    assert [tuple(f.shape[0] for f in p) for p in passes] == [(3, 3, 3), (3, 3, 3), (1, 1, 1)]
    for j, whole in enumerate((x, y, ids)):
        assert torch.equal(torch.cat([p[j] for p in passes]), whole) and all(p[j].dtype == whole.dtype and p[j].is_contiguous() for p in passes)
    assert passes[0][2].tolist() == [100, 101, 102] and passes[1][1].tolist() == [30, 40, 50]      # image 2 crossed a batch border with its fields
    assert list(T.regroup([], 3)) == []


def test_read_rows_concatenates_per_field_in_one_read(monkeypatch):
    import numpy as np
    kept = [dict(ids=torch.tensor([3, 1]), same=torch.arange(12.0).reshape(2, 2, 3), lost=None, base=torch.ones(2, 3, dtype=torch.float64)),
            dict(ids=torch.tensor([7]), same=100 + torch.arange(6.0).reshape(2, 1, 3), lost=None, base=torch.zeros(1, 3, dtype=torch.float64))]
    calls, real = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append(1) or real(self, *a, **k))
    rows = T.read_rows(kept, "somebody", dict(same=1))
    monkeypatch.undo()
    assert len(calls) == 1 and list(rows) == ["ids", "same", "lost", "base"] and rows["lost"] is None
    assert rows["ids"].tolist() == [3, 1, 7] and rows["ids"].dtype == np.int64
    assert rows["same"].shape == (2, 3, 3) and rows["same"].dtype == np.float32                   # [n, N, K]: the images on dim 1
    assert rows["same"][:, :2].tobytes() == kept[0]["same"].numpy().tobytes() and rows["same"][:, 2].tolist() == [[100, 101, 102], [103, 104, 105]]
    assert rows["base"].shape == (3, 3) and rows["base"].dtype == np.float64 and rows["base"][:, 0].tolist() == [1, 1, 0]
    with pytest.raises(ValueError, match="somebody: the loader gave no image"):
        T.read_rows([], "somebody")


def test_write_json_cleans_nan_and_keys_at_every_depth(tmp_path):
    import json
    import types
    nan = float("nan")
    doc = dict(images=3, overall=dict(mean=nan, rows=2), per_prototype={4: dict(share=nan, deep={7: [1.5, nan, (nan, 2)]}), 11: dict(share=0.25)}, none=None)
    args = types.SimpleNamespace(output_dir=str(tmp_path / "made" / "here"))
    path = T.write_json(args, "doc.json", doc)
    assert path == str(tmp_path / "made" / "here" / "doc.json")
    text = open(path).read()
    assert "NaN" not in text and json.loads(text) == dict(images=3, overall=dict(mean=None, rows=2), none=None,
                                                          per_prototype={"4": dict(share=None, deep={"7": [1.5, None, [None, 2]]}), "11": dict(share=0.25)})
    # what the tools wrote before: a shallow clean of the values, prototype ids as strings, indent 1
    shallow = dict(overall={k: (None if isinstance(v, float) and v != v else v) for k, v in doc["overall"].items()}, per={str(p): v for p, v in {4: 1, 11: 2}.items()})
    assert open(T.write_json(args, "same.json", dict(overall=doc["overall"], per={4: 1, 11: 2}))).read() == json.dumps(shallow, indent=1)


@pytest.mark.parametrize("device_data", [False, True])
def test_eval_loader_passes_square_to_the_view_and_the_device_loader(monkeypatch, device_data):
    import types
    from protopformer_amd import data as D
    seen = {}
    monkeypatch.setattr(D, "build_view_transform", lambda args, square=False: seen.update(view=square) or "view")
    monkeypatch.setattr(D, "build_dataset", lambda train, args, transform=None: (types.SimpleNamespace(return_id=False, transform=transform), 7))
    monkeypatch.setattr(D, "device_data_enabled", lambda args: device_data)
    monkeypatch.setattr(D, "DeviceDataset", lambda ds, device, num_workers=0: ("resident", ds))
    monkeypatch.setattr(D, "DeviceAugLoader", lambda dds, bs, fin, train, args, square=False: seen.update(loader=square) or "device loader")
    monkeypatch.setattr(D, "DeviceLoader", lambda ds, bs, device, fin, shuffle=False, num_workers=0: "host loader")
    args = types.SimpleNamespace(split="test", num_workers=0, batch_size=4)
    for square in (True, False):
        seen.clear()
        ds, classes, loader = T.eval_loader(args, "cpu", square=square)
        assert seen["view"] is square and ds.transform == "view" and ds.return_id is True and classes == 7
        assert (loader, seen.get("loader")) == (("device loader", square) if device_data else ("host loader", None))
