"""PartsWorld on the device: ppf_synth_scene and ppf_synth_render against the numpy referees of data.py, bit for bit; a DeviceDataset
rendered in place and the loaders over it; the train driver on both loader paths; focus, interp_eval and faithfulness on the rendered
set with nothing on disk."""
import json
import math
import os

import numpy as np
import pytest
import torch

from protopformer_amd import data as D
from protopformer_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPECIAL_IDS = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 3]


def _spec(H=64, W=64, **kw):
    kw = dict(dict(classes=200, parts=8, distractors=8, n_train=64, n_test=32, seed=3, noise=8, grid=4), **kw)
    return D.PartsWorldSpec(height=H, width=W, **kw)


def _ids(B, offset=0):
    """B ids that start with the ones whose low word wraps and whose high word is set."""
    more = [7 + offset + 3 * i for i in range(max(0, B - len(SPECIAL_IDS)))]
    return np.array((SPECIAL_IDS + more)[:B] if B >= len(SPECIAL_IDS) else SPECIAL_IDS[2:2 + B], dtype=np.int64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ ppf_synth_scene
@pytest.mark.parametrize("seed", [0, (1 << 63) + 12345])
@pytest.mark.parametrize("C", [2, 200])
@pytest.mark.parametrize("K,Dn", [(1, 0), (8, 8)])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_scene_kernel_equals_referee(B, K, Dn, C, seed):
    if C > D.SYNTH_ATTRS ** K:
        with pytest.raises(ValueError, match=r"C > A\^K"):                     # 200 classes of one part: refused by name, as the library refuses it
            _spec(37, 48, classes=C, parts=K, distractors=Dn, seed=seed)
        rc = ops._lib.lib().ppf_synth_scene(None, None, B, C, K, Dn, 37, 48, 4, 8, 0, None)
        assert rc == -1 and "A^K" in ops._lib.lib().ppf_last_error().decode()
        return
    spec = _spec(37, 48, classes=C, parts=K, distractors=Dn, seed=seed, grid=3)
    ids = _ids(B)
    got = D.partsworld_scene_from_ids(spec, ids, device=True)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (B, D.SYNTH_WORDS)
    assert np.array_equal(got.cpu().numpy(), D.partsworld_scene_from_ids(spec, ids))


def test_scene_kernel_at_every_frame_and_grid():
    ids = _ids(40)
    for (H, W), g in (((32, 32), 1), ((256, 256), 8), ((64, 64), 5), ((1024, 32), 2)):
        spec = _spec(H, W, grid=g)
        assert np.array_equal(ops.synth_scene(spec, _dev(ids)).cpu().numpy(), D.partsworld_scene_from_ids(spec, ids)), (H, W, g)


# ------------------------------------------------------------------------------------------------ ppf_synth_render
def _check_render(spec, ids, partmap=True):
    scene = D.partsworld_scene_from_ids(spec, ids)
    want_f, want_m = D.partsworld_render(spec, scene, ids, partmap=True)
    got = D.partsworld_render(spec, scene, ids, device=True, partmap=partmap)
    got_f, got_m = got if partmap else (got, None)
    assert got_f.is_cuda and got_f.dtype == torch.uint8 and tuple(got_f.shape) == want_f.shape
    assert np.array_equal(got_f.cpu().numpy(), want_f)
    if partmap:
        assert got_m.dtype == torch.uint8 and np.array_equal(got_m.cpu().numpy(), want_m)
    return want_f, want_m


@pytest.mark.parametrize("noise", [0, 32])
@pytest.mark.parametrize("g", [1, 8])
@pytest.mark.parametrize("H,W,B", [(32, 32, 1), (32, 32, 5), (32, 32, 67), (37, 48, 5), (64, 64, 5), (256, 256, 2)])
def test_render_kernel_equals_referee(H, W, B, g, noise):
    _check_render(_spec(H, W, grid=g, noise=noise), _ids(B))


def test_render_kernel_without_partmap_and_few_primitives():
    _check_render(_spec(37, 48, classes=2, parts=1, distractors=0), _ids(5), partmap=False)
    _check_render(_spec(32, 64, classes=20, parts=4, distractors=3, noise=0), _ids(6))
    f, m = _check_render(_spec(48, 1024, grid=7), _ids(2))                      # the widest row
    assert (m >= 3).any() and (m == 1).any() and (m == 0).any()


def test_one_launch_of_eight_equals_two_of_four():
    spec = _spec(37, 48, noise=32)
    ids = _dev(_ids(8))
    scene = ops.synth_scene(spec, ids)
    whole_f, whole_m = ops.synth_render(spec, scene, ids, partmap=True)
    for s in (slice(0, 4), slice(4, 8)):
        part_scene = ops.synth_scene(spec, ids[s].contiguous())
        assert torch.equal(part_scene, scene[s])
        f, m = ops.synth_render(spec, part_scene, ids[s].contiguous(), partmap=True)
        assert torch.equal(f, whole_f[s]) and torch.equal(m, whole_m[s])


def test_render_into_a_larger_buffer_leaves_the_guards_alone():
    spec = _spec(37, 48)
    ids = _ids(5)
    n = 5 * 37 * 48
    for offset in (16, 4096 + 48):
        buf = torch.full((offset + 3 * n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        pm = torch.full((offset + n + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        scene = ops.synth_scene(spec, _dev(ids))
        out, pmo = ops.synth_render(spec, scene, _dev(ids), out=buf[offset:offset + 3 * n], partmap=pm[offset:offset + n])
        assert out.data_ptr() == buf.data_ptr() + offset and pmo.data_ptr() == pm.data_ptr() + offset
        want_f, want_m = D.partsworld_render(spec, scene.cpu().numpy(), ids, partmap=True)
        assert np.array_equal(buf[offset:offset + 3 * n].cpu().numpy(), want_f.reshape(-1)) and np.array_equal(pm[offset:offset + n].cpu().numpy(), want_m.reshape(-1))
        assert bool((buf[:offset] == 0xA5).all()) and bool((buf[offset + 3 * n:] == 0xA5).all())
        assert bool((pm[:offset] == 0x5A).all()) and bool((pm[offset + n:] == 0x5A).all())
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.synth_render(spec, scene, _dev(ids), out=buf[8:8 + 3 * n])
    with pytest.raises(ValueError, match="out must be"):
        ops.synth_render(spec, scene, _dev(ids), out=buf[:3 * n - 16])
    with pytest.raises(ValueError, match="scene must be"):
        ops.synth_render(spec, scene[:4], _dev(ids))


# ------------------------------------------------------------------------------------------------ DeviceDataset and the loaders
WORLD = dict(classes=4, parts=4, distractors=3, n_train=32, n_test=16, seed=5, noise=8, grid=4)


def _args(spec, **kw):
    import types
    return types.SimpleNamespace(input_size=64, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="PartsWorld", data_path="", batch_size=4,
                                 num_workers=0, reprob=0.25, partsworld=spec, **kw)


@pytest.fixture(scope="module")
def world():
    spec = _spec(80, 96, **WORLD)                                              # not square, not the input size: the resize has work to do
    ds = D.PartsWorld(spec, train=False, return_id=True)
    return spec, ds, D.DeviceDataset(ds, DEV)


def test_device_dataset_is_rendered_in_place(world):
    spec, ds, dd = world
    want = D.partsworld_render(spec, D.partsworld_scene_from_ids(spec, ds.ids), ds.ids)
    assert dd.rendered and len(dd) == 16 and dd.flat.dtype == torch.uint8 and np.array_equal(dd.flat.cpu().numpy(), want.reshape(-1))
    assert dd.offsets_host.tolist() == [i * 80 * 96 * 3 for i in range(16)] and torch.equal(dd.offsets.cpu(), torch.from_numpy(dd.offsets_host))
    assert dd.sizes_host.tolist() == [[80, 96]] * 16 and dd.sizes.dtype == torch.int32 and dd.offsets.dtype == torch.int64
    assert np.array_equal(dd.labels_host, ds.ids % 4) and np.array_equal(dd.ids_host, ds.ids) and torch.equal(dd.ids.cpu(), torch.from_numpy(ds.ids))
    assert np.array_equal(np.asarray(ds[3][0]), want[3]) and ds[3][1:] == (int(ds.ids[3] % 4), int(ds.ids[3]))
    plain = D.DeviceDataset(D.PartsWorld(spec, train=True), DEV)
    assert plain.rendered and plain.ids is None and plain.ids_host is None and len(plain) == 32
    with pytest.raises(RuntimeError, match=r"max_bytes is 1000\b"):
        D.DeviceDataset(ds, DEV, max_bytes=1000)


def test_more_frames_than_one_run():
    spec = _spec(32, 32, classes=7, parts=2, distractors=1, n_train=300, n_test=1)
    ds = D.PartsWorld(spec, train=True)
    dd = D.DeviceDataset(ds, DEV)
    want = D.partsworld_render(spec, D.partsworld_scene_from_ids(spec, ds.ids), ds.ids)
    assert np.array_equal(dd.flat.cpu().numpy(), want.reshape(-1))


@pytest.mark.parametrize("square", [False, True], ids=["centre_crop", "square"])
@pytest.mark.parametrize("batch_size", [3, 8])
def test_eval_batches_equal_the_cpu_loader(world, batch_size, square):
    spec, ds, dd = world
    args = _args(spec)
    cpu_ds = D.PartsWorld(spec, train=False, transform=D.build_view_transform(args, square=square), return_id=True)
    cpu = D.DeviceLoader(cpu_ds, batch_size, torch.device(DEV), D.GpuFinisher(re_prob=0.0), shuffle=False, num_workers=0)
    dev = D.DeviceAugLoader(dd, batch_size, D.GpuFinisher(re_prob=0.0), False, args, square=square)
    n = 0
    for (x, y, ids), (xd, yd, idsd) in zip(cpu, dev):
        assert x.shape[1:] == (3, 64, 64) and torch.equal(x, xd) and torch.equal(y, yd) and torch.equal(torch.as_tensor(ids), idsd)
        n += len(y)
    assert n == 16 and len(cpu) == len(dev)


# ------------------------------------------------------------------------------------------------ the train driver
def _micro_model(classes=None):
    """The micro DeiT of tests/helpers.py (64 x 64 inputs, 10 classes: the 4 of the world are its first 4); with `classes`, the same
    backbone under a head of that many classes from a seeded init, so that the driver's accuracy is not 0 by construction."""
    from helpers import build_micro, micro
    sd, cfg, _ = micro("micro_deit.npz")
    if classes is None:
        return build_micro(cfg, sd)
    from protopformer_amd.deit import MyVisionTransformer
    from protopformer_amd.protopformer import PPNet
    torch.manual_seed(17)
    feats = MyVisionTransformer(img_size=cfg["img"], patch_size=16, embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"], drop_path_rate=0.0)
    m = PPNet(features=feats, img_size=cfg["img"], prototype_shape=[classes * cfg["protos_per_class"], cfg["proto_dim"], 1, 1], proto_layer_rf_info=None,
              num_classes=classes, reserve_layers=[cfg["reserve_layer"]], reserve_token_nums=[cfg["reserve_k"]], use_global=True, use_ppc_loss=True,
              ppc_cov_thresh=1., ppc_mean_thresh=2., global_coe=cfg["global_coe"], global_proto_per_class=cfg["global_per_class"],
              add_on_layers_type=cfg.get("add_on", "regular"))
    m.features.load_state_dict({k[len("features."):]: v for k, v in sd.items() if k.startswith("features.")}, strict=True)
    return m.cuda()


def _driver_args(out, spec, device_data, *extra):
    from protopformer_amd.train import get_args_parser
    args = get_args_parser().parse_args(["--data_set", "PartsWorld", "--output_dir", str(out), "--model", "micro_deit", "--input_size", "64",
                                         "--batch_size", "8", "--num_workers", "0", "--use_global", "true", "--no-pretrained", *extra])
    args.partsworld, args.device_data = spec, device_data
    return args


@pytest.mark.parametrize("device_data", [True, False], ids=["resident", "cpu_loader"])
def test_driver_trains_and_evaluates(tmp_path, device_data):
    from protopformer_amd import train
    spec = _spec(64, 64, **WORLD)
    out = tmp_path / "run"
    rec = train.main(_driver_args(out, spec, device_data, "--epochs", "2", "--save_ep_freq", "1"), model=_micro_model(4))
    assert len(rec) == 2 and all(math.isfinite(r["train_loss"]) and math.isfinite(r["test_loss"]) and r["test_n"] == 16 for r in rec)
    print(f"[{'resident' if device_data else 'cpu loader'}] acc1 per epoch {[r['test_acc1'] for r in rec]}")
    best, last = os.path.join(str(out), "checkpoints", "epoch-best.pth"), os.path.join(str(out), "checkpoints", "checkpoint-1.pth")
    assert os.path.exists(best) and os.path.exists(last)
    # --eval --resume gives back the evaluation of the epoch the checkpoint was written after: the last one, and the best one
    got = train.main(_driver_args(tmp_path / "eval_last", spec, device_data, "--eval", "--resume", last), model=_micro_model(4))
    assert got["acc1"] == rec[1]["test_acc1"] and got["loss"] == rec[1]["test_loss"] and got["n"] == 16
    accs = [r["test_acc1"] for r in rec]
    got = train.main(_driver_args(tmp_path / "eval_best", spec, device_data, "--eval", "--resume", best), model=_micro_model(4))
    assert got["acc1"] == max(accs) == rec[accs.index(max(accs))]["test_acc1"] and got["loss"] == rec[accs.index(max(accs))]["test_loss"]


# ------------------------------------------------------------------------------------------------ the tools
TOOL_WORLD = dict(WORLD, n_test=12)


def _json_round_trip(doc):
    from protopformer_amd.tooling import json_clean
    return json.loads(json.dumps(json_clean(doc)))


@pytest.mark.parametrize("device_data", [False, True], ids=["cpu_loader", "resident"])
def test_focus_on_the_rendered_set(tmp_path, device_data):
    from protopformer_amd import focus as tool
    from protopformer_amd import tooling
    from protopformer_amd.interpret import foreground_focus
    spec = _spec(80, 96, **TOOL_WORLD)
    args = tool.get_args_parser().parse_args(["--data_set", "PartsWorld", "--output_dir", str(tmp_path), "--input_size", "64", "--batch_size", "5",
                                              "--num_workers", "0", "--percentile", "90"])
    args.partsworld, args.device_data = spec, device_data
    m = _micro_model()
    path = tool.main(args, model=m)
    doc = json.load(open(path))
    ds, nb, loader = tooling.eval_loader(args, torch.device(DEV), square=True)
    ann = ds.annotation()
    assert nb == 4 and isinstance(ds, D.PartsWorld) and not ds.train
    want = foreground_focus(m, loader, ann.id_to_bbox, ann.image_sizes, protos="own", protos_per_image=3, percentile=90.0)
    assert doc == _json_round_trip(tool.summarize(want, args))
    assert doc["images"] == 12 and doc["settings"]["boxes"] == "annotation" and doc["settings"]["data_set"] == "PartsWorld"
    assert 0 < doc["overall"]["prototype_maps"]["chance"] < 1


def test_interp_eval_on_the_rendered_set(tmp_path):
    from protopformer_amd import interp_eval as tool
    from protopformer_amd.interpret import interpretability_scores
    spec = _spec(80, 96, **TOOL_WORLD)
    args = tool.get_args_parser().parse_args(["--data_set", "PartsWorld", "--out_dir", str(tmp_path), "--input_size", "64", "--batch_size", "5"])
    assert tool.get_args_parser().parse_args([]).data_set == "CUB2011U"         # the default stays CUB
    args.partsworld, args.device_data = spec, True
    m = _micro_model()
    got = tool.main(args, model=m)
    doc = json.load(open(os.path.join(str(tmp_path), "interpretability.json")))
    ds = D.PartsWorld(spec, train=False, transform=D.build_view_transform(args, square=True), return_id=True)
    loader = D.DeviceAugLoader(D.DeviceDataset(ds, DEV), 5, D.GpuFinisher(re_prob=0.0), False, args, square=True)
    ann = ds.annotation()
    want = interpretability_scores(m, loader, ann, ann.image_sizes, num_classes=4, part_thresh=0.8, half_size=36, n_parts=4, noise_std=0.2, seed=0)
    assert _json_round_trip(got) == _json_round_trip(want) and doc == _json_round_trip(tool.report(want, 12, args))
    assert doc["images"] == 12 and len(doc["effects"]) >= 1


def test_faithfulness_runs_through_on_the_rendered_set(tmp_path):
    from protopformer_amd import faithfulness as tool
    spec = _spec(80, 96, **TOOL_WORLD)
    args = tool.get_args_parser().parse_args(["--data_set", "PartsWorld", "--output_dir", str(tmp_path), "--input_size", "64", "--batch_size", "5",
                                              "--num_workers", "0", "--steps", "4", "--max_images", "7", "--orders", "evidence", "random"])
    args.partsworld, args.device_data = spec, True
    path = tool.main(args, model=_micro_model())
    doc = json.load(open(path))
    assert doc["images"] == 7 and set(doc["orders"]) == {"evidence", "random"}
