"""The device-resident data path on the GPU: every kernel of csrc/device_data.hip bit-equal to its numpy referee (which
tests/test_device_data_cpu.py holds to Pillow), the loader bit-equal to Pillow end to end, evaluation metrics unchanged."""
import random
import types

import numpy as np
import pytest
import torch
from PIL import Image

from protopformer_amd import data as D
from test_device_data_cpu import RESIZE_CASES, ScriptedRng, aug_images, frame

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pack(frames, lead=0):
    """(flat uint8 buffer with `lead` bytes in front, offsets, (h, w) sizes) of a list of HWC frames."""
    offsets, at = [], lead
    for f in frames:
        offsets.append(at)
        at += f.size
    return np.concatenate([np.zeros(lead, dtype=np.uint8)] + [f.reshape(-1) for f in frames]), offsets, [f.shape[:2] for f in frames]


def _both(flat, plan, H, W, filt=Image.BICUBIC):
    want = D.resize_crop(flat, plan, H, W, filter=filt)
    got = D.resize_crop(torch.from_numpy(flat).to(DEV), plan, H, W, device=True, filter=filt).cpu().numpy()
    return got, want


@pytest.mark.parametrize("case", sorted(RESIZE_CASES))
def test_resize_kernel_equals_referee(case):
    h, w, box, out, win, size = RESIZE_CASES[case]
    flat, offsets, sizes = _pack([frame(h, w, 11), frame(h, w, 12)], lead=5)       # plain and mirrored in one launch, odd offsets
    plan = D.resize_plan(offsets, sizes, [box, box], [out, out], [win, win], [0, 1])
    got, want = _both(flat, plan, *size)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("W", [16, 20])
def test_resize_kernel_ragged_batch(W):
    """Three frames of different sizes and scales in one launch (the workspace is sized by the largest), the second at an odd offset."""
    frames = [frame(37, 53, 1), frame(90, 61, 2), frame(9, 7, 3)]
    flat, offsets, sizes = _pack(frames, lead=0)
    assert offsets[1] % 2 == 1
    plan = D.resize_plan(offsets, sizes, [(3, 2, 50, 30), (0, 0, 61, 90), (0, 0, 7, 9)], [(12, W)] * 3, [(0, 0)] * 3, [0, 1, 0])
    got, want = _both(flat, plan, 12, W)
    assert np.array_equal(got, want), int((got != want).sum())
    for b, f in enumerate(frames):                                               # and the referee is Pillow's
        box = [(3, 2, 50, 30), (0, 0, 61, 90), (0, 0, 7, 9)][b]
        ref = np.asarray(Image.fromarray(f).resize((W, 12), Image.BICUBIC, box=box))
        assert np.array_equal(want[b], ref[:, ::-1] if b == 1 else ref)


def test_resize_kernel_bilinear_square_view():
    flat, offsets, sizes = _pack([frame(37, 53, 4)])
    got, want = _both(flat, D.resize_plan(offsets, sizes, [(0, 0, 53, 37)], [(16, 16)], [(0, 0)], [0]), 16, 16, Image.BILINEAR)
    assert np.array_equal(got, want)


def test_resize_kernel_refuses_a_bad_plan():
    flat, offsets, sizes = _pack([frame(37, 53, 4)])
    plan = D.resize_plan([1], sizes, [(0, 0, 53, 37)], [(12, 16)], [(0, 0)], [0])        # the frame would end one byte past the buffer
    with pytest.raises(RuntimeError, match="leaves the"):
        D.resize_crop(torch.from_numpy(flat).to(DEV), plan, 12, 16, device=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.resize_crop(torch.from_numpy(flat), plan, 12, 16, device=True)


def _aug_both(frames, plan, fill):
    want = D.randaugment_apply(frames, plan, fill)
    got = D.randaugment_apply(torch.from_numpy(frames).to(DEV), plan, fill, device=True).cpu().numpy()
    return got, want


@pytest.mark.parametrize("name", D.RandAugment.OPS)
def test_aug_kernels_equal_referee_op_by_op(name):
    """One launch chain per op over the CPU cases: noise and constant image x magnitudes x signs x resample filters."""
    frames, draws = [], []
    for img in aug_images().values():
        for mag in (0, 4.3, 9, 10):
            for negate in (False, True):
                for resample in (Image.BILINEAR, Image.BICUBIC):
                    frames.append(img)
                    draws.append([D.RandAugment(rng=ScriptedRng(resample, negate))._draw_op(name, mag)])
    if name.startswith("Translate"):
        frames += [frame(24, 20, 2)] * 2
        draws += [[(name, 1.5, Image.BILINEAR)], [(name, -1.5, Image.BICUBIC)]]       # fully out of frame
    frames = np.stack(frames)
    got, want = _aug_both(frames, D.aug_plan(draws, 24, 20), D.RandAugment().fill)
    bad = [b for b in range(len(frames)) if not np.array_equal(got[b], want[b])]
    assert not bad, [(draws[b], int((got[b] != want[b]).sum())) for b in bad[:4]]


def test_aug_kernels_mixed_batch_and_skipped_sample():
    """Every sample carries another op in each slot; one sample has both slots skipped and must come back as it went in."""
    ops = D.RandAugment.OPS
    ra = D.RandAugment(rng=random.Random(9))
    draws = [[ra._draw_op(ops[b], 9.0), ra._draw_op(ops[(b + 7) % 15], 4.3)] for b in range(15)]
    draws += [[(None, 0.0, Image.BILINEAR)] * 2, [(None, 0.0, Image.BILINEAR), ra._draw_op("Rotate", 9.0)], [ra._draw_op("Equalize", 9.0), (None, 0.0, Image.BILINEAR)]]
    frames = np.stack([frame(31, 27, 40 + b) for b in range(len(draws))])                # odd sizes: 31 * 27 pixels is no multiple of the block
    got, want = _aug_both(frames, D.aug_plan(draws, 31, 27), ra.fill)
    assert np.array_equal(got, want), [b for b in range(len(draws)) if not np.array_equal(got[b], want[b])]
    assert np.array_equal(got[15], frames[15])
    for b in (0, 3, 10):                                                                 # and the referee is Pillow's
        assert np.array_equal(want[b], np.asarray(ra.apply(draws[b], Image.fromarray(frames[b]))))


def test_aug_histogram_more_than_one_block():
    """224 x 224: the histogram of one sample is gathered by several workgroups."""
    frames = np.stack([frame(224, 224, 70), frame(224, 224, 71), frame(224, 224, 72)])
    draws = [[("Equalize", 0.0, Image.BILINEAR)], [("AutoContrast", 0.0, Image.BILINEAR)], [("ContrastIncreasing", 1.81, Image.BILINEAR)]]
    frames[1] = frames[1] // 2 + 17
    got, want = _aug_both(frames, D.aug_plan(draws, 224, 224), (124, 116, 104))
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def cub(tmp_path_factory):
    from mini_trees import build_cub
    root = str(tmp_path_factory.mktemp("cub_dd"))
    build_cub(root)
    return root


def _args(root, **kw):
    return types.SimpleNamespace(input_size=64, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="CUB2011U", data_path=root, batch_size=4,
                                 num_workers=0, reprob=0.25, **kw)


@pytest.fixture(scope="module")
def resident(cub):
    return {train: D.DeviceDataset(D.Cub2011(cub, train=train, return_id=not train), DEV) for train in (True, False)}


def _frame_of(dd, i):
    h, w = (int(v) for v in dd.sizes_host[i])
    o = int(dd.offsets_host[i])
    return Image.fromarray(dd.flat[o:o + h * w * 3].cpu().numpy().reshape(h, w, 3))


def test_device_dataset_tables(cub, resident):
    dd = resident[False]
    ds = D.Cub2011(cub, train=False, transform=D.ToUint8HWC(), return_id=True)
    assert len(dd) == len(ds) and dd.flat.dtype == torch.uint8 and dd.offsets.dtype == torch.int64 and dd.sizes.dtype == torch.int32
    for i in range(len(ds)):
        a, label, img_id = ds[i]
        assert np.array_equal(np.asarray(_frame_of(dd, i)), a) and int(dd.labels[i]) == label and int(dd.ids[i]) == img_id
    assert resident[True].ids is None


def test_device_dataset_over_max_bytes_raises(cub):
    with pytest.raises(RuntimeError, match=r"max_bytes is 100000\b"):
        D.DeviceDataset(D.Cub2011(cub, train=True), DEV, max_bytes=100000)


@pytest.mark.parametrize("batch_size", [3, 4])
def test_train_loader_equals_pillow(cub, resident, batch_size):
    """The finished fp32 batches against the same decoded frames pushed through Compose under the same plan (the crop box, the flip, the
    RandAugment draws) and through GpuFinisher with the same rectangles; the epoch is the same at both batch sizes."""
    dd, args = resident[True], _args(cub)
    loader = D.DeviceAugLoader(dd, batch_size, D.GpuFinisher(re_prob=0.25, seed=5), True, args, shuffle=True, seed=3, keep_plans=True)
    loader.set_epoch(2)
    ref_finish = D.GpuFinisher(re_prob=0.25, seed=5)
    ra = D.RandAugment(args.aa, img_size=64)
    batches = list(loader)
    assert len(batches) == len(loader) == -(-len(dd) // batch_size) and len(loader.host_seconds) == len(batches)
    for (x, y), plan in zip(batches, loader.plans):
        frames = []
        for j, i in enumerate(plan["idx"]):
            p = plan["resize"][j]
            t = D.Compose([lambda im: im.resize((64, 64), Image.BICUBIC, box=tuple(int(v) for v in p[3:7])),
                           lambda im: im.transpose(Image.FLIP_LEFT_RIGHT) if p[11] else im, lambda im: ra.apply(plan["draws"][j], im), D.ToUint8HWC()])
            frames.append(t(_frame_of(dd, int(i))))
        want = ref_finish(torch.from_numpy(np.stack(frames)).to(DEV), rects=plan["rects"])
        assert x.dtype == torch.float32 and tuple(x.shape) == (len(plan["idx"]), 3, 64, 64) and torch.equal(x, want)
        assert torch.equal(y.cpu(), torch.from_numpy(dd.labels_host[plan["idx"]]))
    # the epoch is a function of (seed, epoch, rank) and the order alone: the same samples, boxes, flips, ops and rectangles as at batch size 1
    one = D.DeviceAugLoader(dd, 1, D.GpuFinisher(re_prob=0.25, seed=5), True, args, shuffle=True, seed=3, keep_plans=True)
    one.set_epoch(2)
    assert len(list(one)) == len(dd)
    for key in ("idx", "resize", "aug", "rects"):
        assert np.array_equal(np.concatenate([p[key] for p in loader.plans]), np.concatenate([p[key] for p in one.plans])), key
    assert sum(len(p["idx"]) for p in loader.plans) == len(dd) and any(p["rects"][:, 2].any() for p in loader.plans)
    assert any((p["aug"][:, :, 0] != D.AUG_SKIP).any() for p in loader.plans) and any(p["resize"][:, 11].any() for p in loader.plans)


@pytest.mark.parametrize("batch_size", [3, 4])
def test_eval_loader_equals_pillow(cub, resident, batch_size):
    dd, args = resident[False], _args(cub)
    loader = D.DeviceAugLoader(dd, batch_size, D.GpuFinisher(re_prob=0.0), False, args)
    t, finish, at = D.build_transform(False, args), D.GpuFinisher(re_prob=0.0), 0
    for x, y, ids in loader:
        idx = range(at, at + len(y))
        want = finish(torch.from_numpy(np.stack([t(_frame_of(dd, i)) for i in idx])).to(DEV))
        assert torch.equal(x, want) and torch.equal(y.cpu(), torch.from_numpy(dd.labels_host[list(idx)]))
        assert torch.equal(ids, torch.from_numpy(dd.ids_host[list(idx)]))
        at += len(y)
    assert at == len(dd)


def test_square_view_loader_equals_pillow(cub, resident):
    dd, args = resident[False], _args(cub)
    t, finish = D.build_view_transform(args, square=True), D.GpuFinisher(re_prob=0.0)
    x = next(iter(D.DeviceAugLoader(dd, 5, D.GpuFinisher(re_prob=0.0), False, args, square=True)))[0]
    assert torch.equal(x, finish(torch.from_numpy(np.stack([t(_frame_of(dd, i)) for i in range(5)])).to(DEV)))


def test_evaluate_epoch_metrics_identical(cub, tmp_path):
    """engine.evaluate_epoch through DeviceLoader and through the resident path (the switch on args): identical metrics."""
    from helpers import build_micro, micro
    from protopformer_amd.engine import evaluate_epoch
    sd, cfg, _ = micro("micro_deit.npz")                   # 64 x 64 inputs, 10 classes
    model = build_micro(cfg, sd)
    args = _args(cub)
    _, val, _ = D.build_loaders(args, torch.device(DEV))
    args.device_data = True
    train_r, val_r, nb = D.build_loaders(args, torch.device(DEV))
    assert type(val) is D.DeviceLoader and type(val_r) is D.DeviceAugLoader and type(train_r) is D.DeviceAugLoader and nb == 200
    assert len(train_r) == len(train_r.dd) // 4 and len(val_r.dataset) == len(val.dataset)
    old, new = evaluate_epoch(val, model, torch.device(DEV)), evaluate_epoch(val_r, model, torch.device(DEV))
    assert old == new and new["n"] == len(val_r.dd)
    x, y = next(iter(train_r))                             # the train loader of the switch runs: crop, RandAugment, erase
    assert tuple(x.shape) == (4, 3, 64, 64) and bool(torch.isfinite(x).all())


def _driver_args(cub, out, *extra):
    from protopformer_amd.train import get_args_parser
    return get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", cub, "--output_dir", str(out), "--model", "micro_deit", "--input_size", "64",
                                         "--batch_size", "4", "--num_workers", "0", "--use_global", "true", *extra])


def test_driver_under_the_environment_switch(cub, tmp_path, monkeypatch):
    """python -m protopformer_amd.train with PPF_DEVICE_DATA=1: --eval gives the metrics of the CPU loaders exactly, and an epoch trains."""
    import math
    from helpers import build_micro, micro
    from protopformer_amd import train
    sd, cfg, _ = micro("micro_deit.npz")
    monkeypatch.delenv("PPF_DEVICE_DATA", raising=False)
    want = train.main(_driver_args(cub, tmp_path / "cpu", "--eval"), model=build_micro(cfg, sd))
    monkeypatch.setenv("PPF_DEVICE_DATA", "1")
    got = train.main(_driver_args(cub, tmp_path / "dev", "--eval"), model=build_micro(cfg, sd))
    assert got == want and got["n"] == 12
    rec = train.main(_driver_args(cub, tmp_path / "run", "--epochs", "1", "--step", "eager"), model=build_micro(cfg, sd))
    assert len(rec) == 1 and math.isfinite(rec[0]["train_loss"]) and rec[0]["test_n"] == 12


def test_tooling_eval_loader_under_the_switch(cub):
    """tooling.eval_loader (bank, explain, protostats, faithfulness, because, alignment, attribute): the same batches, ids included."""
    from protopformer_amd import tooling
    args = _args(cub, split="test", device_data=None)
    _, _, cpu = tooling.eval_loader(args, torch.device(DEV))
    args.device_data = True
    _, nb, dev = tooling.eval_loader(args, torch.device(DEV))
    assert type(cpu) is D.DeviceLoader and type(dev) is D.DeviceAugLoader and nb == 200
    n = 0
    for (x, y, ids), (xd, yd, idsd) in zip(cpu, dev):
        assert torch.equal(x, xd) and torch.equal(y, yd) and torch.equal(torch.as_tensor(ids), idsd)
        n += len(y)
    assert n == 12 and len(cpu) == len(dev)
