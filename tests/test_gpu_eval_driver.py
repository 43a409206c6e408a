"""GPU tests of the on-device evaluation metrics (ppf_eval_metrics, engine.EvalMeter / evaluate_epoch) and of the training driver
(protopformer_amd/train.py) end to end on a synthetic 16-image CUB tree."""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-10          # the loss sum is an fp64 function of the fp32 logits (fp64 row statistics): a few ulp of fp64 per row


def _acc(dev="cuda"):
    return torch.zeros(8, dtype=torch.float64, device=dev)


def _expected(x, y, g=None, l=None):
    """[n, ce sum, top-1, top-5, global top-1, local top-1] by torch on the CPU copies (labels all in range)."""
    B, C = x.shape
    ce = float(-torch.log_softmax(x.double(), 1)[torch.arange(B), y].sum())
    top5 = int((x.topk(min(5, C), 1).indices == y[:, None]).any(1).sum())
    return [float(B), ce, float((x.argmax(1) == y).sum()), float(top5),
            float((g.argmax(1) == y).sum()) if g is not None else 0.0, float((l.argmax(1) == y).sum()) if l is not None else 0.0]


def _tie_free(x):
    return bool((x.sort(1).values.diff(dim=1) != 0).all()) if x.shape[1] > 1 else True


def _random_logits(B, C, gen, scale=1.0):
    """Random fp32 logits without equal values in a row.  fp32 normal draws do collide now and then (1000 values a row, 24 mantissa
    bits: about one row in 257 x 1000), so rows that hold a tie are drawn again; the callers assert the result is tie-free."""
    x = torch.randn(B, C, generator=gen) * scale
    for _ in range(100):
        bad = (x.sort(1).values.diff(dim=1) == 0).any(1) if C > 1 else torch.zeros(B, dtype=torch.bool)
        if not bool(bad.any()):
            break
        x[bad] = torch.randn(int(bad.sum()), C, generator=gen) * scale
    return x


def _check(got, want, what=""):
    got = got.cpu().tolist()
    print(f"{what}: acc={got} expected={want} loss rel.err={abs(got[1] - want[1]) / max(abs(want[1]), 1e-300):.3e}")
    assert got[0] == want[0] and got[2:6] == want[2:6], (what, got, want)
    assert abs(got[1] - want[1]) <= LOSS_RTOL * abs(want[1]), (what, got[1], want[1])
    assert got[6] == 0.0 and got[7] == 0.0


@pytest.mark.parametrize("B,C", [(1, 200), (34, 200), (384, 200), (7, 3), (257, 1000)])
def test_eval_metrics_against_torch(B, C):
    from protopformer_amd import ops
    gen = torch.Generator().manual_seed(1000 * B + C)
    x, g, l = (_random_logits(B, C, gen, 3.0) for _ in range(3))
    y = torch.randint(0, C, (B,), generator=gen)
    assert _tie_free(x) and _tie_free(g) and _tie_free(l)          # top-1 / top-5 are unambiguous
    acc = _acc()
    ops.eval_metrics(acc, x.cuda(), y.cuda(), g.cuda(), l.cuda())
    want = _expected(x, y, g, l)
    _check(acc, want, f"{B}x{C}")
    if C < 5:
        assert want[3] == B
    # a second batch accumulates into the same buffer
    x2, g2, l2 = (_random_logits(B, C, gen) for _ in range(3))
    y2 = torch.randint(0, C, (B,), generator=gen)
    assert _tie_free(x2) and _tie_free(g2) and _tie_free(l2)
    ops.eval_metrics(acc, x2.cuda(), y2.cuda(), g2.cuda(), l2.cuda())
    w2 = _expected(x2, y2, g2, l2)
    _check(acc, [a + b for a, b in zip(want, w2)], f"{B}x{C} two batches")
    # without the global / local logits their slots stay untouched
    acc0 = _acc()
    ops.eval_metrics(acc0, x.cuda(), y.cuda())
    _check(acc0, _expected(x, y), f"{B}x{C} no branches")
    assert acc0[4].item() == 0.0 and acc0[5].item() == 0.0
    acc[4], acc[5] = 123.0, 456.0
    ops.eval_metrics(acc, x.cuda(), y.cuda())
    assert acc[4].item() == 123.0 and acc[5].item() == 456.0


def test_eval_metrics_ties_known_answers():
    from protopformer_amd import ops
    row = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0]
    for label, top1, top5 in ((4, 0.0, 1.0), (5, 0.0, 0.0), (0, 1.0, 1.0), (6, 0.0, 0.0)):
        acc = _acc()
        x = torch.tensor([row])
        ops.eval_metrics(acc, x.cuda(), torch.tensor([label]).cuda(), x.cuda(), x.cuda())
        got = acc.cpu().tolist()
        assert got[0] == 1.0 and got[2] == top1 and got[3] == top5 and got[4] == top1 and got[5] == top1, (label, got)
        ce = float(-torch.log_softmax(x.double(), 1)[0, label])
        assert abs(got[1] - ce) <= LOSS_RTOL * ce
    # C = 3: every in-range label is a top-5 hit, whatever the logits
    x = torch.tensor([[3.0, 2.0, 1.0], [3.0, 2.0, 1.0], [3.0, 2.0, 1.0], [0.0, 0.0, 0.0]])
    acc = _acc()
    ops.eval_metrics(acc, x.cuda(), torch.tensor([0, 1, 2, 2]).cuda())
    assert acc.cpu().tolist()[0] == 4.0 and acc[3].item() == 4.0 and acc[2].item() == 1.0


def test_eval_metrics_labels_out_of_range():
    from protopformer_amd import ops
    from protopformer_amd.engine import EvalMeter
    gen = torch.Generator().manual_seed(5)
    B, C = 9, 200
    x, g, l = (torch.randn(B, C, generator=gen) for _ in range(3))
    y = torch.randint(0, C, (B,), generator=gen)
    y[2], y[7] = -1, C
    good = torch.tensor([i for i in range(B) if i not in (2, 7)])
    m = EvalMeter(torch.device("cuda"))
    m.update(x.cuda(), y.cuda(), g.cuda(), l.cuda())
    got = m.acc.cpu().tolist()
    want = _expected(x[good], y[good], g[good], l[good])
    assert got[0] == float(B) and got[6] == 2.0 and got[7] == 0.0
    assert got[2:6] == want[2:6] and abs(got[1] - want[1]) <= LOSS_RTOL * abs(want[1])
    with pytest.raises(ValueError, match="outside"):
        m.result()
    m.reset()
    m.update(x[good].cuda(), y[good].cuda(), g[good].cuda(), l[good].cuda())
    r = m.result()
    assert r["n"] == 7 and r["acc1"] == 100.0 * want[2] / 7 and r["acc5"] == 100.0 * want[3] / 7 and r["global_acc1"] == 100.0 * want[4] / 7
    assert abs(r["loss"] - want[1] / 7) <= LOSS_RTOL * want[1] / 7
    with pytest.raises(ValueError):
        ops.eval_metrics(_acc(), x.cuda(), y.int().cuda())
    with pytest.raises(ValueError):
        ops.eval_metrics(torch.zeros(8, device="cuda"), x.cuda(), y.cuda())


def test_eval_metrics_large_logits():
    from protopformer_amd import ops
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(34, 200, generator=gen) * 3e4
    y = torch.randint(0, 200, (34,), generator=gen)
    acc = _acc()
    ops.eval_metrics(acc, x.cuda(), y.cuda())
    assert math.isfinite(acc[1].item())
    _check(acc, _expected(x, y), "3e4 logits")


def test_eval_metrics_bit_identical_runs():
    from protopformer_amd import ops
    gen = torch.Generator().manual_seed(11)
    batches = [(torch.randn(384, 200, generator=gen).cuda(), torch.randint(0, 200, (384,), generator=gen).cuda(),
                torch.randn(384, 200, generator=gen).cuda(), torch.randn(384, 200, generator=gen).cuda()) for _ in range(16)]
    runs = []
    for _ in range(2):
        acc = _acc()
        for x, y, g, l in batches:
            ops.eval_metrics(acc, x, y, g, l)
        runs.append(acc.cpu())
    assert runs[0][0].item() == 16 * 384
    assert torch.equal(runs[0].view(torch.int64), runs[1].view(torch.int64))


# ------------------------------------------------------------------------------------------------ the synthetic tree
def _jpeg(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path, quality=95)


def _build_tree(root):
    """16 images, 10 classes, images 1..12 train and 13..16 test, in CUB-200-2011's on-disk format."""
    meta = os.path.join(root, "CUB_200_2011")
    os.makedirs(os.path.join(meta, "images"))
    rows = []
    for i in range(1, 17):
        cls = (i - 1) % 10 + 1
        fp = f"{cls:03d}.B/{i:04d}.jpg"
        _jpeg(os.path.join(meta, "images", fp), 90 + i, 70 + i, i)
        rows.append((i, fp, cls, 1 if i <= 12 else 0))
    with open(os.path.join(meta, "images.txt"), "w") as f:
        f.write("".join(f"{i} {fp}\n" for i, fp, _, _ in rows))
    with open(os.path.join(meta, "image_class_labels.txt"), "w") as f:
        f.write("".join(f"{i} {c}\n" for i, _, c, _ in rows))
    with open(os.path.join(meta, "train_test_split.txt"), "w") as f:
        f.write("".join(f"{i} {t}\n" for i, _, _, t in rows))
    return root


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return _build_tree(str(tmp_path_factory.mktemp("cub16")))


def _micro_model():
    sd, cfg, _ = micro("micro_deit.npz")                   # 64x64 inputs, 10 classes
    return build_micro(cfg, sd)


def _args(tree, out, *extra):
    from protopformer_amd.train import get_args_parser
    return get_args_parser().parse_args(["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", str(out), "--model", "micro_deit",
                                         "--input_size", "64", "--batch_size", "4", "--num_workers", "0", "--use_global", "true",
                                         *extra])


def test_evaluate_epoch_against_evaluate(tree, tmp_path):
    """The new validation loop against the unchanged engine.evaluate on the micro DeiT: counts exactly, loss within 1e-5 (evaluate's
    ce_kernel is fast-math fp32), and the loss against fp64 torch on the model's own logits within 1e-10."""
    from protopformer_amd import data as D
    from protopformer_amd.engine import evaluate, evaluate_epoch
    args = _args(tree, tmp_path)
    _, val, nb = D.build_loaders(args, torch.device("cuda"))
    m = _micro_model()
    old = evaluate(val, m, torch.device("cuda"))
    new = evaluate_epoch(val, m, torch.device("cuda"))
    gap = abs(new["loss"] - old["loss"]) / abs(old["loss"])
    print(f"evaluate {old}\nevaluate_epoch {new}\nloss gap (new vs fp32 ce_kernel) {gap:.3e}")
    assert new["n"] == 4 and set(new) == {"acc1", "acc5", "global_acc1", "local_acc1", "loss", "n"}
    assert new["acc1"] == old["acc1"] and new["global_acc1"] == old["global_acc1"] and new["local_acc1"] == old["local_acc1"]
    assert gap <= 1e-5
    ce, hits5, n = 0.0, 0, 0
    with torch.no_grad():
        for x, y in val:
            logits = m.eval()(x)[0].cpu()
            ce += float(-torch.log_softmax(logits.double(), 1)[torch.arange(len(y)), y.cpu()].sum())
            hits5 += int((logits.topk(5, 1).indices == y.cpu()[:, None]).any(1).sum())
            n += len(y)
    assert abs(new["loss"] - ce / n) <= LOSS_RTOL * ce / n and new["acc5"] == 100.0 * hits5 / n


# ------------------------------------------------------------------------------------------------ the driver end to end
@pytest.fixture(scope="module", params=["eager", "replayed"])
def run(request, tree, tmp_path_factory):
    """Two epochs on the synthetic tree with the micro model, a checkpoint after each."""
    from protopformer_amd import train
    out = tmp_path_factory.mktemp("run_" + request.param)
    args = _args(tree, out, "--epochs", "2", "--save_ep_freq", "1", "--use_ppc_loss", "true", "--model_ema", "--step", request.param)
    records = train.main(args, model=_micro_model())
    return dict(kind=request.param, out=str(out), records=records)


def test_driver_two_epochs(run):
    from protopformer_amd.train import SCALARS
    rec, ck = run["records"], os.path.join(run["out"], "checkpoints")
    assert len(rec) == 2 and [r["epoch"] for r in rec] == [0, 1]
    assert all(math.isfinite(r["train_loss"]) and math.isfinite(r["test_loss"]) and r["test_n"] == 4 for r in rec)
    assert os.path.exists(os.path.join(ck, "checkpoint-0.pth")) and os.path.exists(os.path.join(ck, "checkpoint-1.pth"))
    best = os.path.exists(os.path.join(ck, "epoch-best.pth"))
    all_zero = all(r["test_acc1"] == 0.0 for r in rec)
    print(f"[{run['kind']}] acc1 per epoch {[r['test_acc1'] for r in rec]}: epoch-best.pth "
          + ("absent, acc1 was 0.0 in both epochs (as in the reference)" if all_zero else "written"))
    assert best == (not all_zero)
    lines = [json.loads(ln) for ln in open(os.path.join(run["out"], "train-logs", "scalars.jsonl"))]
    assert len(lines) == 2 and all(k in ln for ln in lines for k in SCALARS)
    assert lines[1]["epoch/val_acc1"] == rec[1]["test_acc1"] and lines[1]["epoch/train_loss"] == rec[1]["train_loss"]
    assert os.path.getsize(os.path.join(run["out"], "train-logs", "micro_deit_CUB2011U.log")) > 0
    saved = torch.load(os.path.join(ck, "checkpoint-0.pth"), map_location="cpu", weights_only=False)
    assert saved["epoch"] == 0 and saved["model_ema"] is not None and set(saved["model_ema"]) == set(saved["model"])


def test_driver_resume_runs_exactly_epoch_1(run, tree, tmp_path):
    from protopformer_amd import train
    ck0 = os.path.join(run["out"], "checkpoints", "checkpoint-0.pth")
    args = _args(tree, tmp_path, "--epochs", "2", "--save_ep_freq", "1", "--use_ppc_loss", "true", "--model_ema", "--step", run["kind"],
                 "--resume", ck0)
    rec = train.main(args, model=_micro_model())
    assert len(rec) == 1 and rec[0]["epoch"] == 1 and math.isfinite(rec[0]["train_loss"])
    assert rec[0]["train_lr"] == run["records"][1]["train_lr"]          # (the reference's scheduler off-by-one is kept)
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoints", "checkpoint-1.pth"))
    assert len(open(os.path.join(str(tmp_path), "train-logs", "scalars.jsonl")).readlines()) == 1


def test_driver_eval_only_reproduces_the_logged_metrics(run, tree, tmp_path):
    from protopformer_amd import train
    ck1 = os.path.join(run["out"], "checkpoints", "checkpoint-1.pth")
    stats = train.main(_args(tree, tmp_path, "--eval", "--resume", ck1, "--use_ppc_loss", "true"), model=_micro_model())
    want = run["records"][1]
    print(f"[{run['kind']}] --eval {stats} ; logged for epoch 1: acc1 {want['test_acc1']} acc5 {want['test_acc5']} loss {want['test_loss']!r}")
    assert stats["acc1"] == want["test_acc1"] and stats["acc5"] == want["test_acc5"] and stats["n"] == want["test_n"]
    assert stats["loss"] == want["test_loss"]                            # evaluation is deterministic: bit-identical
    assert os.path.isdir(os.path.join(str(tmp_path), "eval-logs"))


def test_driver_crosses_the_ppc_phase_boundary(tree, tmp_path):
    from protopformer_amd import train
    args = _args(tree, tmp_path, "--start_epoch", "19", "--epochs", "21", "--step", "replayed", "--use_ppc_loss", "true")
    rec = train.main(args, model=_micro_model())
    assert [r["epoch"] for r in rec] == [19, 20]
    assert all(math.isfinite(r["train_loss"]) and math.isfinite(r["test_loss"]) for r in rec)


def test_driver_refuses_mixup_with_ppc(tree, tmp_path):
    from protopformer_amd import train
    with pytest.raises(ValueError, match="use_ppc_loss"):
        train.main(_args(tree, tmp_path, "--epochs", "1", "--enable_mixup", "1", "--use_ppc_loss", "true"), model=_micro_model())


def test_driver_named_architecture(tree, tmp_path):
    """No model= : construct_PPNet builds deit_tiny (a BASELINE shape family) with seeded random weights; the checkpoint reads back."""
    from protopformer_amd import train
    from protopformer_amd.engine import load_checkpoint
    from protopformer_amd.protopformer import construct_PPNet
    from protopformer_amd.train import get_args_parser
    args = get_args_parser().parse_args(
        ["--data_set", "CUB2011U", "--data_path", tree, "--output_dir", str(tmp_path), "--base_architecture", "deit_tiny_patch16_224",
         "--no-pretrained", "--prototype_shape", "2000", "192", "1", "1", "--reserve_layers", "11", "--reserve_token_nums", "81",
         "--use_global", "true", "--use_ppc_loss", "true", "--global_proto_per_class", "10", "--input_size", "224", "--batch_size", "2",
         "--epochs", "1", "--save_ep_freq", "1", "--num_workers", "0"])
    rec = train.main(args)
    assert len(rec) == 1 and rec[0]["epoch"] == 0 and math.isfinite(rec[0]["train_loss"]) and rec[0]["test_n"] == 4
    path = os.path.join(str(tmp_path), "checkpoints", "checkpoint-0.pth")
    assert os.path.exists(path)
    fresh = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=[2000, 192, 1, 1], num_classes=200,
                            reserve_layers=[11], reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=10,
                            add_on_layers_type="regular")
    assert load_checkpoint(path, fresh, strict=True) == 0
    saved = torch.load(path, map_location="cpu", weights_only=False)
    assert all(torch.equal(v, saved["model"][k]) for k, v in fresh.state_dict().items())
