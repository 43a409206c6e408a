"""Mixup / CutMix kernels and the soft-target / label-smoothing cross-entropy on the MI355X: the in-place mixing bit-exact against timm
0.5.4's torch arithmetic (restated here, run on a clone), the mixed targets, the losses against fp64 torch, and the train step with
mixed batches (eager == recorded command list, bit for bit; train_one_epoch with create_mixup)."""
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import build_micro, micro
from test_mixup_cpu import TimmDraws, t_cutmix_bbox_and_lam

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ timm 0.5.4 mixing, restated in torch
def t_one_hot(x, num_classes, on_value=1., off_value=0., device='cuda'):
    x = x.long().view(-1, 1)
    return torch.full((x.size()[0], num_classes), off_value, device=device).scatter_(1, x, on_value)


def t_mixup_target(target, num_classes, lam=1., smoothing=0.0, device='cuda'):
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    y1 = t_one_hot(target, num_classes, on_value=on_value, off_value=off_value, device=device)
    y2 = t_one_hot(target.flip(0), num_classes, on_value=on_value, off_value=off_value, device=device)
    return y1 * lam + y2 * (1. - lam)


class TimmMixup(TimmDraws):
    def __init__(self, label_smoothing=0.1, num_classes=1000, **kw):
        super().__init__(**kw)
        self.label_smoothing, self.num_classes = label_smoothing, num_classes

    def _mix_elem(self, x):
        batch_size = len(x)
        lam_batch, use_cutmix = self._params_per_elem(batch_size)
        x_orig = x.clone()
        for i in range(batch_size):
            j = batch_size - i - 1
            lam = lam_batch[i]
            if lam != 1.:
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(x[i].shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                    x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
                    lam_batch[i] = lam
                else:
                    x[i] = x[i] * lam + x_orig[j] * (1 - lam)
        return torch.tensor(lam_batch, device=x.device, dtype=x.dtype).unsqueeze(1)

    def _mix_pair(self, x):
        batch_size = len(x)
        lam_batch, use_cutmix = self._params_per_elem(batch_size // 2)
        x_orig = x.clone()
        for i in range(batch_size // 2):
            j = batch_size - i - 1
            lam = lam_batch[i]
            if lam != 1.:
                if use_cutmix[i]:
                    (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(x[i].shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                    x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
                    x[j][:, yl:yh, xl:xh] = x_orig[i][:, yl:yh, xl:xh]
                    lam_batch[i] = lam
                else:
                    x[i] = x[i] * lam + x_orig[j] * (1 - lam)
                    x[j] = x[j] * lam + x_orig[i] * (1 - lam)
        lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
        return torch.tensor(lam_batch, device=x.device, dtype=x.dtype).unsqueeze(1)

    def _mix_batch(self, x):
        lam, use_cutmix = self._params_per_batch()
        if lam == 1.:
            return 1.
        if use_cutmix:
            (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(x.shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        else:
            x_flipped = x.flip(0).mul_(1. - lam)
            x.mul_(lam).add_(x_flipped)
        return lam

    def __call__(self, x, target):
        assert len(x) % 2 == 0
        lam = self._mix_elem(x) if self.mode == 'elem' else self._mix_pair(x) if self.mode == 'pair' else self._mix_batch(x)
        return x, t_mixup_target(target, self.num_classes, lam, self.label_smoothing)


def _ulps(a, b):
    ia = a.contiguous().view(torch.int32).long()
    ib = b.contiguous().view(torch.int32).long()
    return int((ia - ib).abs().max())


KINDS = {"blend": dict(mixup_alpha=0.8, cutmix_alpha=0.0), "box": dict(mixup_alpha=0.0, cutmix_alpha=1.0)}


# ------------------------------------------------------------------------------------------------ 1. + 2. mixing and targets
@pytest.mark.parametrize("B", [2, 6, 64])
@pytest.mark.parametrize("hw", [(224, 224), (37, 53)])
def test_mixing_bit_exact_against_timm(B, hw):
    from protopformer_amd.mixup import Mixup
    H, W = hw
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H)
    x0 = torch.randn(B, 3, H, W, device="cuda", generator=g)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    for mode in ("batch", "pair", "elem"):
        for kind, kw in KINDS.items():
            for seed, extra in ((1, {}), (2, dict(prob=0.5)), (3, dict(correct_lam=False))):
                for smoothing in (0.0, 0.1):
                    np.random.seed(seed)
                    x, t = Mixup(mode=mode, label_smoothing=smoothing, num_classes=10, **kw, **extra)(x0.clone(), y)
                    np.random.seed(seed)
                    xr, tr = TimmMixup(mode=mode, label_smoothing=smoothing, num_classes=10, **kw, **extra)(x0.clone(), y)
                    what = (mode, kind, seed, smoothing)
                    assert torch.equal(x, xr), what
                    assert t.dtype == torch.float32 and t.shape == (B, 10) and _ulps(t, tr.float()) <= 1, what


def _table(rows):
    from protopformer_amd import mixup as M
    t = np.zeros((len(rows), M.MIX_WORDS), np.int32)
    for i, r in enumerate(rows):
        kind, box, ws, wo = r
        t[i, M.KIND] = kind
        t[i, M.YL:M.XH + 1] = box
        t[i, M.WSELF], t[i, M.WOTHER] = M._bits(ws), M._bits(wo)
    return t


def _apply(x, table):
    from protopformer_amd import ops
    host = torch.from_numpy(table.reshape(-1).copy()).pin_memory()
    dev = torch.empty(host.numel(), dtype=torch.int32, device=x.device)
    ops.mixup_apply(x, host, dev)
    torch.cuda.synchronize()
    return dev


def _restate(x_orig, table):
    """The kernel's contract in torch fp32 on a clone: blend x_i*ws + x_j*wo, box paste of x_j, kind 0 untouched (j = B-1-i, pre-call)."""
    from protopformer_amd import mixup as M
    x = x_orig.clone()
    B = x.shape[0]
    for i in range(B):
        j = B - 1 - i
        r = table[i]
        ws, wo = (float(np.array(r[k], np.int32).view(np.float32)) for k in (M.WSELF, M.WOTHER))
        if r[M.KIND] == M.BLEND:
            x[i] = x_orig[i] * ws + x_orig[j] * wo
        elif r[M.KIND] == M.BOX:
            yl, yh, xl, xh = (int(v) for v in r[M.YL:M.XH + 1])
            x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
    return x


@pytest.mark.parametrize("hw", [(224, 224), (37, 53)])
def test_mixing_kernel_boxes_and_untouched_samples(hw):
    """Hand-made tables: boxes clipped at the border, empty (yl == yh / xl == xh), the whole image; blends and untouched samples in the
    same batch, pairs of different kinds.  Everything outside the boxes and every kind-0 sample is unchanged bit for bit."""
    H, W = hw
    rows = [
        (2, (0, H // 3, W - 5, W), 0.7, 0.3),            # 0: clipped at the top-right border, ragged column range (partner 10)
        (1, (0, 0, 0, 0), 0.6180339, 1 - 0.6180339),     # 1: blend
        (0, (0, 0, 0, 0), 1.0, 0.0),                     # 2: untouched
        (2, (5, 5, 1, W - 1), 0.5, 0.5),                 # 3: empty rows
        (2, (1, H - 1, 7, 7), 0.5, 0.5),                 # 4: empty columns
        (1, (0, 0, 0, 0), 0.25, 0.75),                   # 5: odd B, the middle sample blends with itself
        (2, (0, H, 0, W), 0.0, 1.0),                     # 6: the whole image (partner 4)
        (2, (H - 3, H, 0, 3), 0.9, 0.1),                 # 7: clipped at the bottom-left corner
        (0, (0, 0, 0, 0), 1.0, 0.0),                     # 8: untouched
        (2, (2, 9, 3, 4), 0.5, 0.5),                     # 9: one column
        (1, (0, 0, 0, 0), 0.125, 0.875),                 # 10
    ]
    B = len(rows)
    table = _table(rows)
    g = torch.Generator(device="cuda").manual_seed(7)
    x0 = torch.randn(B, 3, H, W, device="cuda", generator=g)
    x = x0.clone()
    _apply(x, table)
    ref = _restate(x0, table)
    assert torch.equal(x, ref)
    assert torch.equal(x[2], x0[2]) and torch.equal(x[8], x0[8])
    assert torch.equal(x[3], x0[3]) and torch.equal(x[4], x0[4])
    assert torch.equal(x[6], x0[4])
    mask = torch.ones(H, W, dtype=torch.bool, device="cuda")
    mask[0:H // 3, W - 5:W] = False
    assert torch.equal(x[0][:, mask], x0[0][:, mask]) and torch.equal(x[0][:, ~mask], x0[B - 1][:, ~mask])
    # all kinds 0: the batch is not touched
    x = x0.clone()
    _apply(x, _table([(0, (0, 0, 0, 0), 1.0, 0.0)] * B))
    assert torch.equal(x, x0)


def test_mixup_target_kernel():
    """ppf_mixup_target against timm's mixup_target: one lam for the batch (stride 0) and per-sample lam, smoothing 0 and 0.1."""
    from protopformer_amd import _lib
    B, C = 6, 1001
    g = torch.Generator(device="cuda").manual_seed(3)
    y = torch.randint(0, C, (B,), device="cuda", generator=g)
    y[1] = y[B - 2]                                      # a pair with equal labels
    for s in (0.0, 0.1):
        off, on = s / C, 1. - s + s / C
        for lam in (0.3141592653589793, 1.0, 0.0):
            w = torch.tensor([lam, 1. - lam], dtype=torch.float32, device="cuda")
            t = torch.empty(B, C, device="cuda")
            _lib.call("ppf_mixup_target", y, w, 0, off, on, t, B, C)
            assert _ulps(t, t_mixup_target(y, C, lam, s)) <= 1, (s, lam)
        lam32 = torch.rand(B, 1, device="cuda", generator=g)
        w = torch.cat([lam32, 1. - lam32], 1).contiguous()
        t = torch.empty(B, C, device="cuda")
        _lib.call("ppf_mixup_target", y, w, 2, off, on, t, B, C)
        assert _ulps(t, t_mixup_target(y, C, lam32, s)) <= 1, s


# ------------------------------------------------------------------------------------------------ 3. - 5. losses
def _check_loss(fn, logits, ref_fn, rtol=1e-5, atol_g=1e-7, up=1.0):
    x = logits.clone().requires_grad_(True)
    loss = fn(x)
    (up * loss).backward()
    x64 = logits.double().cpu().requires_grad_(True)
    ref = ref_fn(x64)
    (up * ref).backward()
    l, r = float(loss), float(ref)
    assert math.isfinite(l) and abs(l - r) <= rtol * abs(r), (l, r)
    gerr = float((x.grad.double().cpu() - x64.grad).abs().max())
    assert gerr <= atol_g, gerr
    return loss


@pytest.mark.parametrize("B", [1, 3, 256])
@pytest.mark.parametrize("C", [1, 2, 200, 1000, 1001])
def test_soft_target_ce_against_fp64(B, C):
    from protopformer_amd.mixup import SoftTargetCrossEntropy
    g = torch.Generator(device="cuda").manual_seed(B * 7 + C)
    crit = SoftTargetCrossEntropy()
    logits = torch.randn(B, C, device="cuda", generator=g) * 3
    probs = torch.softmax(torch.randn(B, C, device="cuda", generator=g), 1)
    _check_loss(lambda x: crit(x, probs), logits, lambda x: F.cross_entropy(x, probs.double().cpu()))
    # targets that do not sum to one (torch does not normalise them either)
    t = torch.rand(B, C, device="cuda", generator=g) * 1.7 / C
    _check_loss(lambda x: crit(x, t), logits, lambda x: F.cross_entropy(x, t.double().cpu()))
    # logits of +-3e4: finite and still right
    big = (torch.rand(B, C, device="cuda", generator=g) * 2 - 1) * 3e4
    _check_loss(lambda x: crit(x, probs), big, lambda x: F.cross_entropy(x, probs.double().cpu()))
    near = 3e4 - torch.rand(B, C, device="cuda", generator=g) * 3           # all logits near 3e4: lse*sum(t) - sum(t*x) would cancel
    _check_loss(lambda x: crit(x, probs), near, lambda x: F.cross_entropy(x, probs.double().cpu()))


@pytest.mark.parametrize("B,C", [(1, 200), (3, 1001), (256, 200)])
def test_label_smoothing_ce_against_fp64(B, C):
    from protopformer_amd.mixup import LabelSmoothingCrossEntropy
    from protopformer_amd.protopformer import CrossEntropyLoss
    g = torch.Generator(device="cuda").manual_seed(B + C)
    logits = torch.randn(B, C, device="cuda", generator=g) * 3
    y = torch.randint(0, C, (B,), device="cuda", generator=g)
    for s in (0.1, 0.3):
        crit = LabelSmoothingCrossEntropy(smoothing=s)
        _check_loss(lambda x: crit(x, y), logits, lambda x: F.cross_entropy(x, y.cpu(), label_smoothing=s))
        # an upstream != 1 scales the gradient
        _check_loss(lambda x: crit(x, y), logits, lambda x: F.cross_entropy(x, y.cpu(), label_smoothing=s), up=3.0, atol_g=4e-7)
    big = (torch.rand(B, C, device="cuda", generator=g) * 2 - 1) * 3e4
    crit = LabelSmoothingCrossEntropy(smoothing=0.1)
    _check_loss(lambda x: crit(x, y), big, lambda x: F.cross_entropy(x, y.cpu(), label_smoothing=0.1))
    # s = 0 is the plain cross-entropy of the existing kernel
    l0 = float(LabelSmoothingCrossEntropy(smoothing=0.0)(logits, y))
    lc = float(CrossEntropyLoss()(logits, y))
    assert abs(l0 - lc) <= 1e-6 * abs(lc), (l0, lc)


def test_cross_entropy_loss_takes_probability_targets():
    from protopformer_amd import ops
    from protopformer_amd.mixup import SoftTargetCrossEntropy
    from protopformer_amd.protopformer import CrossEntropyLoss
    g = torch.Generator(device="cuda").manual_seed(11)
    B, C = 8, 200
    logits = torch.randn(B, C, device="cuda", generator=g)
    probs = torch.softmax(torch.randn(B, C, device="cuda", generator=g), 1)
    grads = []
    for crit in (CrossEntropyLoss(), SoftTargetCrossEntropy()):
        x = logits.clone().requires_grad_(True)
        loss = crit(x, probs)
        (2.0 * loss).backward()
        grads.append((loss.detach(), x.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    ref = F.cross_entropy(logits.double(), probs.double())
    assert abs(float(grads[0][0]) - float(ref)) <= 1e-5 * abs(float(ref))
    # int labels: exactly the existing kernel (ppf_cross_entropy), untouched
    y = torch.randint(0, C, (B,), device="cuda", generator=g)
    loss_ref, dl_ref = ops.cross_entropy(logits, y)
    x = logits.clone().requires_grad_(True)
    loss = CrossEntropyLoss()(x, y)
    loss.backward(gradient=ops.const_scalar(loss.device, 1.0))
    assert torch.equal(loss.detach(), loss_ref[0]) and torch.equal(x.grad, dl_ref)


# ------------------------------------------------------------------------------------------------ 6. - 8. training
def _deit(use_ppc):
    from protopformer_amd import backbone
    from protopformer_amd.engine import FlatAdamW
    from protopformer_amd.protopformer import construct_PPNet
    backbone._KEEP_CACHE.clear()
    torch.manual_seed(3)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, img_size=224, prototype_shape=(200, 64, 1, 1), num_classes=20,
                        reserve_layers=[11], reserve_token_nums=[81], use_global=True, use_ppc_loss=use_ppc, global_proto_per_class=5,
                        add_on_layers_type="regular").cuda().train()
    return m, FlatAdamW(m, weight_decay=0.05, ema_decay=0.999)


@pytest.mark.parametrize("variant", ["mixup-soft-target", "label-smoothing-ppc"])
def test_replayed_step_with_mixed_batches_equals_eager(variant):
    """Six batches, each mixed by the same seeded draws before the step: the eager step and the recorded command list (warm-up 2,
    dense [B, C] targets copied into its static buffer) give bit-identical losses, parameters, moments and EMA."""
    from protopformer_amd.engine import ReplayedTrainStep, train_one_step
    from protopformer_amd.mixup import LabelSmoothingCrossEntropy, Mixup, SoftTargetCrossEntropy
    use_ppc = variant == "label-smoothing-ppc"
    g = torch.Generator(device="cuda").manual_seed(9)
    batches = [(torch.randn(6, 3, 224, 224, device="cuda", generator=g), torch.randint(0, 20, (6,), device="cuda", generator=g)) for _ in range(6)]
    if use_ppc:
        crit, mix = LabelSmoothingCrossEntropy(0.1), None
    else:
        crit, mix = SoftTargetCrossEntropy(), Mixup(0.8, 1.0, label_smoothing=0.1, mode='batch', num_classes=20)

    def inputs(i):
        x, y = batches[i][0].clone(), batches[i][1]
        if mix is None:
            return x, y
        np.random.seed(50 + i)
        return mix(x, y)

    a, opt_a = _deit(use_ppc)
    la = [float(train_one_step(a, crit, *inputs(i), opt_a, epoch=20, max_norm=1.0, use_ppc_loss=use_ppc)[0]) for i in range(6)]
    b, opt_b = _deit(use_ppc)
    rs = ReplayedTrainStep(b, crit, opt_b, epoch=20, max_norm=1.0, warmup=2, use_ppc_loss=use_ppc)
    lb = [float(rs(*inputs(i))[0]) for i in range(6)]
    torch.cuda.synchronize()
    assert rs.rec is not None and len(rs.rec.cmds) > 100
    if mix is not None:
        assert rs.static_in[1].shape == (6, 20) and rs.static_in[1].is_floating_point()
    assert all(math.isfinite(v) for v in la) and len(set(la)) == 6
    assert la == lb, (la, lb)
    assert torch.equal(a.flat_store().params, b.flat_store().params) and torch.equal(opt_a.exp_avg, opt_b.exp_avg)
    assert torch.equal(opt_a.ema, opt_b.ema)


def test_train_one_epoch_with_mixup(tmp_path):
    import os
    from test_data_cpu import _jpeg
    from protopformer_amd import data as D
    from protopformer_amd.engine import FlatAdamW, evaluate, train_one_epoch
    from protopformer_amd.mixup import Mixup, create_criterion, create_mixup
    from protopformer_amd.protopformer import CrossEntropyLoss
    meta = tmp_path / "CUB_200_2011"
    os.makedirs(meta / "images")
    rows = []
    for i in range(1, 17):
        cls = (i - 1) % 10 + 1
        fp = f"{cls:03d}.B/{i:04d}.jpg"
        _jpeg(str(meta / "images" / fp), 90 + i, 70 + i, i)
        rows.append((i, fp, cls, 1 if i <= 12 else 0))
    (meta / "images.txt").write_text("".join(f"{i} {fp}\n" for i, fp, _, _ in rows))
    (meta / "image_class_labels.txt").write_text("".join(f"{i} {c}\n" for i, _, c, _ in rows))
    (meta / "train_test_split.txt").write_text("".join(f"{i} {t}\n" for i, _, _, t in rows))
    sd, cfg, z = micro("micro_deit.npz")                              # 64x64 inputs, 10 classes
    args = types.SimpleNamespace(input_size=64, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="CUB2011U",
                                 data_path=str(tmp_path), batch_size=4, num_workers=0, reprob=0.25,
                                 enable_mixup=True, enable_smoothing=True, mixup=0.0, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0,
                                 mixup_switch_prob=0.5, mixup_mode="batch", smoothing=0.0, nb_classes=10, use_ppc_loss=False)
    train, val, _ = D.build_loaders(args, torch.device("cuda"))
    mixup_fn, crit = create_mixup(args), create_criterion(args)
    assert isinstance(mixup_fn, Mixup) and mixup_fn.label_smoothing == 0.1
    args.enable_smoothing = False                                     # CutMix-only under the flag defaults: nn.CrossEntropyLoss, probability targets
    crit = create_criterion(args)
    assert type(crit) is CrossEntropyLoss
    m = build_micro(cfg, sd)
    opt = FlatAdamW(m, weight_decay=0.05)
    np.random.seed(0)
    seen = []
    orig_call = mixup_fn.__call__

    def spy(x, y):
        x, t = orig_call(x, y)
        seen.append(t.shape)
        return x, t
    stats = train_one_epoch(m, crit, train, opt, torch.device("cuda"), epoch=20, args=args, log_every=1, logger=lambda s: None, mixup_fn=spy)
    assert np.isfinite(stats["loss"]) and seen == [(4, 10)] * 3
    acc = evaluate(val, m, torch.device("cuda"))
    assert 0.0 <= acc["acc1"] <= 100.0 and np.isfinite(acc["loss"])


def test_ppc_with_soft_targets_raises_before_any_launch():
    from protopformer_amd import _lib
    from protopformer_amd.engine import FlatAdamW, train_one_step
    from protopformer_amd.mixup import Mixup, SoftTargetCrossEntropy
    sd, cfg, z = micro("micro_deit.npz")
    m = build_micro(cfg, sd).train()
    img, label = torch.from_numpy(z["img"]).cuda(), torch.from_numpy(z["label"]).cuda()
    with torch.no_grad():
        logits, aux = m(img)
    np.random.seed(1)
    x, soft = Mixup(0.8, 1.0, num_classes=10)(img.clone(), label)
    torch.cuda.synchronize()
    rec = _lib.start_recording()
    try:
        with pytest.raises(ValueError, match="integer class labels"):
            m.get_PPC_loss(aux[2], aux[3], aux[4], soft)
        with pytest.raises(ValueError, match="integer class labels"):
            m.get_PPC_loss(aux[2], aux[3], aux[4], soft.argmax(1).float())
    finally:
        _lib.stop_recording()
    assert rec.cmds == []                                              # nothing was launched
    with pytest.raises(ValueError, match="integer class labels"):
        train_one_step(m, SoftTargetCrossEntropy(), x, soft, FlatAdamW(m), epoch=20, use_ppc_loss=True)
