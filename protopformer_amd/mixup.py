"""Mixup / CutMix and the soft-target losses of the reference's training recipe (main.py:159-170, 257-258, 318-335, 382-390; timm 0.5.4
data/mixup.py and loss/cross_entropy.py) on the HIP kernels.

The parameter draws (lam, CutMix or blend, boxes) stay on the host and restate timm's public definitions of _params_per_batch,
_params_per_elem, rand_bbox, rand_bbox_minmax and cutmix_bbox_and_lam: they take the global np.random in timm's call order, so a seeded
run draws what timm draws.  The draws become one per-sample table (PPF_MIX_* of include/ppf_hip.h: kind, box, two fp32 weights rounded
the way timm's torch arithmetic rounds them) that reaches the device with one small pinned H2D copy per call; the in-place mixing
(ppf_mixup_apply) and the mixed, smoothed targets (ppf_mixup_target) are HIP kernels.  There is no CPU fallback.

The losses: SoftTargetCrossEntropy (main.py:384-386), LabelSmoothingCrossEntropy (main.py:387-388) and protopformer.CrossEntropyLoss
given [B, C] probability targets all run ppf_soft_cross_entropy."""
import numpy as np
import torch
import torch.nn as nn

from . import ops

MIX_WORDS = ops.MIX_WORDS
KIND, YL, YH, XL, XH, WSELF, WOTHER = range(7)          # PPF_MIX_KIND .. PPF_MIX_WOTHER
UNTOUCHED, BLEND, BOX = 0, 1, 2


def _bits(v):
    return int(np.array(v, dtype=np.float32).view(np.int32))


# ------------------------------------------------------------------------------------------------ parameter draws (timm 0.5.4)
def rand_bbox(img_shape, lam, margin=0., count=None, rng=None):
    """CutMix box of area ~(1 - lam), centre uniform, clipped at the border."""
    rng = np.random if rng is None else rng
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    margin_y, margin_x = int(margin * cut_h), int(margin * cut_w)
    cy = rng.randint(0 + margin_y, img_h - margin_y, size=count)
    cx = rng.randint(0 + margin_x, img_w - margin_x, size=count)
    yl = np.clip(cy - cut_h // 2, 0, img_h)
    yh = np.clip(cy + cut_h // 2, 0, img_h)
    xl = np.clip(cx - cut_w // 2, 0, img_w)
    xh = np.clip(cx + cut_w // 2, 0, img_w)
    return yl, yh, xl, xh


def rand_bbox_minmax(img_shape, minmax, count=None, rng=None):
    """CutMix box with side ratios uniform in [minmax[0], minmax[1]), fully inside the image."""
    rng = np.random if rng is None else rng
    assert len(minmax) == 2
    img_h, img_w = img_shape[-2:]
    cut_h = rng.randint(int(img_h * minmax[0]), int(img_h * minmax[1]), size=count)
    cut_w = rng.randint(int(img_w * minmax[0]), int(img_w * minmax[1]), size=count)
    yl = rng.randint(0, img_h - cut_h, size=count)
    xl = rng.randint(0, img_w - cut_w, size=count)
    return yl, yl + cut_h, xl, xl + cut_w


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None, rng=None):
    """Box and the lam corrected to the box's actual area (always when ratio_minmax is given)."""
    if ratio_minmax is not None:
        yl, yu, xl, xu = rand_bbox_minmax(img_shape, ratio_minmax, count=count, rng=rng)
    else:
        yl, yu, xl, xu = rand_bbox(img_shape, lam, count=count, rng=rng)
    if correct_lam or ratio_minmax is not None:
        bbox_area = (yu - yl) * (xu - xl)
        lam = 1. - bbox_area / float(img_shape[-2] * img_shape[-1])
    return (yl, yu, xl, xu), lam


class Mixup:
    """timm 0.5.4 Mixup (main.py:325-335): same constructor, same draws, same results; __call__(x, target) -> (x mixed in place, soft target
    [B, num_classes] fp32).  x must be a contiguous fp32 CUDA batch [B, C, H, W] of even size, target int class indices [B].
    rng: an np.random.RandomState to draw from instead of the global np.random."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000, rng=None):
        if mode not in ('batch', 'pair', 'elem'):
            raise ValueError(f"Mixup: mode must be 'batch', 'pair' or 'elem', not {mode!r}")
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0                      # timm: minmax forces CutMix on
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True                        # set to False by a train loop to stop mixing (targets stay smoothed one-hot)
        self.rng = rng
        self._ring = [[None, None] for _ in range(4)]    # pinned host tables + the event after their upload
        self._next = 0
        self._dev = None                                 # the device table (stream-ordered: one is enough)

    def _params_per_elem(self, batch_size):
        rng = np.random if self.rng is None else self.rng
        lam = np.ones(batch_size, dtype=np.float32)
        use_cutmix = np.zeros(batch_size, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = rng.rand(batch_size) < self.switch_prob
                lam_mix = np.where(use_cutmix, rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size),
                                   rng.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size))
            elif self.mixup_alpha > 0.:
                lam_mix = rng.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(batch_size, dtype=bool)
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size)
            else:
                raise ValueError("Mixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must hold")
            lam = np.where(rng.rand(batch_size) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        rng = np.random if self.rng is None else self.rng
        lam = 1.
        use_cutmix = False
        if self.mixup_enabled and rng.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = rng.rand() < self.switch_prob
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = rng.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam_mix = rng.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                raise ValueError("Mixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must hold")
            lam = float(lam_mix)
        return lam, use_cutmix

    def _box(self, H, W, lam):
        return cutmix_bbox_and_lam((H, W), lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam, rng=self.rng)

    def draw(self, B, H, W):
        """One call's draws as the per-sample table (int32 [B, MIX_WORDS]); consumes np.random exactly as timm's _mix_<mode> does.
        Weights: 'batch' mixes with lam a Python double (x.mul_(lam) / mul_(1. - lam): f32(lam), f32(1 - lam)); 'elem' / 'pair' with
        lam an np.float32 (x*lam + x_orig*(1 - lam): lam, 1 - lam in fp32).  For a CutMix sample they carry the corrected lam, which
        only the target uses."""
        t = np.zeros((B, MIX_WORDS), dtype=np.int32)
        t[:, WSELF] = _bits(1.0)

        def put(rows, kind, w_self, w_other, box=None):
            t[rows, KIND] = kind
            t[rows, WSELF], t[rows, WOTHER] = _bits(w_self), _bits(w_other)
            if box is not None:
                t[rows, YL], t[rows, YH], t[rows, XL], t[rows, XH] = (int(v) for v in box)

        if self.mode == 'batch':
            lam, use_cutmix = self._params_per_batch()
            if lam != 1.:
                box = None
                if use_cutmix:
                    box, lam = self._box(H, W, lam)
                put(slice(None), BOX if use_cutmix else BLEND, np.float32(lam), np.float32(1. - lam), box)
            return t
        n = B if self.mode == 'elem' else B // 2
        lam_batch, use_cutmix = self._params_per_elem(n)
        for i in range(n):
            lam = lam_batch[i]
            if lam == 1.:
                continue
            rows = [i] if self.mode == 'elem' else [i, B - 1 - i]
            box = None
            if use_cutmix[i]:
                box, lam = self._box(H, W, lam)
                lam_batch[i] = lam                       # stored into the float32 array: the target's lam
            w = np.float32(lam_batch[i])
            put(rows, BOX if use_cutmix[i] else BLEND, w, np.float32(1.) - w, box)
        return t

    def _host_slot(self, n):
        slot = self._ring[self._next]
        self._next = (self._next + 1) % len(self._ring)
        if slot[1] is not None:
            slot[1].synchronize()                        # the upload that last read this buffer has run
        if slot[0] is None or slot[0].numel() < n:
            slot[0] = torch.empty(n, dtype=torch.int32, pin_memory=True)
        return slot

    def __call__(self, x, target):
        if len(x) % 2 != 0:
            raise ValueError("Mixup: batch size should be even when using this")
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4):
            raise RuntimeError("Mixup: x must be a contiguous fp32 CUDA tensor [B, C, H, W] (the mixing is a HIP kernel, "
                               "there is no CPU fallback)")
        if target.is_floating_point() or target.dim() != 1 or target.shape[0] != x.shape[0] or target.device != x.device:
            raise ValueError(f"Mixup: target must be integer class indices [B] on {x.device}, got {tuple(target.shape)} "
                             f"{target.dtype} on {target.device}")
        B, _, H, W = x.shape
        table = self.draw(B, H, W)
        slot = self._host_slot(B * MIX_WORDS)
        host = slot[0]
        host.numpy()[:B * MIX_WORDS] = table.reshape(-1)
        if self._dev is None or self._dev.numel() < B * MIX_WORDS or self._dev.device != x.device:
            self._dev = torch.empty(B * MIX_WORDS, dtype=torch.int32, device=x.device)
        ops.mixup_apply(x, host, self._dev)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record()
        off_value = self.label_smoothing / self.num_classes          # timm mixup_target: doubles, rounded to fp32 by torch.full / scatter_
        on_value = 1. - self.label_smoothing + off_value
        return x, ops.mixup_target(target.long().contiguous(), self._dev, self.num_classes, off_value, on_value)


# ------------------------------------------------------------------------------------------------ losses
class SoftCrossEntropyFn(torch.autograd.Function):
    """Mean cross-entropy against a dense target (label None) or int64 labels with smoothing (target None); no gradient to the target."""

    @staticmethod
    def forward(ctx, logits, target, label, smoothing):
        loss, dlogits = ops.soft_cross_entropy(logits.contiguous(), target, label, smoothing)
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, up):
        (dlogits,) = ctx.saved_tensors
        if ops.is_const_one(up):                                                    # seeded by the train loop's cached one: nothing to scale
            return dlogits, None, None, None
        return ops.scale_by_scalar(dlogits, up.float().contiguous()), None, None, None


def dense_target(logits, target):
    """A [B, C] floating-point target as the kernel's fp32 contiguous operand; anything else is refused (the kernel would misread it)."""
    if not target.is_floating_point() or target.dim() != 2 or tuple(target.shape) != tuple(logits.shape):
        raise ValueError(f"soft-target cross-entropy needs a floating-point target of the logits' shape {tuple(logits.shape)}, got "
                         f"{tuple(target.shape)} {target.dtype}")
    return target.float().contiguous()


class SoftTargetCrossEntropy(nn.Module):
    """timm SoftTargetCrossEntropy (main.py:384-386): mean_b sum_c -t_bc log_softmax(x_b)_c."""

    def forward(self, x, target):
        return SoftCrossEntropyFn.apply(x, dense_target(x, target), None, 0.0)


class LabelSmoothingCrossEntropy(nn.Module):
    """timm LabelSmoothingCrossEntropy (main.py:387-388): mean_b (1-s) nll_b + s mean_c(-log_softmax(x_b)_c)."""

    def __init__(self, smoothing=0.1):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"LabelSmoothingCrossEntropy: smoothing must be in [0, 1), got {smoothing}")
        self.smoothing = smoothing
        self.confidence = 1. - smoothing

    def forward(self, x, target):
        if target.is_floating_point() or target.dim() != 1:
            raise ValueError(f"LabelSmoothingCrossEntropy needs integer class indices [B], got {tuple(target.shape)} {target.dtype}")
        return SoftCrossEntropyFn.apply(x, None, target.long().contiguous(), self.smoothing)


# ------------------------------------------------------------------------------------------------ main.py's selection
def _smoothing(args):
    """main.py:257-258, 319-324: --enable_smoothing sets smoothing 0.1; without it any other smoothing is refused."""
    if getattr(args, "enable_smoothing", False):
        return 0.1
    s = getattr(args, "smoothing", 0.0)
    if s != 0:
        raise ValueError(f"smoothing {s} without enable_smoothing (the reference asserts smoothing == 0 then)")
    return 0.0


def create_mixup(args):
    """mixup_fn of main.py:318-335: a Mixup when enable_mixup and one of mixup > 0, cutmix > 0, cutmix_minmax is set; else None."""
    smoothing = _smoothing(args)
    mixup, cutmix, minmax = getattr(args, "mixup", 0.0), getattr(args, "cutmix", 1.0), getattr(args, "cutmix_minmax", None)
    if not getattr(args, "enable_mixup", False):
        if mixup != 0.0:
            raise ValueError(f"mixup {mixup} without enable_mixup (the reference asserts mixup == 0 then)")
        return None
    if not (mixup > 0 or cutmix > 0. or minmax is not None):
        return None
    if getattr(args, "use_ppc_loss", False):
        raise ValueError("mixup / CutMix together with use_ppc_loss: the PPC loss needs integer class labels (it selects each sample's "
                         "prototypes by its label) and Mixup turns the targets into [B, C] mixtures; the reference fails on this "
                         "combination as well.  Turn one of the two off.")
    return Mixup(mixup_alpha=mixup, cutmix_alpha=cutmix, cutmix_minmax=minmax, prob=getattr(args, "mixup_prob", 1.0),
                 switch_prob=getattr(args, "mixup_switch_prob", 0.5), mode=getattr(args, "mixup_mode", "batch"),
                 label_smoothing=smoothing, num_classes=args.nb_classes)


def create_criterion(args):
    """criterion of main.py:382-390: SoftTargetCrossEntropy when mixup > 0, else LabelSmoothingCrossEntropy(smoothing) when smoothing,
    else nn.CrossEntropyLoss (protopformer.CrossEntropyLoss, which also takes the [B, C] targets of CutMix-only Mixup)."""
    from .protopformer import CrossEntropyLoss
    smoothing = _smoothing(args)
    if getattr(args, "mixup", 0.0) > 0.:
        return SoftTargetCrossEntropy()
    if smoothing:
        return LabelSmoothingCrossEntropy(smoothing=smoothing)
    return CrossEntropyLoss()
