"""Mixup / CutMix and the soft-target losses without a GPU: the host-side parameter draws against a restatement of timm 0.5.4's
(seeded np.random, same call order), the flag mapping of main.py:257-258, 318-335, 382-390 (create_mixup / create_criterion), the
refusals (odd batch, PPC with soft targets, malformed targets) and the C entry points' argument validation."""
import ctypes
import types

import numpy as np
import pytest
import torch

from protopformer_amd import mixup as M


# ------------------------------------------------------------------------------------------------ timm 0.5.4, restated
# (data/mixup.py: rand_bbox, rand_bbox_minmax, cutmix_bbox_and_lam, Mixup._params_per_elem / _params_per_batch / _mix_elem / _mix_pair /
# _mix_batch; the statements that write x are replaced by a record of what they would do)
def t_rand_bbox(img_shape, lam, margin=0., count=None):
    ratio = np.sqrt(1 - lam)
    img_h, img_w = img_shape[-2:]
    cut_h, cut_w = int(img_h * ratio), int(img_w * ratio)
    margin_y, margin_x = int(margin * cut_h), int(margin * cut_w)
    cy = np.random.randint(0 + margin_y, img_h - margin_y, size=count)
    cx = np.random.randint(0 + margin_x, img_w - margin_x, size=count)
    yl = np.clip(cy - cut_h // 2, 0, img_h)
    yh = np.clip(cy + cut_h // 2, 0, img_h)
    xl = np.clip(cx - cut_w // 2, 0, img_w)
    xh = np.clip(cx + cut_w // 2, 0, img_w)
    return yl, yh, xl, xh


def t_rand_bbox_minmax(img_shape, minmax, count=None):
    img_h, img_w = img_shape[-2:]
    cut_h = np.random.randint(int(img_h * minmax[0]), int(img_h * minmax[1]), size=count)
    cut_w = np.random.randint(int(img_w * minmax[0]), int(img_w * minmax[1]), size=count)
    yl = np.random.randint(0, img_h - cut_h, size=count)
    xl = np.random.randint(0, img_w - cut_w, size=count)
    return yl, yl + cut_h, xl, xl + cut_w


def t_cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True, count=None):
    if ratio_minmax is not None:
        yl, yu, xl, xu = t_rand_bbox_minmax(img_shape, ratio_minmax, count=count)
    else:
        yl, yu, xl, xu = t_rand_bbox(img_shape, lam, count=count)
    if correct_lam or ratio_minmax is not None:
        bbox_area = (yu - yl) * (xu - xl)
        lam = 1. - bbox_area / float(img_shape[-2] * img_shape[-1])
    return (yl, yu, xl, xu), lam


class TimmDraws:
    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if cutmix_minmax is not None:
            self.cutmix_alpha = 1.0
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam, self.mixup_enabled = prob, switch_prob, mode, correct_lam, True

    def _params_per_elem(self, batch_size):
        lam = np.ones(batch_size, dtype=np.float32)
        use_cutmix = np.zeros(batch_size, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand(batch_size) < self.switch_prob
                lam_mix = np.where(use_cutmix, np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size),
                                   np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size))
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=batch_size)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(batch_size, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=batch_size)
            lam = np.where(np.random.rand(batch_size) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _params_per_batch(self):
        lam = 1.
        use_cutmix = False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand() < self.switch_prob
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else \
                    np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            lam = float(lam_mix)
        return lam, use_cutmix

    def run(self, shape):
        """-> (ops, lam): ops = [(i, j, 'blend', lam_used) | (i, j, 'box', (yl, yh, xl, xh))], lam = the lam handed to mixup_target."""
        B = shape[0]
        ops = []
        if self.mode == 'elem':
            lam_batch, use_cutmix = self._params_per_elem(B)
            for i in range(B):
                j = B - i - 1
                lam = lam_batch[i]
                if lam != 1.:
                    if use_cutmix[i]:
                        (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(shape[1:], lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                        ops.append((i, j, 'box', (yl, yh, xl, xh)))
                        lam_batch[i] = lam
                    else:
                        ops.append((i, j, 'blend', lam))
            return ops, lam_batch
        if self.mode == 'pair':
            lam_batch, use_cutmix = self._params_per_elem(B // 2)
            for i in range(B // 2):
                j = B - i - 1
                lam = lam_batch[i]
                if lam != 1.:
                    if use_cutmix[i]:
                        (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(shape[1:], lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
                        ops += [(i, j, 'box', (yl, yh, xl, xh)), (j, i, 'box', (yl, yh, xl, xh))]
                        lam_batch[i] = lam
                    else:
                        ops += [(i, j, 'blend', lam), (j, i, 'blend', lam)]
            return ops, np.concatenate((lam_batch, lam_batch[::-1]))
        lam, use_cutmix = self._params_per_batch()
        if lam == 1.:
            return ops, 1.
        if use_cutmix:
            (yl, yh, xl, xh), lam = t_cutmix_bbox_and_lam(shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
            ops += [(i, B - 1 - i, 'box', (yl, yh, xl, xh)) for i in range(B)]
        else:
            ops += [(i, B - 1 - i, 'blend', lam) for i in range(B)]
        return ops, lam


def expected_table(ops, lam, B, mode):
    """The per-sample table the port must produce for timm's draws: kinds and boxes from the ops, weights as timm's torch arithmetic
    rounds them ('batch': Python double lam -> f32(lam), f32(1 - lam); 'elem' / 'pair': np.float32 lam -> lam, 1 - lam in fp32)."""
    t = np.zeros((B, M.MIX_WORDS), np.int32)
    t[:, M.WSELF] = M._bits(1.0)
    for i, j, kind, arg in ops:
        t[i, M.KIND] = M.BOX if kind == 'box' else M.BLEND
        if kind == 'box':
            t[i, M.YL:M.XH + 1] = [int(v) for v in arg]
    if mode == 'batch':
        if lam != 1.:
            t[:, M.WSELF], t[:, M.WOTHER] = M._bits(np.float32(lam)), M._bits(np.float32(1. - lam))
    else:
        for i in range(B):
            if t[i, M.KIND] != 0:
                w = np.float32(lam[i])
                t[i, M.WSELF], t[i, M.WOTHER] = M._bits(w), M._bits(np.float32(1.) - w)
    return t


CONFIGS = [
    dict(mixup_alpha=0.8, cutmix_alpha=0.0),                                   # mixup only
    dict(mixup_alpha=0.0, cutmix_alpha=1.0),                                   # CutMix only (main.py's flag defaults)
    dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5),                  # both, switched
    dict(mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5, correct_lam=False),
    dict(mixup_alpha=0.0, cutmix_alpha=0.0, cutmix_minmax=(0.2, 0.8)),         # minmax forces CutMix
    dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.3, 0.9), correct_lam=False),
    dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),                         # some draws leave samples / batches untouched
]


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("cfg", range(len(CONFIGS)))
def test_draws_match_timm(mode, cfg):
    kw = CONFIGS[cfg]
    B, H, W = 8, 37, 53
    port = M.Mixup(mode=mode, num_classes=10, **kw)
    ref = TimmDraws(mode=mode, **kw)
    kinds = set()
    for seed in range(12):
        np.random.seed(seed)
        got = port.draw(B, H, W)
        after_port = np.random.rand()
        np.random.seed(seed)
        ops, lam = ref.run((B, 3, H, W))
        after_ref = np.random.rand()
        want = expected_table(ops, lam, B, mode)
        assert np.array_equal(got, want), (seed, got, want)
        assert after_port == after_ref                                        # the same number of draws from the global stream
        kinds |= set(got[:, M.KIND].tolist())
        box = got[got[:, M.KIND] == M.BOX]
        assert (box[:, M.YL] >= 0).all() and (box[:, M.YL] <= box[:, M.YH]).all() and (box[:, M.YH] <= H).all()
        assert (box[:, M.XL] >= 0).all() and (box[:, M.XL] <= box[:, M.XH]).all() and (box[:, M.XH] <= W).all()
    if kw.get("prob", 1.0) < 1.0:
        assert 0 in kinds                                                    # lam == 1.0 exactly: untouched, weights (1, 0)
        assert (got[got[:, M.KIND] == 0][:, [M.WSELF, M.WOTHER]] == [M._bits(1.0), 0]).all()


def test_rng_argument_overrides_global_stream():
    a = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", rng=np.random.RandomState(5))
    b = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")
    np.random.seed(5)
    state = np.random.get_state()[1].copy()
    ta = a.draw(6, 32, 32)
    assert np.array_equal(np.random.get_state()[1], state)                  # the global stream was not touched
    tb = b.draw(6, 32, 32)
    assert np.array_equal(ta, tb)


def test_disabled_mixup_draws_nothing():
    m = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair")
    m.mixup_enabled = False
    t = m.draw(4, 16, 16)
    assert (t[:, M.KIND] == 0).all() and (t[:, M.WSELF] == M._bits(1.0)).all() and (t[:, M.WOTHER] == 0).all()


def test_odd_batch_and_bad_inputs_raise():
    m = M.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0)
    with pytest.raises(ValueError, match="even"):
        m(torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 3, 8, 8), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="mode"):
        M.Mixup(mode="row")


def _args(**kw):
    base = dict(enable_smoothing=False, enable_mixup=False, smoothing=0.0, mixup=0.0, cutmix=1.0, cutmix_minmax=None, mixup_prob=1.0,
                mixup_switch_prob=0.5, mixup_mode="batch", nb_classes=200, use_ppc_loss=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_create_mixup_and_criterion_follow_main():
    from protopformer_amd.protopformer import CrossEntropyLoss
    # no flag: nn.CrossEntropyLoss, no mixing
    a = _args()
    assert M.create_mixup(a) is None and type(M.create_criterion(a)) is CrossEntropyLoss
    # --enable_smoothing: LabelSmoothingCrossEntropy(0.1)
    a = _args(enable_smoothing=True)
    c = M.create_criterion(a)
    assert M.create_mixup(a) is None and isinstance(c, M.LabelSmoothingCrossEntropy) and c.smoothing == 0.1
    # --enable_mixup with the flag defaults (mixup 0, cutmix 1): CutMix-only Mixup and nn.CrossEntropyLoss given probability targets
    a = _args(enable_mixup=True)
    m, c = M.create_mixup(a), M.create_criterion(a)
    assert type(c) is CrossEntropyLoss
    assert isinstance(m, M.Mixup) and m.mixup_enabled and m.mixup_alpha == 0.0 and m.cutmix_alpha == 1.0 and m.label_smoothing == 0.0
    assert m.num_classes == 200 and m.mode == "batch" and m.mix_prob == 1.0 and m.switch_prob == 0.5 and m.cutmix_minmax is None
    # --enable_mixup --mixup 0.8: SoftTargetCrossEntropy
    a = _args(enable_mixup=True, mixup=0.8, mixup_mode="elem", mixup_prob=0.7, mixup_switch_prob=0.3)
    m, c = M.create_mixup(a), M.create_criterion(a)
    assert isinstance(c, M.SoftTargetCrossEntropy)
    assert (m.mixup_alpha, m.cutmix_alpha, m.mode, m.mix_prob, m.switch_prob) == (0.8, 1.0, "elem", 0.7, 0.3)
    # both flags: the smoothing moves into the mixed targets
    a = _args(enable_mixup=True, enable_smoothing=True, mixup=0.8)
    m, c = M.create_mixup(a), M.create_criterion(a)
    assert isinstance(c, M.SoftTargetCrossEntropy) and m.label_smoothing == 0.1
    a = _args(enable_mixup=True, enable_smoothing=True)
    m, c = M.create_mixup(a), M.create_criterion(a)
    assert isinstance(c, M.LabelSmoothingCrossEntropy) and c.smoothing == 0.1 and m.label_smoothing == 0.1
    # cutmix_minmax alone activates CutMix (alpha forced to 1)
    a = _args(enable_mixup=True, cutmix=0.0, cutmix_minmax=[0.2, 0.8])
    m = M.create_mixup(a)
    assert m.cutmix_alpha == 1.0 and list(m.cutmix_minmax) == [0.2, 0.8]
    # nothing active under --enable_mixup: no mixing
    assert M.create_mixup(_args(enable_mixup=True, cutmix=0.0)) is None
    # the reference's assertions
    with pytest.raises(ValueError, match="enable_mixup"):
        M.create_mixup(_args(mixup=0.8))
    with pytest.raises(ValueError, match="enable_smoothing"):
        M.create_criterion(_args(smoothing=0.2))
    with pytest.raises(ValueError, match="enable_smoothing"):
        M.create_mixup(_args(smoothing=0.2))


def test_ppc_with_mixup_is_refused():
    with pytest.raises(ValueError, match="PPC"):
        M.create_mixup(_args(enable_mixup=True, use_ppc_loss=True))
    with pytest.raises(ValueError, match="PPC"):
        M.create_mixup(_args(enable_mixup=True, mixup=0.8, use_ppc_loss=True))
    assert M.create_mixup(_args(enable_mixup=True, cutmix=0.0, use_ppc_loss=True)) is None      # no mixing, nothing to refuse


def test_soft_targets_refused_before_any_launch():
    from protopformer_amd.protopformer import CrossEntropyLoss, construct_PPNet
    logits = torch.zeros(4, 10)
    with pytest.raises(ValueError, match="floating-point target"):
        CrossEntropyLoss()(logits, torch.zeros(4))                           # a float [B] target: torch refuses it too
    with pytest.raises(ValueError, match="floating-point target"):
        M.SoftTargetCrossEntropy()(logits, torch.zeros(4, 9))
    with pytest.raises(ValueError, match="integer class indices"):
        M.LabelSmoothingCrossEntropy(0.1)(logits, torch.zeros(4, 10))
    with pytest.raises(ValueError):
        M.LabelSmoothingCrossEntropy(1.0)
    m = construct_PPNet("deit_tiny_patch16_224", pretrained=False, prototype_shape=(20, 32, 1, 1), num_classes=10, reserve_layers=[11],
                        reserve_token_nums=[81], use_global=True, use_ppc_loss=True, global_proto_per_class=2, add_on_layers_type="regular")
    with pytest.raises(ValueError, match="soft targets"):
        m.get_PPC_loss(torch.zeros(4, 20, 9, 9), torch.zeros(4, 196), 196, torch.full((4, 10), 0.1))


@pytest.fixture(scope="module")
def lib():
    from protopformer_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    lib.ppf_last_error.restype = ctypes.c_char_p
    return lib


def test_entry_points_validate_before_any_device_call(lib):
    B, H, W = 2, 8, 8
    t = np.zeros((B, M.MIX_WORDS), np.int32)
    fake = ctypes.c_void_p(0x1000)                                           # never dereferenced: validation fails first
    t[1, M.KIND] = 3
    rc = lib.ppf_mixup_apply(fake, t.ctypes.data_as(ctypes.c_void_p), fake, B, 3, H, W, None)
    assert rc == -3 and b"kind 3" in lib.ppf_last_error()
    t[1] = [M.BOX, 2, 9, 0, 4, 0, 0, 0]                                      # yh > H
    rc = lib.ppf_mixup_apply(fake, t.ctypes.data_as(ctypes.c_void_p), fake, B, 3, H, W, None)
    assert rc == -3 and b"not inside" in lib.ppf_last_error()
    t[1] = [M.BOX, 5, 4, 0, 4, 0, 0, 0]                                      # yl > yh
    rc = lib.ppf_mixup_apply(fake, t.ctypes.data_as(ctypes.c_void_p), fake, B, 3, H, W, None)
    assert rc == -3 and b"not inside" in lib.ppf_last_error()
    rc = lib.ppf_mixup_apply(fake, t.ctypes.data_as(ctypes.c_void_p), fake, 0, 3, H, W, None)
    assert rc == -1
    rc = lib.ppf_mixup_target(fake, fake, 8, ctypes.c_float(0.0), ctypes.c_float(1.0), fake, B, 0, None)
    assert rc == -1
    rc = lib.ppf_soft_cross_entropy(fake, None, None, ctypes.c_float(0.0), fake, fake, fake, B, 10, None)
    assert rc == -3 and b"exactly one" in lib.ppf_last_error()
    rc = lib.ppf_soft_cross_entropy(fake, fake, fake, ctypes.c_float(0.0), fake, fake, fake, B, 10, None)
    assert rc == -3
    rc = lib.ppf_soft_cross_entropy(fake, None, fake, ctypes.c_float(1.5), fake, fake, fake, B, 10, None)
    assert rc == -3 and b"smoothing" in lib.ppf_last_error()
    rc = lib.ppf_soft_cross_entropy(fake, None, fake, ctypes.c_float(0.1), fake, fake, fake, 0, 10, None)
    assert rc == -1
