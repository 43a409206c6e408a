"""The numpy referees of the device-resident data path against Pillow itself, bit for bit: the resize / crop / mirror referee against
Image.resize, the RandAugment referee against RandAugment._apply, op by op; the draw / apply split keeps the sequence of calls on the
random generator; without the switch build_loaders constructs what it always did.  The HIP kernels are held to these referees in
tests/test_gpu_device_data.py."""
import os
import random
import types

import numpy as np
import pytest
from PIL import Image

from protopformer_amd import data as D

# (frame h, w, box (x0, y0, x1, y1), full output (oh, ow), window (y0, x0), window size (H, W)); shared with the GPU tests
RESIZE_CASES = {
    "minify": (37, 53, (0, 0, 53, 37), (12, 16), (0, 0), (12, 16)),                   # more than nine taps per axis
    "magnify": (7, 9, (0, 0, 9, 7), (12, 16), (0, 0), (12, 16)),                      # the filter scale clamps to 1
    "box_left": (37, 53, (0, 5, 20, 30), (12, 16), (0, 0), (12, 16)),                 # the taps clamp at the frame, not at the box
    "box_top": (37, 53, (10, 0, 40, 20), (12, 16), (0, 0), (12, 16)),
    "box_right": (37, 53, (30, 10, 53, 30), (12, 16), (0, 0), (12, 16)),
    "box_bottom": (37, 53, (5, 20, 40, 37), (12, 16), (0, 0), (12, 16)),
    "box_one_wide": (37, 53, (20, 3, 21, 30), (12, 16), (0, 0), (12, 16)),
    "eval_wide": (37, 50) + ((0, 0, 50, 37),) + (lambda g: (g[:2], g[2:], (16, 16)))(D.eval_geometry(37, 50, 18, 16)),
    "eval_tall": (50, 37) + ((0, 0, 37, 50),) + (lambda g: (g[:2], g[2:], (16, 16)))(D.eval_geometry(50, 37, 18, 16)),
}


def frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pil_resize_crop(img, box, out, win, size, mirror, filt=Image.BICUBIC):
    ref = np.asarray(Image.fromarray(img).resize((out[1], out[0]), filt, box=box))[win[0]:win[0] + size[0], win[1]:win[1] + size[1]]
    return ref[:, ::-1] if mirror else ref


@pytest.mark.parametrize("mirror", [0, 1])
@pytest.mark.parametrize("case", sorted(RESIZE_CASES))
def test_resize_referee_equals_pillow(case, mirror):
    h, w, box, out, win, size = RESIZE_CASES[case]
    img = frame(h, w, 11)
    lead = np.zeros(5, dtype=np.uint8)                                            # the frame does not start the buffer
    plan = D.resize_plan([5], [(h, w)], [box], [out], [win], [mirror])
    got = D.resize_crop(np.concatenate([lead, img.reshape(-1)]), plan, *size)[0]
    assert np.array_equal(got, pil_resize_crop(img, box, out, win, size, mirror))


def test_eval_geometry_is_resize_then_center_crop():
    for h, w in ((37, 50), (50, 37), (18, 40), (41, 41)):
        oh, ow, y0, x0 = D.eval_geometry(h, w, 18, 16)
        img = Image.fromarray(frame(h, w, 3))
        want = np.asarray(D.CenterCrop(16)(D.Resize(18)(img)))
        got = D.resize_crop(np.asarray(img).reshape(-1), D.resize_plan([0], [(h, w)], [(0, 0, w, h)], [(oh, ow)], [(y0, x0)], [0]), 16, 16)[0]
        assert np.array_equal(got, want), (h, w)


def test_bilinear_square_view_equals_pillow():
    img = frame(37, 53, 4)
    want = np.asarray(D.Resize((16, 16), "bilinear")(Image.fromarray(img)))
    got = D.resize_crop(img.reshape(-1), D.resize_plan([0], [(37, 53)], [(0, 0, 53, 37)], [(16, 16)], [(0, 0)], [0]), 16, 16, filter=Image.BILINEAR)[0]
    assert np.array_equal(got, want)


class ScriptedRng:
    """Stands in for RandAugment.rng: the resample choice and the sign are the test's."""

    def __init__(self, resample, negate):
        self.resample, self.negate = resample, negate

    def choice(self, seq):
        assert self.resample in seq
        return self.resample

    def random(self):
        return 0.9 if self.negate else 0.1


def aug_images():
    return {"noise": frame(24, 20, 1), "constant": np.full((24, 20, 3), 77, dtype=np.uint8)}      # constant: lo == hi, a one-bin histogram


@pytest.mark.parametrize("name", D.RandAugment.OPS)
def test_randaugment_referee_equals_pillow(name):
    for iname, img in aug_images().items():
        for mag in (0, 4.3, 9, 10):
            for negate in (False, True):
                for resample in (Image.BILINEAR, Image.BICUBIC):
                    ra = D.RandAugment(rng=ScriptedRng(resample, negate))
                    want = np.asarray(ra._apply(name, Image.fromarray(img), mag))
                    plan = D.aug_plan([[ra._draw_op(name, mag)]], *img.shape[:2])
                    got = D.randaugment_apply(img[None], plan, ra.fill)[0]
                    assert np.array_equal(got, want), (iname, mag, negate, resample, int((got != want).sum()))


@pytest.mark.parametrize("resample", [Image.BILINEAR, Image.BICUBIC])
@pytest.mark.parametrize("name,param", [("TranslateXRel", 1.5), ("TranslateXRel", -1.5), ("TranslateYRel", 1.5), ("TranslateYRel", -1.5)])
def test_translation_out_of_frame_is_the_fill_colour(name, param, resample):
    ra, img = D.RandAugment(), frame(24, 20, 2)
    want = np.asarray(ra._apply_drawn(name, param, resample, Image.fromarray(img)))
    got = D.randaugment_apply(img[None], D.aug_plan([[(name, param, resample)]], 24, 20), ra.fill)[0]
    assert np.array_equal(got, want) and (got == np.asarray(ra.fill, dtype=np.uint8)).all()


def test_two_slots_compose_and_skip_is_identity():
    ra, img = D.RandAugment(rng=random.Random(5)), frame(24, 20, 6)
    for _ in range(40):
        draws = ra.draw()
        want = np.asarray(ra.apply(draws, Image.fromarray(img)))
        assert np.array_equal(D.randaugment_apply(img[None], D.aug_plan([draws], 24, 20), ra.fill)[0], want), draws
    skipped = [(None, 0.0, Image.BILINEAR)] * 2
    assert np.array_equal(D.randaugment_apply(img[None], D.aug_plan([skipped], 24, 20), ra.fill)[0], img)


def test_draw_order_is_the_old_call_order():
    """RandAugment(rng=Random(7)) gives the images it gave before the draw / apply split: the old __call__ is replayed here, call by call."""
    imgs = [Image.fromarray(frame(40, 36, 100 + k)) for k in range(60)]
    ra = D.RandAugment(rng=random.Random(7))
    new = [np.asarray(ra(im)) for im in imgs]
    rng = random.Random(7)
    old_ra, applied = D.RandAugment(rng=rng), 0
    for im, got in zip(imgs, new):
        for name in [rng.choice(D.RandAugment.OPS) for _ in range(2)]:
            if rng.random() > 0.5:
                continue
            mag = rng.gauss(9.0, 0.5)
            im = old_ra._apply(name, im, min(10.0, max(0.0, mag)))
            applied += 1
        assert np.array_equal(np.asarray(im), got)
    assert 30 <= applied <= 90
    # draw() then apply() is __call__, and leaves the generator where __call__ leaves it
    a, b = D.RandAugment(rng=random.Random(7)), D.RandAugment(rng=random.Random(7))
    for im in imgs[:10]:
        assert np.array_equal(np.asarray(a.apply(a.draw(), im)), np.asarray(b(im)))
    assert a.rng.random() == b.rng.random()


def test_switch_is_off_by_default_and_build_loaders_is_unchanged(tmp_path, monkeypatch):
    import torch
    from mini_trees import build_cub
    build_cub(str(tmp_path))
    args = types.SimpleNamespace(input_size=64, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="CUB2011U", data_path=str(tmp_path),
                                 batch_size=4, num_workers=0, reprob=0.25)
    monkeypatch.delenv("PPF_DEVICE_DATA", raising=False)
    assert not D.device_data_enabled(args)
    train, val, nb = D.build_loaders(args, torch.device("cpu"))
    assert type(train) is D.DeviceLoader and type(val) is D.DeviceLoader and nb == 200
    assert train.loader.drop_last and train.loader.batch_size == 4 and val.loader.batch_size == 6
    assert train.finisher.re_prob == 0.25 and val.finisher.re_prob == 0.0
    assert [type(t) for t in train.loader.dataset.transform.transforms] == [D.RandomResizedCrop, D.RandomHorizontalFlip, D.RandAugment, D.ToUint8HWC]
    assert [type(t) for t in val.loader.dataset.transform.transforms] == [D.Resize, D.CenterCrop, D.ToUint8HWC]
    for env, flag, want in (("1", None, True), ("0", None, False), ("", None, False), ("1", False, False), ("0", True, True), (None, True, True)):
        if env is None:
            monkeypatch.delenv("PPF_DEVICE_DATA", raising=False)
        else:
            monkeypatch.setenv("PPF_DEVICE_DATA", env)
        args.device_data = flag
        assert D.device_data_enabled(args) is want, (env, flag)


def test_resize_plan_is_validated_on_the_host():
    """ppf_resize_crop_workspace_bytes refuses a plan that would read outside the frames, before anything is launched (no GPU needed)."""
    from protopformer_amd import _lib
    from protopformer_amd.build import build
    build(verbose=False)
    good = D.resize_plan([0], [(37, 53)], [(0, 0, 53, 37)], [(12, 16)], [(0, 0)], [0])
    assert D.resize_workspace_bytes(good, 12, 16, Image.BICUBIC, 37 * 53 * 3) > 0
    for word, value, text in ((0, 1.0, "leaves the"), (5, 54.0, "box"), (9, 1.0, "window"), (11, 2.0, "mirror"), (1, float("nan"), "finite")):
        bad = good.copy()
        bad[0, word] = value
        with pytest.raises(RuntimeError, match=text):
            D.resize_workspace_bytes(bad, 12, 16, Image.BICUBIC, 37 * 53 * 3)
    with pytest.raises(RuntimeError, match="filter"):
        D.resize_workspace_bytes(good, 12, 16, Image.NEAREST, 37 * 53 * 3)
    assert _lib.DEFINES["PPF_RC_WORDS"] == D.RC_WORDS and _lib.DEFINES["PPF_AUG_WORDS"] == D.AUG_WORDS and _lib.DEFINES["PPF_AUG_SKIP"] == D.AUG_SKIP
    assert [_lib.DEFINES["PPF_AUG_" + n] for n in ("AUTOCONTRAST", "EQUALIZE", "INVERT", "ROTATE", "POSTERIZE", "SOLARIZE", "SOLARIZE_ADD", "COLOR", "CONTRAST",
                                                   "BRIGHTNESS", "SHARPNESS", "SHEAR_X", "SHEAR_Y", "TRANSLATE_X", "TRANSLATE_Y")] == list(range(15))
