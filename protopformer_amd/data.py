"""Real-data input pipeline of the train / eval loop (reference: tools/datasets.py:167-335 build_dataset /
build_transform, :402-474 Cub2011, :477-589 StanfordCars, :662-907 Dogs, tools/preprocess.py:1-33).

MI355X-first split of the work:
  * CPU worker processes do what only a CPU library can do here -- JPEG decode (PIL) and the PIL-space geometric / photometric
    augmentations (RandomResizedCrop, flip, RandAugment) -- and hand over **uint8 HWC frames** (150 KB per 224x224 image: a
    quarter of the fp32 tensor the reference's ToTensor produces, so the host-to-device copy of a 256-image batch is 38 MB);
  * the GPU does the rest in ONE kernel pass (`ppf_image_finish_u8`, csrc/elementwise.hip): uint8 -> fp32, HWC -> NCHW,
    mean/std normalisation and timm's RandomErasing ('pixel' mode: N(0,1) noise from Philox) written straight into the batch
    buffer the train step reads.
Dataset index parsing follows the reference's classes line by line in behaviour (same files, same label shifts, same splits).

Third-party boundary: the train transform the reference builds is timm 0.5.4's `create_transform(..., auto_augment=
'rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25, re_mode='pixel')` (tools/datasets.py:280-309); timm is not
vendored and not installed here, so RandAugment / RandomResizedCrop / RandomErasing below are written from timm's public API
("parity unpinned" at that boundary, as for PatchEmbed / Mlp in the oracle) and tested for their invariants.
"""
import math
import os
import random
import xml.etree.ElementTree

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageOps

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def default_loader(path):
    with open(path, "rb") as f:
        return Image.open(f).convert("RGB")


# ------------------------------------------------------------------------------------------------ datasets
class Cub2011:
    """CUB-200-2011 (tools/datasets.py:402-474): root/CUB_200_2011/{images.txt, image_class_labels.txt, train_test_split.txt,
    images/}; targets shifted to 0..199; `train` selects is_training_img == 1 / 0.  return_id=True also yields the image id
    (eval_interpretability.py:140 iterates (data, targets, img_ids))."""
    base_folder = "CUB_200_2011/images"

    def __init__(self, root, train=True, transform=None, loader=default_loader, download=False, return_id=False):
        self.root = os.path.expanduser(root)
        self.transform, self.loader, self.train, self.return_id = transform, loader, train, return_id
        if download:
            raise RuntimeError("no network access: place CUB_200_2011 under the data path")
        meta = os.path.join(self.root, "CUB_200_2011")
        try:
            paths = dict(self._pairs(os.path.join(meta, "images.txt"), str))
            labels = dict(self._pairs(os.path.join(meta, "image_class_labels.txt"), int))
            split = dict(self._pairs(os.path.join(meta, "train_test_split.txt"), int))
        except OSError as e:
            raise RuntimeError("Dataset not found or corrupted. (no download possible here)") from e
        want = 1 if train else 0
        # pandas inner merges on img_id (tools/datasets.py:427-434): rows stay in the order of images.txt, ids missing from either of
        # the other two files drop out
        self.data = [(i, paths[i], labels[i]) for i in paths if split.get(i) == want and i in labels]
        for _, fp, _ in self.data:
            if not os.path.isfile(os.path.join(self.root, self.base_folder, fp)):
                raise RuntimeError("Dataset not found or corrupted: missing " + fp)

    @staticmethod
    def _pairs(path, conv):
        with open(path) as f:
            for line in f:
                a, b = line.rstrip("\n").split(" ", 1)
                yield int(a), conv(b)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        img_id, fp, target = self.data[idx]
        img = self.loader(os.path.join(self.root, self.base_folder, fp))
        if self.transform is not None:
            img = self.transform(img)
        return (img, target - 1, img_id) if self.return_id else (img, target - 1)


class StanfordCars:
    """Stanford Cars (tools/datasets.py:477-589): root/stanford_cars/{devkit/cars_train_annos.mat, devkit/cars_meta.mat,
    cars_test_annos_withlabels.mat, cars_train/, cars_test/}; class ids shifted to 0..195."""

    def __init__(self, root, split="train", transform=None, target_transform=None, download=False):
        import scipy.io as sio
        if split not in ("train", "test"):
            raise ValueError("split must be 'train' or 'test'")
        base = os.path.join(root, "stanford_cars")
        devkit = os.path.join(base, "devkit")
        annos = os.path.join(devkit, "cars_train_annos.mat") if split == "train" else os.path.join(base, "cars_test_annos_withlabels.mat")
        images = os.path.join(base, "cars_train" if split == "train" else "cars_test")
        if not (os.path.exists(annos) and os.path.isdir(images)):
            raise RuntimeError("Dataset not found. (no download possible here)")
        self.transform, self.target_transform = transform, target_transform
        ann = np.atleast_1d(sio.loadmat(annos, squeeze_me=True)["annotations"])
        self._samples = [(os.path.join(images, str(a["fname"])), int(a["class"]) - 1) for a in ann]
        self.classes = [str(c) for c in np.atleast_1d(sio.loadmat(os.path.join(devkit, "cars_meta.mat"), squeeze_me=True)["class_names"]).tolist()]
        self.class_to_idx = {c: i for i, c in enumerate(self.classes)}

    def __len__(self):
        return len(self._samples)

    def __getitem__(self, idx):
        path, target = self._samples[idx]
        img = Image.open(path).convert("RGB")
        if self.transform is not None:
            img = self.transform(img)
        if self.target_transform is not None:
            target = self.target_transform(target)
        return img, target


class Dogs:
    """Stanford Dogs (tools/datasets.py:662-907): root/{Images/, Annotation/, train_list.mat, test_list.mat}; `cropped` cuts every
    annotated bounding box out as its own sample."""

    def __init__(self, root, train=True, cropped=False, transform=None, target_transform=None, download=False):
        import scipy.io as sio
        self.root, self.train, self.cropped, self.transform, self.target_transform = root, train, cropped, transform, target_transform
        lst = sio.loadmat(os.path.join(root, "train_list.mat" if train else "test_list.mat"))
        split = [(str(item[0][0]), int(lab[0]) - 1) for item, lab in zip(lst["annotation_list"], lst["labels"])]
        self.images_folder, self.annotations_folder = os.path.join(root, "Images"), os.path.join(root, "Annotation")
        self._breeds = sorted(d for d in os.listdir(self.images_folder) if os.path.isdir(os.path.join(self.images_folder, d)))
        if cropped:
            self._flat_breed_annotations = [(a, box, idx) for a, idx in split for box in self.get_boxes(os.path.join(self.annotations_folder, a))]
            self._flat_breed_images = [(a + ".jpg", idx) for a, _, idx in self._flat_breed_annotations]
        else:
            self._flat_breed_images = [(a + ".jpg", idx) for a, idx in split]

    @staticmethod
    def get_boxes(path):
        e = xml.etree.ElementTree.parse(path).getroot()
        return [[int(o.find("bndbox").find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")] for o in e.iter("object")]

    def __len__(self):
        return len(self._flat_breed_images)

    def __getitem__(self, index):
        name, target = self._flat_breed_images[index]
        img = Image.open(os.path.join(self.images_folder, name)).convert("RGB")
        if self.cropped:
            img = img.crop(self._flat_breed_annotations[index][1])
        if self.transform:
            img = self.transform(img)
        if self.target_transform:
            target = self.target_transform(target)
        return img, target

    def stats(self):
        counts = {}
        for _, t in self._flat_breed_images:
            counts[t] = counts.get(t, 0) + 1
        return counts


# ------------------------------------------------------------------------------------------------ PIL-space transforms (CPU workers)
_INTERP = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "nearest": Image.NEAREST}


class Resize:
    """torchvision Resize: int -> shorter side to `size` keeping the aspect ratio; (h, w) -> exact."""

    def __init__(self, size, interpolation="bicubic"):
        self.size, self.interp = size, _INTERP[interpolation] if isinstance(interpolation, str) else interpolation

    def __call__(self, img):
        if isinstance(self.size, int):
            w, h = img.size
            if (w <= h and w == self.size) or (h <= w and h == self.size):
                return img
            if w < h:
                return img.resize((self.size, int(self.size * h / w)), self.interp)
            return img.resize((int(self.size * w / h), self.size), self.interp)
        return img.resize((self.size[1], self.size[0]), self.interp)


class CenterCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img):
        w, h = img.size
        left, top = int(round((w - self.size) / 2.0)), int(round((h - self.size) / 2.0))
        return img.crop((left, top, left + self.size, top + self.size))


class RandomResizedCrop:
    """timm RandomResizedCropAndInterpolation / torchvision RandomResizedCrop: scale (0.08, 1), ratio (3/4, 4/3), 10 attempts."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), interpolation="bicubic", rng=random):
        self.size, self.scale, self.ratio, self.interp, self.rng = size, scale, ratio, _INTERP[interpolation], rng

    def get_params(self, w, h):
        area = w * h
        for _ in range(10):
            target = self.rng.uniform(*self.scale) * area
            ar = math.exp(self.rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1])))
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                return self.rng.randint(0, h - ch), self.rng.randint(0, w - cw), ch, cw
        in_ratio = w / h
        if in_ratio < self.ratio[0]:
            cw, ch = w, int(round(w / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            ch, cw = h, int(round(h * self.ratio[1]))
        else:
            cw, ch = w, h
        return (h - ch) // 2, (w - cw) // 2, ch, cw

    def __call__(self, img):
        top, left, ch, cw = self.get_params(*img.size)
        return img.resize((self.size, self.size), self.interp, box=(left, top, left + cw, top + ch))


class RandomHorizontalFlip:
    def __init__(self, p=0.5, rng=random):
        self.p, self.rng = p, rng

    def __call__(self, img):
        return img.transpose(Image.FLIP_LEFT_RIGHT) if self.rng.random() < self.p else img


class RandAugment:
    """timm rand_augment_transform('rand-m9-mstd0.5-inc1'): 2 ops per image drawn uniformly from the 'increasing' set, each applied
    with probability 0.5 at magnitude ~ N(9, 0.5) clipped to [0, 10]."""
    OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
           "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")

    def __init__(self, config="rand-m9-mstd0.5-inc1", img_size=224, mean=IMAGENET_DEFAULT_MEAN, rng=random):
        parts = config.split("-")
        assert parts[0] == "rand"
        self.m, self.mstd, self.n, self.inc = 10.0, 0.0, 2, False
        for c in parts[1:]:
            if c.startswith("mstd"):
                self.mstd = float(c[4:])
            elif c.startswith("inc"):
                self.inc = bool(int(c[3:]))
            elif c.startswith("m"):
                self.m = float(c[1:])
            elif c.startswith("n"):
                self.n = int(c[1:])
        if not self.inc:
            raise NotImplementedError("only the 'increasing' op set of the reference's default policy is implemented")
        self.fill = tuple(int(round(255 * x)) for x in mean)
        self.translate_pct = 0.45
        self.rng = rng

    def _neg(self, v):
        return -v if self.rng.random() > 0.5 else v

    def _draw_op(self, name, mag):
        """(name, signed parameter, resample filter) of one op at magnitude `mag`: the resample choice is drawn first, then the sign."""
        lv = mag / 10.0
        resample = self.rng.choice((Image.BILINEAR, Image.BICUBIC))
        if name in ("AutoContrast", "Equalize", "Invert"):
            return name, 0.0, resample
        if name == "Rotate":
            return name, self._neg(lv * 30.0), resample
        if name == "PosterizeIncreasing":
            return name, max(1, 4 - int(lv * 4)), resample
        if name == "SolarizeIncreasing":
            return name, 256 - int(lv * 256), resample
        if name == "SolarizeAdd":
            return name, int(lv * 110), resample
        if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
            return name, max(0.1, 1.0 + self._neg(lv * 0.9)), resample
        if name in ("ShearX", "ShearY"):
            return name, self._neg(lv * 0.3), resample
        if name in ("TranslateXRel", "TranslateYRel"):
            return name, self._neg(lv * self.translate_pct), resample
        raise KeyError(name)

    def _apply_drawn(self, name, param, resample, img):
        if name == "AutoContrast":
            return ImageOps.autocontrast(img)
        if name == "Equalize":
            return ImageOps.equalize(img)
        if name == "Invert":
            return ImageOps.invert(img)
        if name == "Rotate":
            return img.rotate(param, resample=resample, fillcolor=self.fill)
        if name == "PosterizeIncreasing":
            return ImageOps.posterize(img, param)
        if name == "SolarizeIncreasing":
            return ImageOps.solarize(img, param)
        if name == "SolarizeAdd":
            lut = [min(255, i + param) if i < 128 else i for i in range(256)]
            return img.point(lut * 3)
        if name in ("ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing"):
            enh = {"Color": ImageEnhance.Color, "Contrast": ImageEnhance.Contrast, "Brightness": ImageEnhance.Brightness,
                   "Sharpness": ImageEnhance.Sharpness}[name[:-len("Increasing")]]
            return enh(img).enhance(param)
        if name == "ShearX":
            return img.transform(img.size, Image.AFFINE, (1, param, 0, 0, 1, 0), resample=resample, fillcolor=self.fill)
        if name == "ShearY":
            return img.transform(img.size, Image.AFFINE, (1, 0, 0, param, 1, 0), resample=resample, fillcolor=self.fill)
        if name == "TranslateXRel":
            return img.transform(img.size, Image.AFFINE, (1, 0, param * img.size[0], 0, 1, 0), resample=resample, fillcolor=self.fill)
        if name == "TranslateYRel":
            return img.transform(img.size, Image.AFFINE, (1, 0, 0, 0, 1, param * img.size[1]), resample=resample, fillcolor=self.fill)
        raise KeyError(name)

    def _apply(self, name, img, mag):
        return self._apply_drawn(*self._draw_op(name, mag), img)

    def draw(self):
        """The plan of one image: per slot (op name or None when the slot is skipped, signed parameter, resample filter).  The calls on
        `rng` are those __call__ always made, in its order: the names, then per op the skip draw, the magnitude, the resample choice, the sign."""
        plan = []
        for name in [self.rng.choice(self.OPS) for _ in range(self.n)]:
            if self.rng.random() > 0.5:
                plan.append((None, 0.0, Image.BILINEAR))
                continue
            mag = self.m if self.mstd <= 0 else self.rng.gauss(self.m, self.mstd)
            plan.append(self._draw_op(name, min(10.0, max(0.0, mag))))
        return plan

    def apply(self, plan, img):
        for name, param, resample in plan:
            if name is not None:
                img = self._apply_drawn(name, param, resample, img)
        return img

    def __call__(self, img):
        return self.apply(self.draw(), img)


class ToUint8HWC:
    """The hand-over format to the GPU finisher: a contiguous uint8 [H, W, 3] array (no float conversion on the CPU)."""

    def __call__(self, img):
        a = np.asarray(img, dtype=np.uint8)
        if a.ndim == 2:
            a = np.repeat(a[:, :, None], 3, axis=2)
        return np.ascontiguousarray(a[:, :, :3])


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


def build_transform(is_train, args):
    """tools/datasets.py:280-336 for input_size > 32, up to (not including) ToTensor / Normalize / RandomErasing, which run on the
    GPU (GpuFinisher).  Train: RandomResizedCrop(bicubic) + flip + RandAugment(args.aa); eval: Resize(256/224 * size, bicubic) +
    CenterCrop."""
    size = args.input_size
    if size <= 32:
        raise NotImplementedError("the CIFAR-sized (input_size <= 32) branch is not on the ProtoPFormer path")
    if is_train:
        t = [RandomResizedCrop(size, interpolation=getattr(args, "train_interpolation", "bicubic")), RandomHorizontalFlip(0.5)]
        aa = getattr(args, "aa", "rand-m9-mstd0.5-inc1")
        if aa and aa != "none":
            t.append(RandAugment(aa, img_size=size))
        return Compose(t + [ToUint8HWC()])
    return Compose([Resize(int((256 / 224) * size), "bicubic"), CenterCrop(size), ToUint8HWC()])


def build_view_transform(args, square=False):
    """build_dataset_view / build_dataset_noaug geometry (tools/datasets.py:77-166): Resize(256/224 * size, bicubic) + CenterCrop,
    or a plain (size, size) resize when `square` (the reference's 'adam' model branch and eval_interpretability.py:128-132)."""
    size = args.input_size
    if square:
        return Compose([Resize((size, size), "bilinear"), ToUint8HWC()])
    return Compose([Resize(int((256 / 224) * size), "bicubic"), CenterCrop(size), ToUint8HWC()])


def build_dataset(is_train, args, transform=None):
    """tools/datasets.py:167-277 for the fine-grained sets ProtoPFormer is trained on.  Returns (dataset, nb_classes)."""
    transform = transform if transform is not None else build_transform(is_train, args)
    if args.data_set == "CUB2011U":
        return Cub2011(args.data_path, train=is_train, transform=transform), 200
    if args.data_set == "Car":
        return StanfordCars(args.data_path, split="train" if is_train else "test", transform=transform), 196
    if args.data_set == "Dogs":
        return Dogs(root=os.path.join(args.data_path, "stanford_dogs"), train=is_train, cropped=False, transform=transform), 120
    if args.data_set == "PartsWorld":                    # rendered, not read: the spec is the whole data set
        spec = partsworld_spec_from_args(args)
        return PartsWorld(spec, train=is_train, transform=transform), spec.classes
    raise NotImplementedError(f"data_set {args.data_set!r}: only CUB2011U / Car / Dogs (scripts/train_{{cub,car,dog}}.sh) and PartsWorld are on the path")


# ------------------------------------------------------------------------------------------------ GPU finisher + loader
def random_erasing_rects(B, H, W, prob=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, rng=random):
    """timm RandomErasing(probability, mode='pixel', max_count=1) rectangle draw per sample: int32 [B, 4] = (y, x, h, w), h = 0: none."""
    rects = np.zeros((B, 4), dtype=np.int32)
    log_r = (math.log(min_aspect), math.log(1 / min_aspect))
    for b in range(B):
        if rng.random() > prob:
            continue
        for _ in range(10):
            target = rng.uniform(min_area, max_area) * H * W
            ar = math.exp(rng.uniform(*log_r))
            h, w = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if w < W and h < H:
                rects[b] = (rng.randint(0, H - h), rng.randint(0, W - w), h, w)
                break
    return rects


class GpuFinisher:
    """uint8 [B,H,W,3] (device) -> fp32 [B,3,H,W] normalised (+ RandomErasing when training) in one HIP kernel pass."""

    def __init__(self, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, re_prob=0.0, seed=None, rng=random):
        self.mean = np.asarray(mean, dtype=np.float32)
        self.std = np.asarray(std, dtype=np.float32)
        self.re_prob, self.rng = float(re_prob), rng
        self.seed = torch.initial_seed() if seed is None else int(seed)
        self.step = 0

    def __call__(self, frames_u8, out=None, rects=None):
        """rects: int32 [B, 4] erase rectangles drawn by the caller (DeviceAugLoader draws them per sample); None: drawn here."""
        from . import _lib
        if not frames_u8.is_cuda or frames_u8.dtype != torch.uint8:
            raise RuntimeError("GpuFinisher needs a uint8 CUDA tensor [B, H, W, 3] (no CPU fallback path)")
        B, H, W, C = frames_u8.shape
        assert C == 3 and frames_u8.is_contiguous()
        if out is None:
            out = torch.empty((B, 3, H, W), dtype=torch.float32, device=frames_u8.device)
        state = None
        if self.re_prob > 0:
            rects = random_erasing_rects(B, H, W, self.re_prob, rng=self.rng) if rects is None else np.ascontiguousarray(rects, dtype=np.int32).reshape(B, 4)
            rects = torch.from_numpy(rects).to(frames_u8.device, non_blocking=True)
            state = torch.tensor([self.step], dtype=torch.int64, device=frames_u8.device)
            self.step += 1
        _lib.call("ppf_image_finish_u8", frames_u8, out, B, H, W, self.mean.ctypes.data, self.std.ctypes.data, rects, self.seed & 0xFFFFFFFFFFFFFFFF, state)
        return out


def _collate_u8(batch):
    frames = torch.from_numpy(np.stack([b[0] for b in batch]))
    rest = [torch.as_tensor([b[i] for b in batch]) for i in range(1, len(batch[0]))]
    return (frames, *rest)


class DeviceLoader:
    """DataLoader (CPU decode / augmentation workers, uint8 collate, pinned) + GpuFinisher: yields (fp32 NCHW cuda, labels cuda[, ids])
    -- what engine.train_one_epoch / evaluate iterate over (main.py:302-316)."""

    def __init__(self, dataset, batch_size, device, finisher, shuffle=False, sampler=None, num_workers=0, drop_last=False, pin_memory=True):
        self.loader = torch.utils.data.DataLoader(dataset, batch_size=batch_size, shuffle=shuffle if sampler is None else False, sampler=sampler,
                                                  num_workers=num_workers, drop_last=drop_last, pin_memory=pin_memory and torch.cuda.is_available(),
                                                  collate_fn=_collate_u8)
        self.device, self.finisher, self.sampler, self.dataset = device, finisher, sampler, dataset

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for frames, target, *rest in self.loader:
            x = self.finisher(frames.to(self.device, non_blocking=True))
            yield (x, target.to(self.device, non_blocking=True).long(), *rest)


def _collate_list(batch):
    return batch


def device_data_enabled(args):
    """The switch of the device-resident path: args.device_data when it is set, else the environment variable PPF_DEVICE_DATA (set to
    something other than 0).  Off by default."""
    v = getattr(args, "device_data", None)
    if v is None:
        return os.environ.get("PPF_DEVICE_DATA", "0") not in ("", "0")
    return bool(v)


class DeviceDataset:
    """The decoded originals of a Cub2011 / StanfordCars / Dogs on the device: one pass with ToUint8HWC as the only transform (CPU workers
    decode, nothing is decoded again), then one flat uint8 buffer of HWC frames, an int64 offset table, an int32 (h, w) table, the labels
    and, for a data set with return_id, the image ids.  Every rank holds the whole set; samplers keep working on the indices.
    A PartsWorld is rendered straight into the flat buffer by ppf_synth_scene + ppf_synth_render, in runs of at most 256 frames: no
    worker, no decode, no upload; `rendered` says which of the two happened."""

    def __init__(self, dataset, device, num_workers=0, max_bytes=64 << 30):
        import copy
        import time
        t0 = time.perf_counter()
        self.rendered = isinstance(dataset, PartsWorld)
        if self.rendered:
            self._render(dataset, device, max_bytes)
            self.decode_seconds = time.perf_counter() - t0
            return
        ds = copy.copy(dataset)
        ds.transform = ToUint8HWC()
        with_ids = bool(getattr(ds, "return_id", False))
        frames, labels, ids, total = [], [], [], 0
        loader = torch.utils.data.DataLoader(ds, batch_size=16, shuffle=False, num_workers=num_workers, collate_fn=_collate_list)
        for batch in loader:
            for item in batch:
                a = np.asarray(item[0])
                total += a.size
                if total > max_bytes:
                    est = int(total / (len(frames) + 1) * len(ds))
                    raise RuntimeError(f"DeviceDataset: the decoded frames need about {est} bytes ({total} after {len(frames) + 1} of {len(ds)} images), "
                                       f"max_bytes is {max_bytes}; there is no fallback: raise max_bytes or use the CPU loader")
                frames.append(a)
                labels.append(int(item[1]))
                if with_ids:
                    ids.append(int(item[2]))
        if not frames:
            raise RuntimeError("DeviceDataset: the data set is empty")
        self.sizes_host = np.array([f.shape[:2] for f in frames], dtype=np.int32)
        nbytes = self.sizes_host[:, 0].astype(np.int64) * self.sizes_host[:, 1] * 3
        self.offsets_host = np.concatenate(([0], np.cumsum(nbytes)[:-1])).astype(np.int64)
        self.device = torch.device(device)
        self.flat = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=self.device)
        for k in range(0, len(frames), 256):                  # uploaded in runs of 256 frames
            run = torch.from_numpy(np.concatenate([f.reshape(-1) for f in frames[k:k + 256]]))
            self.flat[int(self.offsets_host[k]):int(self.offsets_host[k]) + run.numel()].copy_(run)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.sizes = torch.from_numpy(self.sizes_host).to(self.device)
        self.labels_host = np.array(labels, dtype=np.int64)
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        self.ids_host = np.array(ids, dtype=np.int64) if with_ids else None
        self.ids = torch.from_numpy(self.ids_host).to(self.device) if with_ids else None
        self.dataset = dataset
        self.decode_seconds = time.perf_counter() - t0

    def _render(self, dataset, device, max_bytes):
        from . import ops
        spec, n = dataset.spec, len(dataset)
        frame = spec.height * spec.width * 3
        if n * frame > max_bytes:
            raise RuntimeError(f"DeviceDataset: the {n} rendered frames need {n * frame} bytes, max_bytes is {max_bytes}; there is no fallback: raise "
                               "max_bytes or use the CPU loader")
        self.device = torch.device(device)
        self.sizes_host = np.tile(np.array([[spec.height, spec.width]], dtype=np.int32), (n, 1))
        self.offsets_host = np.arange(n, dtype=np.int64) * frame
        self.flat = torch.empty(n * frame, dtype=torch.uint8, device=self.device)
        self.ids_host = dataset.ids.copy()
        ids = torch.from_numpy(self.ids_host).to(self.device)
        for k in range(0, n, 256):                             # rendered in runs of 256 frames; the frame size is a multiple of 16 bytes
            run = ids[k:k + 256]
            ops.synth_render(spec, ops.synth_scene(spec, run), run, out=self.flat[k * frame:(k + len(run)) * frame])
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.sizes = torch.from_numpy(self.sizes_host).to(self.device)
        self.labels_host = dataset.labels.copy()
        self.labels = torch.from_numpy(self.labels_host).to(self.device)
        if not getattr(dataset, "return_id", False):
            self.ids_host, ids = None, None
        self.ids = ids
        self.dataset = dataset

    def __len__(self):
        return len(self.labels_host)


class DeviceAugLoader:
    """Batches from a DeviceDataset, produced on the device: yields what DeviceLoader yields.  train: RandomResizedCrop + flip (one
    ppf_resize_crop_u8 launch chain), RandAugment (ppf_aug_*), then the finisher with its RandomErasing; eval: Resize(256/224 * size) +
    CenterCrop (`square`: the plain bilinear (size, size) resize of build_view_transform).  The host draws, once per sample in sampler order,
    RandomResizedCrop.get_params, the flip, RandAugment.draw and random_erasing_rects from one random.Random seeded from (seed, epoch,
    rank): an epoch is a function of those three and the sampler's order, whatever the batch size.  The plan of the next batch is drawn
    while the current one runs; host_seconds holds the draw time per batch."""

    def __init__(self, device_dataset, batch_size, finisher, train, args, shuffle=False, sampler=None, drop_last=False, seed=0, square=False,
                 keep_plans=False):
        self.dd, self.batch_size, self.finisher, self.train, self.sampler = device_dataset, int(batch_size), finisher, bool(train), sampler
        self.shuffle, self.drop_last, self.seed, self.square, self.keep_plans = shuffle and sampler is None, drop_last, int(seed), square, keep_plans
        self.dataset, self.device, self.size = device_dataset.dataset, device_dataset.device, int(args.input_size)
        self.epoch, self.rank = 0, int(getattr(sampler, "rank", 0))
        self.host_seconds, self.plans, self._ws = [], [], None
        self.aa = None
        if self.train:
            if getattr(args, "train_interpolation", "bicubic") != "bicubic":
                raise NotImplementedError("DeviceAugLoader: the train crop is bicubic (train_interpolation of the reference's scripts)")
            aa = getattr(args, "aa", "rand-m9-mstd0.5-inc1")
            self.aa = aa if aa and aa != "none" else None
        if self.size <= 32:
            raise NotImplementedError("the CIFAR-sized (input_size <= 32) branch is not on the ProtoPFormer path")

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        if hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dd)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _order(self):
        if self.sampler is not None:
            return [int(i) for i in self.sampler]
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            return torch.randperm(len(self.dd), generator=g).tolist()
        return list(range(len(self.dd)))

    def _plan(self, idx, rrc, ra, rng):
        """The host's share of one batch: the resize table, the RandAugment draws and the erase rectangles of samples idx."""
        import time
        t0 = time.perf_counter()
        S, dd = self.size, self.dd
        boxes, outs, wins, mirror, draws = [], [], [], [], []
        rects = np.zeros((len(idx), 4), dtype=np.int32)
        for j, i in enumerate(idx):
            h, w = (int(v) for v in dd.sizes_host[i])
            if self.train:
                top, left, ch, cw = rrc.get_params(w, h)
                boxes.append((left, top, left + cw, top + ch))
                outs.append((S, S))
                wins.append((0, 0))
                mirror.append(1 if rng.random() < 0.5 else 0)
                draws.append(ra.draw() if ra is not None else [])
                if self.finisher.re_prob > 0:
                    rects[j] = random_erasing_rects(1, S, S, self.finisher.re_prob, rng=rng)[0]
            else:
                oh, ow, y0, x0 = (S, S, 0, 0) if self.square else eval_geometry(h, w, int((256 / 224) * S), S)
                boxes.append((0, 0, w, h))
                outs.append((oh, ow))
                wins.append((y0, x0))
                mirror.append(0)
        plan = {"idx": np.asarray(idx, dtype=np.int64), "resize": resize_plan(dd.offsets_host[idx], dd.sizes_host[idx], boxes, outs, wins, mirror),
                "draws": draws, "aug": aug_plan(draws, S, S) if self.aa and self.train else None, "rects": rects}
        self.host_seconds.append(time.perf_counter() - t0)
        return plan

    def __iter__(self):
        order = self._order()
        nb = len(order) // self.batch_size if self.drop_last else -(-len(order) // self.batch_size)
        rng = random.Random(f"{self.seed}:{self.epoch}:{self.rank}")
        rrc = RandomResizedCrop(self.size, rng=rng) if self.train else None
        ra = RandAugment(self.aa, img_size=self.size, rng=rng) if self.aa else None
        fill = ra.fill if ra is not None else (0, 0, 0)
        filt = Image.BILINEAR if self.square and not self.train else Image.BICUBIC
        chunk = lambda k: order[k * self.batch_size:(k + 1) * self.batch_size]
        plan = self._plan(chunk(0), rrc, ra, rng) if nb else None
        for k in range(nb):
            S = self.size
            need = int(resize_workspace_bytes(plan["resize"], S, S, filt, self.dd.flat.numel()))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            frames = resize_crop(self.dd.flat, plan["resize"], S, S, device=True, workspace=self._ws, filter=filt)
            if plan["aug"] is not None:
                frames = randaugment_apply(frames, plan["aug"], fill, device=True)
            x = self.finisher(frames, rects=plan["rects"] if self.train else None)
            idx = torch.from_numpy(plan["idx"]).to(self.device)
            rest = (torch.from_numpy(self.dd.ids_host[plan["idx"]]),) if self.dd.ids_host is not None else ()
            batch = (x, self.dd.labels[idx], *rest)
            if self.keep_plans:
                self.plans.append(plan)
            plan = self._plan(chunk(k + 1), rrc, ra, rng) if k + 1 < nb else None      # drawn while the device works on batch k
            yield batch


def build_loaders(args, device):
    """main.py:281-316: train loader (shuffled / DistributedSampler, drop_last) and validation loader (batch 1.5x, sequential)."""
    import torch.distributed as dist
    ds_train, nb = build_dataset(True, args)
    ds_val, _ = build_dataset(False, args)
    sampler = None
    if dist.is_initialized() and dist.get_world_size() > 1:
        sampler = torch.utils.data.DistributedSampler(ds_train, num_replicas=dist.get_world_size(), rank=dist.get_rank(), shuffle=True)
    if device_data_enabled(args):                       # opt-in: the originals resident on the device, every batch produced there
        workers, seed = getattr(args, "num_workers", 10), getattr(args, "seed", 0)
        train = DeviceAugLoader(DeviceDataset(ds_train, device, num_workers=workers), args.batch_size, GpuFinisher(re_prob=getattr(args, "reprob", 0.25)),
                                True, args, shuffle=sampler is None, sampler=sampler, drop_last=True, seed=seed)
        val = DeviceAugLoader(DeviceDataset(ds_val, device, num_workers=workers), int(1.5 * args.batch_size), GpuFinisher(re_prob=0.0), False, args, seed=seed)
        return train, val, nb
    train = DeviceLoader(ds_train, args.batch_size, device, GpuFinisher(re_prob=getattr(args, "reprob", 0.25)), shuffle=sampler is None, sampler=sampler,
                         num_workers=getattr(args, "num_workers", 10), drop_last=True)
    val = DeviceLoader(ds_val, int(1.5 * args.batch_size), device, GpuFinisher(re_prob=0.0), num_workers=getattr(args, "num_workers", 10))
    return train, val, nb


# ------------------------------------------------------------------------------------------------ device-resident data sets
# The originals are decoded once and stay on the device; every batch is cropped, flipped and augmented there by csrc/device_data.hip.
# The host only draws (the transform classes above, so the distribution is theirs by construction) and packs the draws into two small
# fp64 tables.  Every function below has a numpy referee (device=False) that is bit-equal to Pillow; the kernels are bit-equal to the
# referee.  The arithmetic contract is written out in include/ppf_hip.h.
RC_WORDS, AUG_WORDS, AUG_SLOTS = 12, 8, 2             # PPF_RC_WORDS / PPF_AUG_WORDS / PPF_AUG_SLOTS of the header
AUG_SKIP = -1
_AFFINE_OPS = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")


def resize_plan(offsets, sizes, boxes, out_sizes, windows, mirror):
    """fp64 [B][RC_WORDS] = (frame offset in bytes, h, w, box x0, y0, x1, y1, full output oh, ow, window y0, x0, mirror) per sample."""
    B = len(offsets)
    plan = np.zeros((B, RC_WORDS), dtype=np.float64)
    plan[:, 0] = np.asarray(offsets, dtype=np.float64)
    plan[:, 1:3] = np.asarray(sizes, dtype=np.float64).reshape(B, 2)
    plan[:, 3:7] = np.asarray(boxes, dtype=np.float64).reshape(B, 4)
    plan[:, 7:9] = np.asarray(out_sizes, dtype=np.float64).reshape(B, 2)
    plan[:, 9:11] = np.asarray(windows, dtype=np.float64).reshape(B, 2)
    plan[:, 11] = np.asarray(mirror, dtype=np.float64)
    return plan


def eval_geometry(h, w, size, crop):
    """(oh, ow, y0, x0): Resize(size)'s output size for an h x w frame and CenterCrop(crop)'s window in it."""
    if w < h:
        oh, ow = int(size * h / w), size
    elif (w <= h and w == size) or (h <= w and h == size):
        oh, ow = h, w
    else:
        oh, ow = size, int(size * w / h)
    return oh, ow, int(round((oh - crop) / 2.0)), int(round((ow - crop) / 2.0))


def _bicubic_weight(x):
    x = np.abs(x)
    a = -0.5
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def _bilinear_weight(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


_RESAMPLE = {Image.BICUBIC: (2.0, _bicubic_weight), Image.BILINEAR: (1.0, _bilinear_weight)}


def resample_taps(in_size, in0, in1, out_size, first, count, filter=Image.BICUBIC):
    """Pillow's 8-bit taps of output coordinates first .. first + count - 1 of one axis: [(xmin, int32 weights)]."""
    fsupport, weight = _RESAMPLE[filter]
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support, ss = fsupport * filterscale, 1.0 / filterscale
    taps = []
    for xx in range(first, first + count):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = weight((np.arange(xmin, xmax) - center + 0.5) * ss)
        ww = 0.0
        for v in w:                                     # summed in tap order
            ww += v
        if ww != 0.0:
            w = w / ww
        taps.append((xmin, np.where(w < 0, -0.5 + w * 4194304.0, 0.5 + w * 4194304.0).astype(np.int32)))
    return taps


def _resize_crop_np(flat, plan, H, W, filter):
    out = np.empty((len(plan), H, W, 3), dtype=np.uint8)
    for b, p in enumerate(plan):
        off, h, w = int(p[0]), int(p[1]), int(p[2])
        oh, ow, y0, x0 = (int(v) for v in p[7:11])
        if not (0 <= y0 and y0 + H <= oh and 0 <= x0 and x0 + W <= ow):
            raise ValueError(f"sample {b}: window ({y0}, {x0}, {H}, {W}) leaves the output size ({oh}, {ow})")
        src = flat[off:off + h * w * 3].reshape(h, w, 3).astype(np.int64)
        tx, ty = resample_taps(w, p[3], p[5], ow, x0, W, filter), resample_taps(h, p[4], p[6], oh, y0, H, filter)
        r0, r1 = ty[0][0], ty[-1][0] + len(ty[-1][1])
        tmp = np.empty((r1 - r0, W, 3), dtype=np.int64)
        for x, (xmin, k) in enumerate(tx):                  # horizontal pass, rounded to uint8
            acc = (1 << 21) + np.tensordot(src[r0:r1, xmin:xmin + len(k)], k.astype(np.int64), axes=([1], [0]))
            tmp[:, x] = np.clip(acc >> 22, 0, 255)
        for y, (ymin, k) in enumerate(ty):                  # vertical pass over those rows
            acc = (1 << 21) + np.tensordot(k.astype(np.int64), tmp[ymin - r0:ymin - r0 + len(k)], axes=([0], [0]))
            out[b, y] = np.clip(acc >> 22, 0, 255)
        if p[11]:
            out[b] = out[b, :, ::-1]
    return out


def resize_crop(flat, plan, H, W, device=False, workspace=None, filter=Image.BICUBIC):
    """uint8 [B][H][W][3]: per sample PIL's Image.resize((ow, oh), filter, box=box) of its frame in `flat`, cropped to the window
    (y0, x0, H, W) and mirrored, bit for bit.  plan = resize_plan(...).  device=False: the numpy referee (flat a numpy uint8 array);
    device=True: ppf_resize_crop_u8 (flat a uint8 CUDA tensor; no fallback)."""
    plan = np.ascontiguousarray(plan, dtype=np.float64).reshape(-1, RC_WORDS)
    if not device:
        return _resize_crop_np(np.asarray(flat, dtype=np.uint8).reshape(-1), plan, H, W, filter)
    from . import _lib
    if not (isinstance(flat, torch.Tensor) and flat.is_cuda and flat.dtype == torch.uint8 and flat.is_contiguous()):
        raise RuntimeError("resize_crop(device=True) needs a contiguous uint8 CUDA tensor of frames (no CPU fallback path)")
    B = len(plan)
    need = resize_workspace_bytes(plan, H, W, filter, flat.numel())
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, dtype=torch.uint8, device=flat.device)
    plan_dev = torch.from_numpy(plan).to(flat.device)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=flat.device)
    _lib.call("ppf_resize_crop_u8", flat, flat.numel(), plan.ctypes.data, plan_dev, B, H, W, int(filter), workspace, workspace.numel(), out)
    return out


def resize_workspace_bytes(plan, H, W, filter, flat_bytes):
    """Bytes of device workspace ppf_resize_crop_u8 needs for this plan; an invalid plan raises with the library's message."""
    from . import _lib
    plan = np.ascontiguousarray(plan, dtype=np.float64).reshape(-1, RC_WORDS)
    need = _lib.lib().ppf_resize_crop_workspace_bytes(plan.ctypes.data, len(plan), H, W, int(filter), int(flat_bytes))
    if need == 0:
        raise RuntimeError("ppf_resize_crop_workspace_bytes: " + _lib.lib().ppf_last_error().decode())
    return need


def aug_plan(draws, H, W):
    """fp64 [B][AUG_SLOTS][AUG_WORDS] = (op index in RandAugment.OPS or AUG_SKIP, resample filter, p0 .. p5) from RandAugment.draw()
    plans of B samples of H x W frames: p0 is the op's parameter, or p0 .. p5 the affine matrix PIL would build (the rotation's sine and
    cosine are taken here, as Image.rotate takes them)."""
    plan = np.zeros((len(draws), AUG_SLOTS, AUG_WORDS), dtype=np.float64)
    plan[:, :, 0] = AUG_SKIP
    for b, slots in enumerate(draws):
        if len(slots) > AUG_SLOTS:
            raise ValueError(f"{len(slots)} RandAugment ops per image: the device path takes {AUG_SLOTS}")
        for s, (name, param, resample) in enumerate(slots):
            if name is None:
                continue
            if resample not in (Image.BILINEAR, Image.BICUBIC):
                raise ValueError(f"resample filter {resample}: the device path takes BILINEAR and BICUBIC")
            m = (float(param), 0.0, 0.0, 0.0, 0.0, 0.0)
            if name == "Rotate":
                angle = param % 360.0
                if angle == 0:
                    continue                            # Image.rotate returns a copy
                angle = -math.radians(angle)
                m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
                cx, cy = W / 2, H / 2
                m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
                m[2] += cx
                m[5] += cy
            elif name == "ShearX":
                m = (1.0, param, 0.0, 0.0, 1.0, 0.0)
            elif name == "ShearY":
                m = (1.0, 0.0, 0.0, param, 1.0, 0.0)
            elif name == "TranslateXRel":
                m = (1.0, 0.0, param * W, 0.0, 1.0, 0.0)
            elif name == "TranslateYRel":
                m = (1.0, 0.0, 0.0, 0.0, 1.0, param * H)
            plan[b, s, 0], plan[b, s, 1] = RandAugment.OPS.index(name), resample
            plan[b, s, 2:] = m
    return plan


def _luma(img):
    i = img.astype(np.int64)
    return ((i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def _blend(a, b, factor):
    """Image.blend(a, b, factor) on uint8 arrays: C float arithmetic and a truncation, clamped only when the factor leaves [0, 1]."""
    f = np.float32(factor)
    a = a.astype(np.int32)
    t = a.astype(np.float32) + f * (b.astype(np.int32) - a).astype(np.float32)
    if not 0.0 <= factor <= 1.0:
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.uint8)


def _smooth(img):
    """ImageFilter.SMOOTH: fp32 3 x 3 sums with 0.5 added first, truncated; the one-pixel border is copied."""
    out = img.copy()
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)).reshape(3, 3)
    f = img.astype(np.float32)
    H, W = img.shape[:2]
    if H < 3 or W < 3:
        return out
    ss = np.full((H - 2, W - 2, 3), 0.5, dtype=np.float32)
    for r in (2, 1, 0):                                   # row y + 1 first, as the C loop
        row = f[r:r + H - 2]
        ss = ss + (row[:, 0:W - 2] * k[r, 0] + row[:, 1:W - 1] * k[r, 1] + row[:, 2:W] * k[r, 2])
    out[1:-1, 1:-1] = np.clip(ss, np.float32(0), np.float32(255)).astype(np.uint8)
    return out


def _cubic(v1, v2, v3, v4, d):
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return v2 + d * (p2 + d * (p3 + d * p4))


def _affine_np(img, m, resample, fill):
    """Image.transform(size, AFFINE, m, resample, fillcolor=fill): every output pixel's centre is mapped in closed form in double."""
    H, W = img.shape[:2]
    xs, ys = (np.arange(W) + 0.5)[None, :], (np.arange(H) + 0.5)[:, None]
    xin, yin = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    x, y = x.astype(np.int64), y.astype(np.int64)
    src = img.astype(np.int64)

    def row(yy, fn):
        cols = [src[np.clip(yy, 0, H - 1), np.clip(x + j, 0, W - 1)] for j in range(fn[0], fn[1])]
        return fn[2](*cols)
    if resample == Image.BILINEAR:
        fn = (0, 2, lambda a, b: a + (b - a) * dx)
        v1 = row(y, fn)
        ok = ((y + 1 >= 0) & (y + 1 < H))[..., None]
        v2 = np.where(ok, row(y + 1, fn), v1)
        v = v1 + (v2 - v1) * dy
    else:
        fn = (-1, 3, lambda a, b, c, d: _cubic(a, b, c, d, dx))
        v1 = row(y - 1, fn)
        v2 = np.where(((y >= 0) & (y < H))[..., None], row(y, fn), v1)
        v3 = np.where(((y + 1 >= 0) & (y + 1 < H))[..., None], row(y + 1, fn), v2)
        v4 = np.where(((y + 2 >= 0) & (y + 2 < H))[..., None], row(y + 2, fn), v3)
        v = _cubic(v1, v2, v3, v4, dy)
    v = _AFFINE_ROUND[resample](v)
    return np.where(inside[..., None], v, np.asarray(fill, dtype=np.uint8)).astype(np.uint8)


_AFFINE_ROUND = {Image.BILINEAR: lambda v: np.clip(v, 0, 255).astype(np.uint8),
                 Image.BICUBIC: lambda v: np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, v.astype(np.int64)))}


def _table_lut(op, p0, img):
    """uint8 [3][256]: the per-channel table of one table op on one frame."""
    name = RandAugment.OPS[op]
    i = np.arange(256, dtype=np.int64)
    if name == "Invert":
        lut = 255 - i
    elif name == "PosterizeIncreasing":
        lut = i & ~((1 << (8 - int(p0))) - 1)
    elif name == "SolarizeIncreasing":
        lut = np.where(i < int(p0), i, 255 - i)
    elif name == "SolarizeAdd":
        lut = np.where(i < 128, np.minimum(255, i + int(p0)), i)
    elif name == "BrightnessIncreasing":
        lut = _blend(np.zeros(256, dtype=np.uint8), i.astype(np.uint8), p0)
    elif name == "ContrastIncreasing":
        mean = int(_luma(img).astype(np.int64).sum() / (img.shape[0] * img.shape[1]) + 0.5)
        lut = _blend(np.full(256, mean, dtype=np.uint8), i.astype(np.uint8), p0)
    else:
        luts = []
        for c in range(3):
            h = np.bincount(img[..., c].reshape(-1), minlength=256).astype(np.int64)
            nz = np.nonzero(h)[0]
            lut = i.copy()
            if name == "AutoContrast":
                lo, hi = int(nz[0]), int(nz[-1])
                if hi > lo:
                    scale = 255.0 / (hi - lo)
                    offset = -lo * scale
                    lut = np.clip((i * scale + offset).astype(np.int64), 0, 255)
            else:
                step = (int(h.sum()) - int(h[nz[-1]])) // 255
                if len(nz) > 1 and step:
                    lut = np.minimum((step // 2 + np.concatenate(([0], np.cumsum(h)[:-1]))) // step, 255)
            luts.append(lut)
        return np.stack(luts).astype(np.uint8)
    return np.broadcast_to(lut.astype(np.uint8), (3, 256))


def _aug_np(img, op, resample, p, fill):
    name = RandAugment.OPS[op]
    if name in _AFFINE_OPS:
        return _affine_np(img, p, resample, fill)
    if name == "ColorIncreasing":
        return _blend(np.repeat(_luma(img)[..., None], 3, axis=2), img, p[0])
    if name == "SharpnessIncreasing":
        return _blend(_smooth(img), img, p[0])
    lut = _table_lut(op, p[0], img)
    return np.stack([lut[c][img[..., c]] for c in range(3)], axis=2)


def randaugment_apply(frames, plan, fill, device=False):
    """uint8 [B][H][W][3] frames after the ops of plan = aug_plan(...), each bit-equal to RandAugment._apply_drawn under Pillow.
    device=False: the numpy referee; device=True: the ppf_aug_* kernels (uint8 CUDA tensor; no fallback)."""
    plan = np.ascontiguousarray(plan, dtype=np.float64).reshape(-1, AUG_SLOTS, AUG_WORDS)
    fill = tuple(int(v) for v in fill)
    if not device:
        out = np.array(frames, dtype=np.uint8)
        for b in range(len(plan)):
            for s in range(AUG_SLOTS):
                if int(plan[b, s, 0]) != AUG_SKIP:
                    out[b] = _aug_np(out[b], int(plan[b, s, 0]), int(plan[b, s, 1]), plan[b, s, 2:], fill)
        return out
    from . import _lib
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4):
        raise RuntimeError("randaugment_apply(device=True) needs a contiguous uint8 CUDA tensor [B, H, W, 3] (no CPU fallback path)")
    B, H, W, _ = frames.shape
    if len(plan) != B:
        raise ValueError(f"plan of {len(plan)} samples for a batch of {B}")
    plan_dev = torch.from_numpy(plan).to(frames.device)
    hist = torch.empty((B, 3, 256), dtype=torch.int32, device=frames.device)
    lut = torch.empty((B, 3, 256), dtype=torch.uint8, device=frames.device)
    cur, nxt = frames, None
    for s in range(AUG_SLOTS):
        ops = plan[:, s, 0].astype(np.int64)
        if (ops == AUG_SKIP).all():
            continue
        nxt = torch.empty_like(frames) if nxt is None else nxt
        _lib.call("ppf_aug_hist", cur, plan_dev, s, B, H, W, hist)
        _lib.call("ppf_aug_lut_build", hist, plan_dev, s, B, H, W, lut)
        _lib.call("ppf_aug_apply", cur, plan_dev, s, lut, B, H, W, nxt)
        if (ops == RandAugment.OPS.index("SharpnessIncreasing")).any():
            _lib.call("ppf_aug_sharpness", cur, plan_dev, s, B, H, W, nxt)
        if np.isin(ops, [RandAugment.OPS.index(n) for n in _AFFINE_OPS]).any():
            _lib.call("ppf_aug_affine", cur, plan_dev, s, B, H, W, fill[0], fill[1], fill[2], nxt)
        cur, nxt = nxt, (cur if cur is not frames else None)
    return cur


# ------------------------------------------------------------------------------------------------ PartsWorld
# A data set the project renders itself: classes are rows of part attributes, and every image knows its object's box, its parts' places
# and the class table (the idea of FunnyBirds, Hesse et al., ICCV 2023).  The contract is written out in include/ppf_hip.h and the shared
# arithmetic in csrc/synth_plan.h, whose constants are mirrored here; the functions below are the numpy referees (device=False) of
# ppf_synth_scene / ppf_synth_render, which equal them bit for bit.  Integers only.
SYNTH_WORDS = 168                                     # PPF_SYNTH_WORDS of the header
SYNTH_SHAPES, SYNTH_COLOURS, SYNTH_ATTRS = ("disk", "square", "diamond", "ring"), 6, 24
SYNTH_PALETTE = np.array([(220, 40, 40), (40, 180, 60), (50, 80, 220), (235, 210, 40), (200, 60, 200), (40, 200, 210)], dtype=np.uint8)
SYNTH_BODY = np.array((112, 112, 112), dtype=np.uint8)
SYNTH_BOX, SYNTH_PART0, SYNTH_DIST0, SYNTH_NODE0, SYNTH_PRIM_WORDS = 1, 5, 45, 85, 5          # (on, cx, cy, r, attribute) per primitive
SYNTH_STREAM_SCENE, SYNTH_STREAM_NOISE = 0xC0000001, 0xC0000002
SYNTH_ITEM_PART0, SYNTH_ITEM_DIST0, SYNTH_ITEM_NODE0 = 1, 9, 32
SYNTH_SLOT_CELLS = (0, 2, 6, 8, 1, 3, 5, 7)
_SPEC_FIELDS = ("classes", "parts", "distractors", "height", "width", "n_train", "n_test", "test_id_base", "seed", "noise", "grid")


class PartsWorldSpec:
    """The settings of a PartsWorld, nothing else: C classes of K parts, D distractors, the frame, the split sizes, the id of the first
    test image, the seed, the pixel-noise amplitude and the background's cells per side.  Round-trips through JSON."""

    def __init__(self, classes=20, parts=4, distractors=3, height=256, width=256, n_train=4096, n_test=1024, test_id_base=1 << 32, seed=0,
                 noise=8, grid=4):
        for k in _SPEC_FIELDS:
            v = locals()[k]
            if isinstance(v, bool) or int(v) != v:
                raise ValueError(f"PartsWorldSpec: {k}={v!r} is not an integer")
            setattr(self, k, int(v))
        self.validate()

    def validate(self):
        """Refuses by name what ppf_synth_scene / ppf_synth_render refuse, and what only the data set sees."""
        C, K = self.classes, self.parts
        if not 1 <= K <= 8:
            raise ValueError(f"PartsWorldSpec: parts K={K} outside [1, 8]")
        if not 0 <= self.distractors <= 8:
            raise ValueError(f"PartsWorldSpec: distractors D={self.distractors} outside [0, 8]")
        if not 2 <= C <= 1024:
            raise ValueError(f"PartsWorldSpec: classes C={C} outside [2, 1024]")
        if C > SYNTH_ATTRS ** K:
            raise ValueError(f"PartsWorldSpec: classes C={C} exceed A^K = {SYNTH_ATTRS ** K} rows of K={K} attributes (C > A^K)")
        if not 32 <= self.height <= 1024:
            raise ValueError(f"PartsWorldSpec: height H={self.height} outside [32, 1024]")
        if not 32 <= self.width <= 1024 or self.width % 16:
            raise ValueError(f"PartsWorldSpec: width W={self.width} outside [32, 1024] or not a multiple of 16")
        if not 1 <= self.grid <= 8:
            raise ValueError(f"PartsWorldSpec: grid g={self.grid} outside [1, 8]")
        if not 0 <= self.noise <= 32:
            raise ValueError(f"PartsWorldSpec: noise={self.noise} amplitude outside [0, 32]")
        if self.n_train < 1 or self.n_test < 1 or not 0 <= self.seed < 1 << 64:
            raise ValueError(f"PartsWorldSpec: n_train={self.n_train}, n_test={self.n_test} must be >= 1 and seed={self.seed} in [0, 2^64)")
        if self.test_id_base < self.n_train or self.test_id_base + self.n_test > 1 << 62:
            raise ValueError(f"PartsWorldSpec: test_id_base={self.test_id_base} must leave the train ids 0 .. {self.n_train - 1} alone and stay below 2^62")

    def to_dict(self):
        return {k: getattr(self, k) for k in _SPEC_FIELDS}

    def to_json(self):
        import json
        return json.dumps(self.to_dict())

    @classmethod
    def from_dict(cls, d):
        unknown = sorted(set(d) - set(_SPEC_FIELDS))
        if unknown:
            raise ValueError(f"PartsWorldSpec: unknown settings {unknown}")
        return cls(**d)

    @classmethod
    def from_json(cls, text):
        import json
        return cls.from_dict(json.loads(text))

    def __eq__(self, other):
        return isinstance(other, PartsWorldSpec) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "PartsWorldSpec(" + ", ".join(f"{k}={getattr(self, k)}" for k in _SPEC_FIELDS) + ")"


def partsworld_class_table(spec):
    """class_parts int32 [C][K]: part k of class c is digit k of c in base A = 24 -- a function of the spec alone, rows pairwise distinct
    because C <= A^K (PartsWorldSpec.validate refuses anything else)."""
    spec.validate()
    c = np.arange(spec.classes, dtype=np.int64)[:, None]
    return ((c // SYNTH_ATTRS ** np.arange(spec.parts, dtype=np.int64)[None, :]) % SYNTH_ATTRS).astype(np.int32)


def _synth_ids(ids):
    ids = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64).reshape(-1)
    if (ids < 0).any():
        raise ValueError("PartsWorld: image ids are >= 0")
    return ids


def _synth_draw(spec, ids, item, stream):
    """uint64 [..., 4]: the four 24-bit draws of Philox counter (item, stream, id low, id high) under the spec's seed."""
    from .interpret import philox4x32_10
    ids = ids.astype(np.uint64)
    item = np.broadcast_to(np.asarray(item, dtype=np.uint64), ids.shape)
    ctr = np.stack([item, np.full(ids.shape, stream, dtype=np.uint64), ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32)], axis=-1)
    key = np.array([spec.seed & 0xFFFFFFFF, spec.seed >> 32], dtype=np.uint64)
    return (philox4x32_10(ctr, key) >> np.uint32(8)).astype(np.uint64)


def _synth_range(u, n):
    return ((u * np.asarray(n, dtype=np.int64).astype(np.uint64)) >> np.uint64(24)).astype(np.int64)


def _device_ids(ids):
    if isinstance(ids, torch.Tensor) and ids.is_cuda:
        return ids
    return torch.from_numpy(_synth_ids(ids)).cuda()


def partsworld_scene_from_ids(spec, ids, device=False):
    """The scene table int32 [B][SYNTH_WORDS] of image ids (include/ppf_hip.h): label, box, parts, distractors, background nodes -- a pure
    function of (spec, id), and the annotation.  device=False: the numpy referee; device=True: ppf_synth_scene (a CUDA tensor comes back;
    no fallback)."""
    spec.validate()
    if device:
        from . import ops
        return ops.synth_scene(spec, _device_ids(ids))
    ids = _synth_ids(ids)
    B, H, W, K = len(ids), spec.height, spec.width, spec.parts
    scene = np.zeros((B, SYNTH_WORDS), dtype=np.int64)
    label = (ids % spec.classes).astype(np.int64)
    scene[:, 0] = label
    m = min(H, W)
    wo = _synth_draw(spec, ids, 0, SYNTH_STREAM_SCENE)
    hs_min, hs_max = 5 * m // 16, 13 * m // 32
    hs = hs_min + _synth_range(wo[:, 0], hs_max - hs_min + 1)
    ox, oy = hs + _synth_range(wo[:, 1], W - 2 * hs), hs + _synth_range(wo[:, 2], H - 2 * hs)
    scene[:, SYNTH_BOX:SYNTH_BOX + 4] = np.stack([ox - hs, oy - hs, ox + hs + 1, oy + hs + 1], axis=1)
    forced = _synth_range(wo[:, 3], K)
    p = (2 * hs + 1) // 3
    j = (p - 1) // 8
    r = (p - 1) // 2 - j
    table = partsworld_class_table(spec)
    for k in range(K):
        w = _synth_draw(spec, ids, SYNTH_ITEM_PART0 + k, SYNTH_STREAM_SCENE)
        cell, at = SYNTH_SLOT_CELLS[k], SYNTH_PART0 + SYNTH_PRIM_WORDS * k
        scene[:, at] = (w[:, 0] < (3 << 22)) | (forced == k)
        scene[:, at + 1] = ox + (cell % 3 - 1) * p + _synth_range(w[:, 1], 2 * j + 1) - j
        scene[:, at + 2] = oy + (cell // 3 - 1) * p + _synth_range(w[:, 2], 2 * j + 1) - j
        scene[:, at + 3] = r
        scene[:, at + 4] = table[label, k]
    for d in range(spec.distractors):
        w0 = _synth_draw(spec, ids, SYNTH_ITEM_DIST0 + 2 * d, SYNTH_STREAM_SCENE)
        w1 = _synth_draw(spec, ids, SYNTH_ITEM_DIST0 + 2 * d + 1, SYNTH_STREAM_SCENE)
        at = SYNTH_DIST0 + SYNTH_PRIM_WORDS * d
        rd = m // 16 + _synth_range(w0[:, 2], m // 8 - m // 16 + 1)
        scene[:, at] = w0[:, 0] < (1 << 23)
        scene[:, at + 1] = rd + _synth_range(w1[:, 0], W - 2 * rd)
        scene[:, at + 2] = rd + _synth_range(w1[:, 1], H - 2 * rd)
        scene[:, at + 3] = rd
        scene[:, at + 4] = _synth_range(w0[:, 1], SYNTH_ATTRS)
    draws = 3 * (spec.grid + 1) ** 2
    for c4 in range(-(-draws // 4)):
        w = _synth_draw(spec, ids, SYNTH_ITEM_NODE0 + c4, SYNTH_STREAM_SCENE)
        for i in range(4):
            e = 4 * c4 + i
            if e < draws:
                scene[:, SYNTH_NODE0 + e // 3] |= (64 + _synth_range(w[:, i], 128)) << (8 * (e % 3))
    return scene.astype(np.int32)


def _synth_inside(shape, dx, dy, r):
    ax, ay = np.abs(dx), np.abs(dy)
    d2, r2 = ax * ax + ay * ay, r * r
    box = (ax <= r) & (ay <= r)
    if shape == 0:
        return box & (d2 <= r2)
    if shape == 1:
        return box
    if shape == 2:
        return box & (ax + ay <= r)
    return box & (d2 <= r2) & ~((16 * d2 > r2) & (4 * d2 < r2))


def _synth_render_np(spec, row, img_id):
    """(frame uint8 [H][W][3], partmap uint8 [H][W]) of one scene row."""
    H, W, g = spec.height, spec.width, spec.grid
    ys, xs = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    row = row.astype(np.int64)
    L, ch, cw = g + 1, -(-H // g), -(-W // g)
    i, ry, j, rx = ys // ch, ys % ch, xs // cw, xs % cw
    nodes = row[SYNTH_NODE0:SYNTH_NODE0 + L * L].reshape(L, L)
    frame = np.empty((H, W, 3), dtype=np.int64)
    for c in range(3):
        n = (nodes >> (8 * c)) & 255
        frame[..., c] = ((ch - ry) * ((cw - rx) * n[i, j] + rx * n[i, j + 1]) + ry * ((cw - rx) * n[i + 1, j] + rx * n[i + 1, j + 1])) // (ch * cw)
    top = np.zeros((H, W), dtype=np.uint8)

    def paint(at, code):
        on, cx, cy, r, attr = (int(v) for v in row[at:at + SYNTH_PRIM_WORDS])
        if on:
            a = attr % SYNTH_ATTRS
            inside = _synth_inside(a // SYNTH_COLOURS, xs - cx, ys - cy, r)
            frame[inside] = SYNTH_PALETTE[a % SYNTH_COLOURS]
            top[inside] = code
    for d in range(spec.distractors):
        paint(SYNTH_DIST0 + SYNTH_PRIM_WORDS * d, 1)
    x0, y0, x1, y1 = (int(v) for v in row[SYNTH_BOX:SYNTH_BOX + 4])
    body = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    frame[body] = SYNTH_BODY
    top[body] = 2
    for k in range(spec.parts):
        paint(SYNTH_PART0 + SYNTH_PRIM_WORDS * k, 3 + k)
    if spec.noise > 0:
        w = _synth_draw(spec, np.full(H * W, img_id, dtype=np.int64), np.arange(H * W, dtype=np.uint64), SYNTH_STREAM_NOISE)
        frame = np.clip(frame + (_synth_range(w[:, :3], 2 * spec.noise + 1) - spec.noise).reshape(H, W, 3), 0, 255)
    return frame.astype(np.uint8), top


def partsworld_render(spec, scene, ids, device=False, partmap=False):
    """uint8 [B][H][W][3] frames of a scene table (the ids carry the pixel noise), and with partmap also uint8 [B][H][W], the code of the
    topmost primitive: 0 background, 1 distractor, 2 body, 3 + k part k.  device=False: the numpy referee; device=True: ppf_synth_render
    (scene a CUDA int32 tensor or a host table; CUDA tensors come back; no fallback)."""
    spec.validate()
    if device:
        from . import ops
        ids = _device_ids(ids)
        if not isinstance(scene, torch.Tensor):
            scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.int32)).to(ids.device)
        return ops.synth_render(spec, scene, ids, partmap=bool(partmap))
    ids = _synth_ids(ids)
    scene = np.asarray(scene.cpu() if isinstance(scene, torch.Tensor) else scene, dtype=np.int32).reshape(len(ids), SYNTH_WORDS)
    frames = np.empty((len(ids), spec.height, spec.width, 3), dtype=np.uint8)
    maps = np.empty((len(ids), spec.height, spec.width), dtype=np.uint8)
    for b, img_id in enumerate(ids):
        frames[b], maps[b] = _synth_render_np(spec, scene[b], int(img_id))
    return (frames, maps) if partmap else frames


EDIT_COPY, EDIT_PARTS_OFF, EDIT_DISTRACTORS_OFF, EDIT_BACKGROUND, EDIT_PART_ATTR = range(5)     # the ops of ppf_synth_edit (include/ppf_hip.h)


def _edit_valid(op, arg, K, Dn):
    a = arg & 0xFFFFFFFF                                 # as the rule reads it: a negative arg is above every mask and colour
    if op == EDIT_COPY:
        return True
    if op == EDIT_PARTS_OFF:
        return a >> K == 0
    if op == EDIT_DISTRACTORS_OFF:
        return a >> Dn == 0
    if op == EDIT_BACKGROUND:
        return a <= 0xFFFFFF
    if op == EDIT_PART_ATTR:
        return (a & 255) < K and (a >> 8) < SYNTH_ATTRS
    return False


def partsworld_edit(spec, scene, edits, device=False, check=True):
    """(out int32 [B][E][SYNTH_WORDS], changed int32 [B][E]) of a scene table int32 [B][SYNTH_WORDS] and edits int32 [B][E][2] = (op, arg):
    every edit applied to the image's own row (include/ppf_hip.h, ppf_synth_edit).  changed: 1 when the edit alters a word of a primitive
    that is on before or after it, or a node; 0 when it alters nothing that is drawn; -1 for an invalid edit, whose row is copied.
    device=False: the numpy referee (it reports -1 and does not raise); device=True: ops.synth_edit (CUDA tensors come back; with check
    it raises on any -1 after its one read; no fallback)."""
    spec.validate()
    if device:
        from . import ops
        dev = scene.device if isinstance(scene, torch.Tensor) and scene.is_cuda else torch.device("cuda")
        to_dev = lambda t: t if isinstance(t, torch.Tensor) and t.is_cuda else torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dev)
        return ops.synth_edit(spec, to_dev(scene), to_dev(edits), check=check)
    host = lambda t: np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, dtype=np.int32)
    scene, edits = host(scene), host(edits)
    B = scene.shape[0]
    if scene.shape != (B, SYNTH_WORDS) or edits.ndim != 3 or edits.shape[0] != B or edits.shape[1] < 1 or edits.shape[2] != 2:
        raise ValueError(f"partsworld_edit: scene must be [B, {SYNTH_WORDS}] and edits [B, E >= 1, 2], got {scene.shape} and {edits.shape}")
    K, Dn, nodes = spec.parts, spec.distractors, (spec.grid + 1) ** 2
    E = edits.shape[1]
    out = np.repeat(scene[:, None, :], E, axis=1).copy()
    changed = np.zeros((B, E), dtype=np.int32)
    for b in range(B):
        for e in range(E):
            op, arg = int(edits[b, e, 0]), int(edits[b, e, 1])
            if not _edit_valid(op, arg, K, Dn):
                changed[b, e] = -1
                continue
            row = out[b, e]
            if op in (EDIT_PARTS_OFF, EDIT_DISTRACTORS_OFF):
                base = SYNTH_PART0 if op == EDIT_PARTS_OFF else SYNTH_DIST0
                for k in range(K if op == EDIT_PARTS_OFF else Dn):
                    if arg >> k & 1:
                        changed[b, e] |= int(row[base + SYNTH_PRIM_WORDS * k] != 0)       # switching off what is off changes nothing
                        row[base + SYNTH_PRIM_WORDS * k] = 0
            elif op == EDIT_BACKGROUND:
                changed[b, e] = int((row[SYNTH_NODE0:SYNTH_NODE0 + nodes] != arg).any())
                row[SYNTH_NODE0:SYNTH_NODE0 + nodes] = arg
            elif op == EDIT_PART_ATTR:
                at = SYNTH_PART0 + SYNTH_PRIM_WORDS * (arg & 255)
                changed[b, e] = int(row[at] != 0 and row[at + 4] != arg >> 8)
                row[at + 4] = arg >> 8
    return out, changed


def partsworld_view_src(i, n, size):
    """PPF_VIEW_SRC of include/ppf_hip.h: the frame coordinate in [0, n) a view coordinate i in [0, size) takes its primitive code from,
    ((2 i + 1) n) // (2 size) -- nearest by pixel centre.  Integers (numpy int64 for arrays)."""
    return ((2 * np.asarray(i, dtype=np.int64) + 1) * int(n)) // (2 * int(size))


def partsworld_view_partmap(partmap, size):
    """uint8 [B][size][size]: the partmap [B][H][W] as the square view of `size` sees it (the view rule)."""
    pm = np.asarray(partmap.cpu() if isinstance(partmap, torch.Tensor) else partmap, dtype=np.uint8)
    i = np.arange(size)
    return pm[:, partsworld_view_src(i, pm.shape[1], size)[:, None], partsworld_view_src(i, pm.shape[2], size)[None, :]]


def partsworld_view(spec, frames_u8, size, finisher, workspace=None):
    """The model's square view fp32 [N, 3, size, size] of rendered frames uint8 [N][H][W][3] on the device: resize_plan over the frames'
    offsets, resize_crop(device=True, filter=Image.BILINEAR), then the GpuFinisher -- the calls DeviceAugLoader(square=True) makes, so the
    view of an unedited frame is bit-equal to what that loader yields for the image.  No new kernel.  workspace: a uint8 CUDA scratch
    tensor to reuse (resize_workspace_bytes says how large; a larger one is made when it is too small)."""
    H, W = spec.height, spec.width
    if not (isinstance(frames_u8, torch.Tensor) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
            and frames_u8.dim() == 4 and tuple(frames_u8.shape[1:]) == (H, W, 3)):
        raise RuntimeError(f"partsworld_view needs a contiguous uint8 CUDA tensor [N, {H}, {W}, 3] (no CPU fallback path)")
    if getattr(finisher, "re_prob", 0.0) > 0:
        raise ValueError("partsworld_view: the finisher must not erase (GpuFinisher(re_prob=0.0)): this is the eval view")
    N, S = frames_u8.shape[0], int(size)
    plan = resize_plan(np.arange(N, dtype=np.int64) * (H * W * 3), np.tile(np.array([[H, W]], dtype=np.int32), (N, 1)), [(0, 0, W, H)] * N,
                       [(S, S)] * N, [(0, 0)] * N, [0] * N)
    return finisher(resize_crop(frames_u8.reshape(-1), plan, S, S, device=True, workspace=workspace, filter=Image.BILINEAR))


class PartsWorldAnnotation:
    """What interpret.CubParts offers its callers, from the scene table: id_to_bbox {id: (x0, y0, x1, y1)}, id_to_part_loc {id: [[part id
    from 1, x, y] of the visible parts]}, part_names {'1': ...}; and image_sizes {id: (W, H)}, class_parts int32 [C][K], n_parts = K, the
    ids and the scene table itself."""

    def __init__(self, spec, ids, scene):
        K = spec.parts
        self.spec, self.ids, self.scene, self.n_parts, self.class_parts = spec, ids, scene, K, partsworld_class_table(spec)
        self.part_names = {str(k + 1): f"part {k + 1}" for k in range(K)}
        self.id_to_bbox, self.id_to_part_loc, self.image_sizes = {}, {}, {}
        for i, row in zip(ids.tolist(), scene.tolist()):
            self.id_to_bbox[i] = tuple(row[SYNTH_BOX:SYNTH_BOX + 4])
            parts = (row[SYNTH_PART0 + SYNTH_PRIM_WORDS * k:SYNTH_PART0 + SYNTH_PRIM_WORDS * (k + 1)] for k in range(K))
            self.id_to_part_loc[i] = [[k + 1, p[1], p[2]] for k, p in enumerate(parts) if p[0]]
            self.image_sizes[i] = (spec.width, spec.height)


class PartsWorld:
    """A map-style data set like Cub2011 over a PartsWorldSpec: train images have ids 0 .. n_train - 1, test images test_id_base .. ;
    label = id % C.  __getitem__ renders the frame with the numpy referee and hands it over as a PIL image, so the CPU loaders work as for
    a file-backed set; DeviceDataset renders the whole set on the device instead.  original(id) and image_size(id) stand in for files."""

    def __init__(self, spec=None, train=True, transform=None, return_id=False):
        self.spec = spec if spec is not None else PartsWorldSpec()
        self.spec.validate()
        self.train, self.transform, self.return_id = bool(train), transform, return_id
        n, base = (self.spec.n_train, 0) if self.train else (self.spec.n_test, self.spec.test_id_base)
        self.ids = base + np.arange(n, dtype=np.int64)
        self.labels = (self.ids % self.spec.classes).astype(np.int64)
        self._annotation = None

    def __len__(self):
        return len(self.ids)

    def original(self, img_id):
        """uint8 [H][W][3]: the frame of image id, as DeviceDataset holds it."""
        ids = np.array([int(img_id)], dtype=np.int64)
        return partsworld_render(self.spec, partsworld_scene_from_ids(self.spec, ids), ids)[0]

    def image_size(self, img_id):
        return (self.spec.width, self.spec.height)

    def __getitem__(self, idx):
        img_id = int(self.ids[idx])
        img = Image.fromarray(self.original(img_id))
        if self.transform is not None:
            img = self.transform(img)
        return (img, int(self.labels[idx]), img_id) if self.return_id else (img, int(self.labels[idx]))

    def annotation(self):
        if self._annotation is None:
            self._annotation = PartsWorldAnnotation(self.spec, self.ids, partsworld_scene_from_ids(self.spec, self.ids))
        return self._annotation


def partsworld_spec_from_args(args):
    """args.partsworld when a Python caller set it (a PartsWorldSpec or its dict); else the settings file --data_path names, when that is
    an existing .json file; else the defaults."""
    spec = getattr(args, "partsworld", None)
    if spec is not None:
        return spec if isinstance(spec, PartsWorldSpec) else PartsWorldSpec.from_dict(dict(spec))
    path = getattr(args, "data_path", None)
    if path and str(path).endswith(".json") and os.path.isfile(path):
        with open(path) as f:
            return PartsWorldSpec.from_json(f.read())
    return PartsWorldSpec()


# ------------------------------------------------------------------------------------------------ tools/preprocess.py
def preprocess(x, mean, std):
    assert x.size(1) == 3
    m = torch.as_tensor(mean, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return (x - m) / s


def preprocess_input_function(x):
    return preprocess(x, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)


def undo_preprocess(x, mean, std):
    assert x.size(1) == 3
    m = torch.as_tensor(mean, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=x.dtype, device=x.device).view(1, 3, 1, 1)
    return x * s + m


def undo_preprocess_input_function(x):
    return undo_preprocess(x, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
