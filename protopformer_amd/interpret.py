"""Consumers of the eval-branch outputs: prototype activation visualisation (reference main_visualize.py:273-474)
and the part-consistency interpretability score on CUB (reference eval_interpretability.py:100-336, tools/local_parts.py).

The model side runs on the HIP kernels (`PPNet.forward` in eval mode / `push_forward`); everything here is the reference's
CPU-side post-processing restated on numpy / PIL.  OpenCV is not installed in this image, so the three cv2 primitives the
reference uses are written out from their documented definitions (unpinned against cv2 itself, tested for their properties):
`resize_cubic` = cv2.resize(..., interpolation=INTER_CUBIC) (Keys kernel a = -0.75, half-pixel centres, replicated border),
`colormap_jet` = cv2.applyColorMap(..., COLORMAP_JET) (BGR), `draw_rect` = cv2.rectangle outline."""
import math
import os

import numpy as np
import torch

from .tooling import batches_with_ids, read_once, read_rows, regroup, take_images


# ------------------------------------------------------------------------------------------------ what the passes below share
class Record:
    """Base of the result records of the passes.  A subclass declares FIELDS, the names of its tensor-valued attributes (device tensors,
    numpy arrays after cpu(); any of them may be None, and one may be a dict of tensors), and META, {name: conversion or None} of its
    plain settings (DEFAULTS: the trailing ones that may be left out).  Construction takes FIELDS then META, by position or by name."""
    FIELDS, META, DEFAULTS = (), {}, {}

    def __init__(self, *args, **kw):
        names = tuple(self.FIELDS) + tuple(self.META)
        given = {**self.DEFAULTS, **dict(zip(names, args)), **kw}
        if len(args) > len(names) or set(kw) - set(names[len(args):]) or set(names) - set(given):
            raise TypeError(f"{type(self).__name__} takes {names}, got {len(args)} positional values and {sorted(kw)}")
        for k in names:
            conv = self.META.get(k)
            setattr(self, k, given[k] if conv is None else conv(given[k]))

    def fields(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    @property
    def on_host(self):
        return not any(isinstance(t, torch.Tensor) for v in self.fields().values() for t in (v.values() if isinstance(v, dict) else (v,)))

    def cpu(self):
        """The same record with numpy arrays: every field in ONE host read (a record among the settings: one more read for it).  A record
        on the host already is returned as it is."""
        if self.on_host:
            return self
        f = self.fields()
        host = read_once({(k, j): t for k, v in f.items() for j, t in (v.items() if isinstance(v, dict) else ((None, v),))})
        return type(self)(**{k: ({j: host[k, j] for j in v} if isinstance(v, dict) else host[k, None]) for k, v in f.items()},
                          **{k: (v.cpu() if isinstance(v, Record) else v) for k, v in ((k, getattr(self, k)) for k in self.META)})


def select_prototypes(mode, ppc, classes, act_max=None, k=None, num_classes=None):
    """int64 [B, K] prototype ids of one class per image, on the device classes [B] (integers) is on; prototype j of class c is c * ppc + j.
      'own'        every prototype of the label classes[b], clamped into [0, num_classes), in id order (K = ppc);
      'predicted'  every prototype of classes[b] = the predicted class (logits.argmax(1), which the caller holds), in id order;
      'top'        the first k of the predicted class's by act_max [B, P]: a stable descending sort, so equal activations go to the
                   smaller id and a NaN sorts as torch.sort sorts it.  The slice [:, :k] is all that is done with k: each caller clamps
                   it by its own rule.
    Plain torch: it runs where its inputs are, the host included."""
    if mode not in ("own", "predicted", "top"):
        raise ValueError(f"select_prototypes: mode must be 'own', 'predicted' or 'top', got {mode!r}")
    ppc = int(ppc)
    cls = classes.clamp(0, int(num_classes) - 1) if mode == "own" else classes
    own = cls[:, None] * ppc + torch.arange(ppc, device=classes.device)[None, :]
    if mode != "top":
        return own
    return own.gather(1, torch.sort(act_max.gather(1, own), dim=1, descending=True, stable=True)[1][:, :k])


def forward_groups(ppnet, imgs, batch_size):
    """The model's forward over imgs [R, C, H, W] in consecutive groups of batch_size images: the list of the groups' output records
    (PPNet._branches without the distances).  The caller holds eval mode and no_grad."""
    return [ppnet._branches(imgs[i:i + batch_size], want_dist=False) for i in range(0, imgs.shape[0], batch_size)]


# ------------------------------------------------------------------------------------------------ activation maps
def reserved_indices(token_attn, k):
    """topk(k) + ascending sort of the rollout scores (main_visualize.py:345-346): the grid cells the reserved tokens came from."""
    return torch.topk(token_attn.reshape(token_attn.shape[0], -1), k=k, dim=-1)[1].sort(dim=-1)[0]


def expand_to_grid(acts, token_attn, k):
    """(B, P, s, s) activations of the k = s*s reserved tokens -> (B, P, g, g) on the full patch grid, zeros elsewhere
    (main_visualize.py:343-350, eval_interpretability.py:156-167)."""
    B, P = acts.shape[:2]
    n = token_attn.reshape(B, -1).shape[-1]
    g = int(round(n ** 0.5))
    idx = reserved_indices(token_attn, k)[:, None, :].expand(B, P, k)
    out = torch.zeros(B, P, n, dtype=acts.dtype, device=acts.device)
    out.scatter_(2, idx, acts.reshape(B, P, -1))
    return out.reshape(B, P, g, g)


def proto_acts_from_distances(distances, epsilon=1e-4):
    """main_visualize.py:326: log((d + 1) / (d + eps))."""
    return np.log((distances + 1) / (distances + epsilon))


@torch.no_grad()
def collect_eval_outputs(ppnet, loader, category_id=None, min_count=20):
    """main_visualize.py:306-327: run the eval branch over `loader` (until more than `min_count` samples of `category_id` were
    seen, if given).  Returns dict(token_attn (B, Np), distances (B, P, s, s), labels, pred)."""
    ppnet.eval()
    attn, dist, labels, pred = [], [], [], []
    for x, y, *_ in loader:
        logits, aux = ppnet(x.cuda() if not x.is_cuda else x)
        attn.append(aux[0].float().cpu().numpy()); dist.append(aux[1].float().cpu().numpy())
        labels.append(np.asarray(y.cpu())); pred.append(logits.argmax(1).cpu().numpy())
        if category_id is not None and int((np.concatenate(labels) == category_id).sum()) > min_count:
            break
    return dict(token_attn=np.concatenate(attn), distances=np.concatenate(dist), labels=np.concatenate(labels), pred=np.concatenate(pred))


# ------------------------------------------------------------------------------------------------ cv2 primitives, restated
def _cubic_weights(f, a=-0.75):
    w0 = ((a * (f + 1) - 5 * a) * (f + 1) + 8 * a) * (f + 1) - 4 * a
    w1 = ((a + 2) * f - (a + 3)) * f * f + 1
    w2 = ((a + 2) * (1 - f) - (a + 3)) * (1 - f) * (1 - f) + 1
    return np.stack([w0, w1, w2, 1.0 - w0 - w1 - w2], axis=-1)


def _resize_axis(a, size, axis):
    n = a.shape[axis]
    s = (np.arange(size) + 0.5) * (n / size) - 0.5
    i0 = np.floor(s).astype(np.int64)
    w = _cubic_weights(s - i0)                                         # (size, 4)
    idx = np.clip(i0[:, None] + np.arange(-1, 3)[None, :], 0, n - 1)   # replicated border
    taken = np.take(a, idx.reshape(-1), axis=axis)
    shape = list(a.shape); shape[axis:axis + 1] = [size, 4]
    taken = taken.reshape(shape)
    wshape = [1] * len(shape); wshape[axis] = size; wshape[axis + 1] = 4
    return (taken * w.reshape(wshape)).sum(axis=axis + 1)


def resize_cubic(a, size):
    """cv2.resize(a, (size, size), interpolation=cv2.INTER_CUBIC) for a 2-D float array."""
    a = np.asarray(a, dtype=np.float64)
    return _resize_axis(_resize_axis(a, size, 0), size, 1).astype(np.float32)


def colormap_jet(gray_u8):
    """cv2.applyColorMap(gray, cv2.COLORMAP_JET): uint8 (...,) -> uint8 (..., 3) in B, G, R order."""
    x = np.asarray(gray_u8, dtype=np.float64) / 255.0
    r = np.clip(1.5 - np.abs(4 * x - 3), 0, 1)
    g = np.clip(1.5 - np.abs(4 * x - 2), 0, 1)
    b = np.clip(1.5 - np.abs(4 * x - 1), 0, 1)
    return np.stack([b, g, r], axis=-1).__mul__(255).round().astype(np.uint8)


def draw_rect(img, start_xy, end_xy, color, thickness=2):
    """cv2.rectangle outline on a copy of an (H, W, 3) image; start / end are (x, y) corners."""
    out = np.array(img, copy=True)
    (x0, y0), (x1, y1) = start_xy, end_xy
    H, W = out.shape[:2]
    x0, x1, y0, y1 = max(0, min(x0, x1)), min(W - 1, max(x0, x1)), max(0, min(y0, y1)), min(H - 1, max(y0, y1))
    t = thickness
    out[y0:y0 + t, x0:x1 + 1] = color; out[max(y0, y1 - t + 1):y1 + 1, x0:x1 + 1] = color
    out[y0:y1 + 1, x0:x0 + t] = color; out[y0:y1 + 1, max(x0, x1 - t + 1):x1 + 1] = color
    return out


# ------------------------------------------------------------------------------------------------ main_visualize.py helpers
def get_discard_img(view_img, discard_indices, fea_size, patch_size, replace_color):
    """main_visualize.py:36-41: paint the patches of the discarded tokens."""
    res = np.copy(view_img)
    for d in discard_indices:
        h, w = int(d) // fea_size, int(d) % fea_size
        res[h * patch_size:(h + 1) * patch_size, w * patch_size:(w + 1) * patch_size] = replace_color
    return res


def find_high_activation_crop(activation_map, percentile=95):
    """main_visualize.py:44-66: bounding box (y0, y1, x0, x1) of the entries >= the given percentile."""
    mask = activation_map >= np.percentile(activation_map, percentile)
    rows, cols = np.nonzero(mask.any(axis=1))[0], np.nonzero(mask.any(axis=0))[0]
    if rows.size == 0:
        return 0, 1, 0, 1
    return int(rows[0]), int(rows[-1]) + 1, int(cols[0]), int(cols[-1]) + 1


def get_gaussian_params(proto_act):
    """main_visualize.py:69-84: weighted mean (2,) and covariance (2, 2) of the grid coordinates, weights rescaled to sum n^2
    (the same estimator as the PPC loss, protopformer.py:249-257)."""
    n = proto_act.shape[-1]
    pts = np.array([[x, y] for x in range(n) for y in range(n)], dtype=np.float64).T        # (2, n*n)
    w = proto_act.reshape(1, -1).astype(np.float64)
    w = w / w.sum(axis=-1) * (n * n)
    mean = np.mean(pts * w, axis=-1)
    cut = pts - mean[:, None]
    return mean, np.dot(cut * w, cut.T) / (n * n - 1)


def multivariate_gaussian(pos, mu, sigma):
    """main_visualize.py:87-98."""
    k = mu.shape[0]
    fac = np.einsum("...k,kl,...l->...", pos - mu, np.linalg.inv(sigma), pos - mu)
    return np.exp(-fac / 2) / np.sqrt((2 * np.pi) ** k * np.linalg.det(sigma))


def activation_overlay(view_img_bgr, proto_act, input_size):
    """main_visualize.py:381-391, 398: upsample one (g, g) activation map to the image, min-max normalise, JET heat map, 0.7 / 0.3
    blend; returns (overlay uint8 BGR, top-5 % box (y0, y1, x0, x1), arg-max grid cell)."""
    up = resize_cubic(proto_act, input_size)
    up = up - up.min()
    up = up / max(float(up.max()), 1e-12)
    heat = colormap_jet(np.uint8(255 * up))
    cell = tuple(int(t[0]) for t in np.where(proto_act == proto_act.max()))
    return (view_img_bgr * 0.7 + heat * 0.3).astype(np.uint8), find_high_activation_crop(up), cell


def visualize_category(ppnet, loader, view_images_bgr, out_dir, category_id, proto_per_category=10, input_size=224, patch_size=16,
                       use_gauss=False, max_images=None):
    """main_visualize.py:273-474 for one category: for every test image of the class and each of its prototypes, write the
    activation overlay, the top-5 % box image and the discarded-token mask (JPEG, via PIL).  `view_images_bgr`: uint8 (B, H, W, 3)
    un-normalised images aligned with `loader`'s order.  Returns the list of written files."""
    from PIL import Image
    out = collect_eval_outputs(ppnet, loader, category_id)
    k = ppnet.reserve_token_nums[-1]
    sel = np.nonzero(out["labels"] == category_id)[0]
    if max_images:
        sel = sel[:max_images]
    acts = torch.from_numpy(proto_acts_from_distances(out["distances"][sel], ppnet.epsilon))
    attn = torch.from_numpy(out["token_attn"][sel])
    grid = expand_to_grid(acts, attn, k).numpy()
    n_patches = attn.shape[-1]
    fea = int(round(n_patches ** 0.5))
    discard = torch.topk(attn, k=n_patches - k, dim=-1, largest=False)[1].numpy()
    cat_dir = os.path.join(out_dir, f"category_{category_id}")
    written = []
    for j, b in enumerate(sel):
        img_dir = os.path.join(cat_dir, f"img_{j}")
        os.makedirs(img_dir, exist_ok=True)
        img = view_images_bgr[b]
        path = os.path.join(img_dir, f"catch_img_reserve{k}_mask.jpg")
        Image.fromarray(get_discard_img(img, discard[j], fea, patch_size, [0, 0, 0])[:, :, ::-1]).save(path); written.append(path)
        for pi in range(proto_per_category):
            act = grid[j, category_id * proto_per_category + pi]
            over, (y0, y1, x0, x1), _ = activation_overlay(img, act, input_size)
            path = os.path.join(img_dir, f"proto{pi}_reserve{k}.jpg")
            Image.fromarray(over[:, :, ::-1]).save(path); written.append(path)
            path = os.path.join(img_dir, f"proto{pi}_reserve{k}_bnd.jpg")
            Image.fromarray(draw_rect(img, (x0, y0), (x1, y1), (0, 255, 255))[:, :, ::-1]).save(path); written.append(path)
            if use_gauss:
                mean, cov = get_gaussian_params(np.maximum(act, 0) + 1e-12)
                np.save(os.path.join(img_dir, f"gaussian_{pi}.npy"), np.concatenate([mean, cov.reshape(-1)]))
    return written


# ------------------------------------------------------------------------------------------------ eval_interpretability.py
class CubParts:
    """tools/local_parts.py: image paths, bounding boxes and the visible part locations of CUB-200-2011."""

    def __init__(self, data_root):
        def lines(*p):
            with open(os.path.join(data_root, *p)) as f:
                return [l.rstrip("\n") for l in f if l.strip()]
        self.id_to_path = {}
        for l in lines("images.txt"):
            i, p = l.split(" ", 1)
            self.id_to_path[int(i)] = tuple(p.split("/", 1))
        self.id_to_bbox = {}
        for l in lines("bounding_boxes.txt"):
            c = l.split(" ")
            x, y, w, h = (int(v.split(".")[0]) for v in c[1:5])
            self.id_to_bbox[int(c[0])] = (x, y, x + w, y + h)
        self.part_names = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in lines("parts", "parts.txt")}
        self.id_to_part_loc = {}
        for l in lines("parts", "part_locs.txt"):
            c = l.split(" ")
            i, pid, x, y, vis = int(c[0]), int(c[1]), int(float(c[2])), int(float(c[3])), int(c[4])
            self.id_to_part_loc.setdefault(i, [])
            if vis == 1:
                self.id_to_part_loc[i].append([pid, x, y])


def in_bbox(loc, bbox):
    return bbox[0] <= loc[0] <= bbox[1] and bbox[2] <= loc[1] <= bbox[3]


def prototype_part_table(acts_grid, part_labels, img_size, half_size=36, n_parts=15):
    """eval_interpretability.py:206-226 for one image: (n_proto, n_parts) 0/1 table -- does the 2*half_size box around the arg-max of
    the up-sampled activation contain the part?  part_labels: [(part_id0, x, y)] in resized-image pixels."""
    table = np.zeros((acts_grid.shape[0], n_parts))
    for pi in range(acts_grid.shape[0]):
        up = resize_cubic(acts_grid[pi], img_size)
        ys, xs = np.where(up == up.max())
        my, mx = int(ys[0]), int(xs[0])
        box = (max(0, my - half_size), min(img_size, my + half_size), max(0, mx - half_size), min(img_size, mx + half_size))
        for pid, x, y in part_labels:
            if in_bbox((y, x), box):
                table[pi, pid] = 1
    return table


def consistency_from_tables(tables, masks, part_thresh=0.8):
    """eval_interpretability.py:262-286 for one class: tables (n_img, n_proto, n_parts), masks (n_img, n_parts) of annotated parts.
    A prototype is consistent if some part falls inside its box in >= part_thresh of the images where that part is visible."""
    tables = np.transpose(np.asarray(tables), (1, 0, 2))
    masks = np.asarray(masks)
    denom = masks.sum(axis=0)
    denom = np.where(denom == 0, 1, denom)
    effect, max_part = [], []
    for t in tables:
        assert ((1.0 - masks) * t).sum() == 0
        frac = t.sum(axis=0) / denom
        effect.append(int((frac >= part_thresh).any()))
        max_part.append(float(frac.max()))
    return effect, max_part


def own_prototype_maps(ppnet, x, targets):
    """push_forward(x) with every image's maps narrowed to the prototypes of its own class: (attn (B, Np) rollout scores, own
    (B, ppc, s, s) activations of prototypes targets[b] * ppc ... + ppc - 1)."""
    ppc = ppnet.num_prototypes_per_class
    ta, pa = ppnet.push_forward(x)
    cols = (targets.to(pa.device) * ppc)[:, None] + torch.arange(ppc, device=pa.device)[None, :]
    return ta, torch.gather(pa, 1, cols[:, :, None, None].expand(-1, -1, pa.shape[-2], pa.shape[-1]))


@torch.no_grad()
def consistency_score(ppnet, loader, parts, image_sizes, num_classes=200, part_thresh=0.8, half_size=36, n_parts=15, device=False):
    """eval_interpretability.py:136-290: push_forward over the test set, the class's own prototypes expanded to the patch grid, the
    part table per image, and the fraction of prototypes that are part-consistent.  loader yields (x, targets, img_ids);
    image_sizes: {img_id: (width, height)} of the original files (the reference reads them with cv2.imread).
    device=True: the part tables are made on the GPU, one peak + table launch per batch (see consistency_from_outputs); only the
    (B, ppc, n_parts) uint8 tables come back.  Same score; the default (host) path is the referee."""
    ppnet.eval()
    ppc, k, img_size = ppnet.num_prototypes_per_class, ppnet.reserve_token_nums[0], ppnet.img_size
    attn, acts, targets, ids, tables, masks = [], [], [], [], [], []
    for x, t, i in loader:
        t = torch.as_tensor(t)
        ta, own = own_prototype_maps(ppnet, x.cuda() if not x.is_cuda else x, t)
        targets.append(t.cpu()); ids.append(torch.as_tensor(i).cpu())
        if device:
            tb, mk = _device_tables(_grid_on_device(ta, own, k), ids[-1].numpy(), parts, image_sizes, img_size, half_size, n_parts)
            tables.append(tb); masks.append(mk)
        else:
            acts.append(own.cpu()); attn.append(ta.cpu())
    if device:
        tables = torch.cat(tables).cpu().numpy() if tables else np.zeros((0, ppc, n_parts), dtype=np.uint8)
        return _score_from_tables(tables, np.concatenate(masks) if masks else np.zeros((0, n_parts)), torch.cat(targets).numpy(), num_classes,
                                  part_thresh)[0]
    return consistency_from_outputs(torch.cat(attn), torch.cat(acts), torch.cat(targets).numpy(), torch.cat(ids).numpy(), parts, image_sizes, k,
                                    img_size, num_classes, part_thresh, half_size, n_parts)[0]


def consistency_from_outputs(attn, acts, targets, ids, parts, image_sizes, k, img_size, num_classes=200, part_thresh=0.8, half_size=36, n_parts=15,
                             device=False):
    """eval_interpretability.py:152-290 on collected push_forward outputs: attn (B, Np) rollout scores, acts (B, ppc, s, s) the class's
    own prototype activations on the k = s*s reserved tokens, targets / ids (B,).  Returns (score, effect per (class, prototype),
    best part fraction per (class, prototype), activations on the patch grid).  Classes without a test image are skipped (the
    reference's loop assumes every class has one).
    device=True: attn / acts go to (or stay on) the GPU, expand_to_grid runs there, one ppf_act_peak launch makes every part table, and
    only the (B, ppc, n_parts) uint8 tables are read back; the grid is returned as a CUDA tensor.  Same score, effects and fractions."""
    targets, ids = np.asarray(targets), np.asarray(ids)
    if device:
        grid = _grid_on_device(torch.as_tensor(attn).cuda(), torch.as_tensor(acts).cuda(), k)
        tables, masks = _device_tables(grid, ids, parts, image_sizes, img_size, half_size, n_parts)
        tables = tables.cpu().numpy()
    else:
        grid = _host_grid(attn, acts, k)
        tables, masks = _host_tables(grid, ids, parts, image_sizes, img_size, half_size, n_parts)
    return _score_from_tables(tables, masks, targets, num_classes, part_thresh) + (grid,)


# ------------------------------------------------------------------------------------------------ the same post-processing on the device
def _maps3(grids):
    """(..., g, g) CUDA maps as the (M, g, g) view the kernels take, and the leading shape; layout and dtype are the kernels' to refuse."""
    if not isinstance(grids, torch.Tensor) or grids.dim() < 2:
        return grids, ()
    lead = tuple(grids.shape[:-2])
    if grids.dim() == 3 or not grids.is_contiguous():
        return grids, lead
    return grids.reshape((int(np.prod(lead, dtype=np.int64)),) + tuple(grids.shape[-2:])), lead


def upsample_cubic_device(grids, size):
    """resize_cubic of every map of a contiguous fp32 CUDA tensor (..., g, g) -> (..., size, size), bit-identical to the host function
    (ppf_act_upsample)."""
    from . import ops
    maps, lead = _maps3(grids)
    return ops.act_upsample(maps, size).reshape(lead + (size, size))


def activation_peaks(grids, size):
    """Maximum and first arg-max in row-major order of every up-sampled map, without materialising it (ppf_act_peak): (values (...)
    fp32, yx (..., 2) int32 as (y, x)) = up.max() and np.where(up == up.max())[..][0] of up = resize_cubic(map, size)."""
    from . import ops
    maps, lead = _maps3(grids)
    val, yx, _ = ops.act_peak(maps, size)
    return val.reshape(lead), yx.reshape(lead + (2,))


def percentile_ranks(n, percentile):
    """The two 0-based ascending ranks np.percentile(a, percentile) (linear) of n values interpolates between, and the fraction of the
    way from the first to the second: numpy's virtual index (n - 1) * q, in the form its implementation evaluates it."""
    if not 0 <= percentile <= 100:
        raise ValueError(f"percentile {percentile} outside [0, 100]")
    q = percentile / 100.0
    v = n * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0
    lo = min(max(int(np.floor(v)), 0), n - 1)
    return lo, min(lo + 1, n - 1), min(max(v - lo, 0.0), 1.0)


def high_activation_boxes(grids, size, percentile=95):
    """find_high_activation_crop(resize_cubic(map, size), percentile) of every map: (..., 4) int32 (y0, y1, x0, x1) on the device.
    ppf_act_order_stats selects the two order statistics around the percentile exactly; the threshold between them is numpy's own
    interpolation (np.percentile of the pair at the matching fraction, on the host: one (M, 2) read-back); ppf_act_box takes it."""
    from . import ops
    maps, lead = _maps3(grids)
    lo, hi, frac = percentile_ranks(int(size) * int(size), percentile) if int(size) >= 1 else (0, 0, 0.0)
    stats = ops.act_order_stats(maps, size, lo, hi).cpu().numpy()
    thr = np.percentile(stats, frac * 100.0, axis=1) if stats.shape[0] else np.zeros(0)
    thr = torch.from_numpy(np.ascontiguousarray(thr, dtype=np.float64)).to(maps.device)
    return ops.act_box(maps, size, thr).reshape(lead + (4,))


def patch_grid(attn, acts, k):
    """The (B, ppc, g, g) fp32 maps on the patch grid: expand_to_grid, unless the k tokens already are the grid.  Torch: it runs where
    its inputs are."""
    attn, acts = attn.float(), acts.float()
    return expand_to_grid(acts, attn, k) if k != attn.reshape(attn.shape[0], -1).shape[-1] else acts


def _grid_on_device(attn, acts, k):
    return patch_grid(attn, acts, k).contiguous()


def _host_grid(attn, acts, k):
    return patch_grid(torch.as_tensor(attn).cpu(), torch.as_tensor(acts).cpu(), k).numpy()


def scaled_parts(ids, parts, image_sizes, img_size, n_parts):
    """The part annotations of a batch in resized-image pixels (eval_interpretability.py:192-200): (labels: per image the list of
    (part_id0, x, y) in annotation order, as prototype_part_table takes it; masks (B, n_parts) of annotated parts).  The host referee
    and the device path both take their pixels from here, so that they score the same boxes."""
    labels, masks = [], np.zeros((len(ids), n_parts))
    for j, i in enumerate(ids):
        w, h = image_sizes[int(i)]
        labels.append([(pid - 1, int(img_size * (x / w)), int(img_size * (y / h))) for pid, x, y in parts.id_to_part_loc.get(int(i), [])])
        masks[j, [pid0 for pid0, _, _ in labels[-1]]] = 1
    return labels, masks


def _part_list(ids, parts, image_sizes, img_size, n_parts):
    """scaled_parts as the kernels take it: (plist (B, n_parts, 3) int32 (valid, x, y) by part id, masks).  Host arrays, built once per
    batch."""
    labels, masks = scaled_parts(ids, parts, image_sizes, img_size, n_parts)
    plist = np.zeros((len(labels), n_parts, 3), dtype=np.int32)
    for j, image in enumerate(labels):
        for pid0, x, y in image:
            if plist[j, pid0, 0]:
                raise ValueError(f"image {int(ids[j])} lists part {pid0 + 1} twice: the device path takes one location per part")
            plist[j, pid0] = (1, x, y)
    return plist, masks


def _tables_for_parts(grid, plist_dev, img_size, half_size):
    """grid (B, ppc, g, g) CUDA and the uploaded part list (B, n_parts, 3) -> tables (B, ppc, n_parts) uint8 CUDA: one ppf_act_peak launch."""
    from . import ops
    B, ppc = grid.shape[:2]
    if B == 0:
        return torch.zeros((0, ppc, plist_dev.shape[1]), dtype=torch.uint8, device=grid.device)
    _, _, table = ops.act_peak(grid.reshape(B * ppc, grid.shape[-2], grid.shape[-1]), img_size, plist_dev, half_size)
    return table.reshape(B, ppc, plist_dev.shape[1])


def _device_tables(grid, ids, parts, image_sizes, img_size, half_size, n_parts):
    """Part tables of a batch: grid (B, ppc, g, g) CUDA -> (tables (B, ppc, n_parts) uint8 CUDA, masks (B, n_parts) numpy)."""
    plist, masks = _part_list(ids, parts, image_sizes, img_size, n_parts)
    return _tables_for_parts(grid, torch.from_numpy(plist).to(grid.device), img_size, half_size), masks


def _score_from_tables(tables, masks, targets, num_classes, part_thresh):
    """(score, effects, best fractions) from per-image tables (B, ppc, n_parts) and masks (B, n_parts), class by class in the host
    path's order."""
    effects, max_parts = [], []
    for c in range(num_classes):
        sel = np.nonzero(targets == c)[0]
        if sel.size == 0:
            continue
        e, m = consistency_from_tables(tables[sel].astype(np.float64), masks[sel], part_thresh)
        effects.extend(e); max_parts.extend(m)
    return (float(np.mean(effects)) if effects else 0.0), effects, max_parts


# ------------------------------------------------------------------------------------------------ stability score
# Huang et al., ICCV 2023 ("Evaluation and Improvement of Interpretability for Self-Explainable Part-Prototype Networks") report the
# consistency score next to a stability score: prototype j of class c is stable on a test image x of class c when its row of the part
# table is the same for x and for x + N(0, sigma^2) noise on the normalised input; stable_j is the fraction of the class's images where
# it is, the score the mean of stable_j over the (class, prototype) pairs of the classes that have an image.  The reference has no
# such pass.
def add_input_noise(x, image_ids, std=0.2, seed=0):
    """Noisy copy of an fp32 CUDA batch [B, ...]: x + std * N(0, 1) (ppf_add_gauss_noise).  The noise of an image depends on (seed, its
    id, element) only, so a data set gets the same perturbation at every batch size and in every order."""
    from . import ops
    ids = torch.as_tensor(image_ids).to(device=x.device, dtype=torch.int64).contiguous()
    return ops.add_gauss_noise(x, ids, std, seed)


def part_meter_scores(hits, visible, stable, images, part_thresh=0.8, with_stability=True):
    """The scores from per-class counts (numpy integers): hits (C, ppc, n_parts) = images where the part lies in the prototype's box,
    visible (C, n_parts) = images where the part is annotated, stable (C, ppc) = images where the prototype's row survived the noise,
    images (C,).  consistency / effects / max_parts as consistency_from_tables computes them (fp64 hits / max(visible, 1),
    >= part_thresh), classes without an image skipped, in class order; stable_fraction = stable / images per (class, prototype) and
    stability its mean (both None without with_stability)."""
    hits, visible, stable, images = (np.asarray(a) for a in (hits, visible, stable, images))
    effects, max_parts, fraction = [], [], []
    for c in np.nonzero(images > 0)[0]:
        denom = visible[c].astype(np.float64)
        denom = np.where(denom == 0, 1, denom)
        for p in range(hits.shape[1]):
            frac = hits[c, p].astype(np.float64) / denom
            effects.append(int((frac >= part_thresh).any()))
            max_parts.append(float(frac.max()))
            fraction.append(float(stable[c, p] / images[c]))
    out = dict(consistency=float(np.mean(effects)) if effects else 0.0, effects=effects, max_parts=max_parts, stability=None, stable_fraction=None,
               images=[int(v) for v in images])
    if with_stability:
        out.update(stability=float(np.mean(fraction)) if fraction else 0.0, stable_fraction=fraction)
    return out


class PartMeter:
    """Per-class accumulators of the consistency and the stability score in device memory (ppf_part_meter_update): update() only
    launches, result() is the one read-back.  Integer counts: the result does not depend on how the images were batched or ordered.
    `device` may be 'cpu' to hold counts made elsewhere (result() works there, update() needs the GPU)."""

    def __init__(self, num_classes, ppc, n_parts, device):
        C, self.ppc, self.n_parts = int(num_classes), int(ppc), int(n_parts)
        self.sizes = (C * self.ppc * self.n_parts, C * self.n_parts, C * self.ppc, C, 1)
        self.buf = torch.zeros(sum(self.sizes), dtype=torch.int32, device=device)          # one buffer: one read-back
        hits, visible, stable, images, self.bad = torch.split(self.buf, self.sizes)
        self.hits, self.visible, self.stable, self.images = hits.view(C, self.ppc, self.n_parts), visible.view(C, self.n_parts), stable.view(C, self.ppc), images
        self.noisy = None                  # whether the updates carry a noisy table; None before the first one

    def reset(self):
        self.buf.zero_()
        self.noisy = None

    def update(self, tables, parts_dev, labels, tables_noisy=None):
        """tables / tables_noisy (B, ppc, n_parts) uint8 as ppf_act_peak writes them, parts_dev (B, n_parts, 3) int32, labels (B,) int64,
        all on the meter's device.  Either every update carries a noisy table or none does."""
        from . import ops
        if self.noisy is not None and self.noisy != (tables_noisy is not None):
            raise ValueError("PartMeter.update: a noisy table must come with every update or with none (stable and images would not match)")
        ops.part_meter_update(tables, tables_noisy, parts_dev, labels, self.hits, self.visible, self.stable, self.images, self.bad)
        self.noisy = tables_noisy is not None

    def result(self, part_thresh=0.8):
        """dict(consistency, effects, max_parts, stability, stable_fraction, images) of part_meter_scores; stability is None if no noisy
        table was ever passed.  Raises if a label lay outside [0, num_classes)."""
        host = self.buf.cpu().numpy()
        hits, visible, stable, images, bad = np.split(host, np.cumsum(self.sizes)[:-1])
        C = self.sizes[3]
        if int(bad[0]) != 0:
            raise ValueError(f"PartMeter: {int(bad[0])} labels lie outside [0, {C}) (of {int(images.sum()) + int(bad[0])} images)")
        return part_meter_scores(hits.reshape(C, self.ppc, self.n_parts), visible.reshape(C, self.n_parts), stable.reshape(C, self.ppc), images,
                                 part_thresh, bool(self.noisy))


def _host_tables(grid, ids, parts, image_sizes, img_size, half_size, n_parts):
    """prototype_part_table of every image of a host grid (B, P, g, g): (tables (B, P, n_parts) of 0 / 1, masks (B, n_parts))."""
    labels, masks = scaled_parts(ids, parts, image_sizes, img_size, n_parts)
    tables = np.zeros((grid.shape[0], grid.shape[1], n_parts))
    for j, image in enumerate(labels):
        tables[j] = prototype_part_table(grid[j], image, img_size, half_size, n_parts)
    return tables, masks


def stability_from_tables(tables, tables_noisy, targets, num_classes):
    """(score, stable fraction per (class, prototype)) from per-image part tables (B, ppc, n_parts) of the clean and the noisy pass:
    rows compared over all parts, averaged over the images of a class; classes without an image are skipped, in class order."""
    same = (np.asarray(tables) == np.asarray(tables_noisy)).all(axis=2)                      # (B, ppc)
    fraction = []
    for c in range(num_classes):
        sel = np.nonzero(np.asarray(targets) == c)[0]
        if sel.size == 0:
            continue
        fraction.extend(float(n / sel.size) for n in same[sel].sum(axis=0))
    return (float(np.mean(fraction)) if fraction else 0.0), fraction


def stability_from_outputs(attn, acts, attn_noisy, acts_noisy, targets, ids, parts, image_sizes, k, img_size, num_classes=200, half_size=36, n_parts=15,
                           device=False):
    """The stability score on collected push_forward outputs of a clean and a noisy pass over the same images: attn / attn_noisy
    (B, Np) rollout scores (each pass is expanded to the patch grid by its own), acts / acts_noisy (B, ppc, s, s) the class's own
    prototype activations, targets / ids (B,).  Returns (score, stable fraction per (class, prototype)).  The host path
    (prototype_part_table and row equality in numpy) is the referee; device=True makes both sets of tables with ppf_act_peak from one
    uploaded part list and reduces them in a PartMeter.  Same values."""
    targets, ids = np.asarray(targets), np.asarray(ids)
    if device:
        attn, acts, attn_noisy, acts_noisy = (torch.as_tensor(a).cuda() for a in (attn, acts, attn_noisy, acts_noisy))
        plist = torch.from_numpy(_part_list(ids, parts, image_sizes, img_size, n_parts)[0]).to(acts.device)
        meter = PartMeter(num_classes, acts.shape[1], n_parts, acts.device)
        meter.update(_tables_for_parts(_grid_on_device(attn, acts, k), plist, img_size, half_size), plist,
                     torch.from_numpy(targets.astype(np.int64)).to(acts.device),
                     _tables_for_parts(_grid_on_device(attn_noisy, acts_noisy, k), plist, img_size, half_size))
        r = meter.result()
        return r["stability"], r["stable_fraction"]
    clean = _host_tables(_host_grid(attn, acts, k), ids, parts, image_sizes, img_size, half_size, n_parts)[0]
    noisy = _host_tables(_host_grid(attn_noisy, acts_noisy, k), ids, parts, image_sizes, img_size, half_size, n_parts)[0]
    return stability_from_tables(clean, noisy, targets, num_classes)


@torch.no_grad()
def interpretability_scores(ppnet, loader, parts, image_sizes, num_classes=200, part_thresh=0.8, half_size=36, n_parts=15, noise_std=0.2, seed=0,
                            stability=True, device=True):
    """Consistency and stability score of a model over a test set in one pass: dict(consistency, stability, effects, max_parts,
    stable_fraction); stability / stable_fraction are None with stability=False.  loader yields (x, targets, img_ids) (img_ids on the
    host); image_sizes: {img_id: (width, height)} of the original files.
    device=True: per batch push_forward(x), push_forward(add_input_noise(x, ids, noise_std, seed)), the gather of the class's own
    prototypes, two ppf_act_peak launches that share one uploaded part list and one PartMeter update; nothing is read back before the
    single read of the meter at the end.  device=False: the outputs of both passes are collected and scored by the host referees
    (consistency_from_tables, stability_from_tables on prototype_part_table's tables); the noise still comes from the kernel, the one
    source there is."""
    ppnet.eval()
    ppc, k, img_size = ppnet.num_prototypes_per_class, ppnet.reserve_token_nums[0], ppnet.img_size
    meter, kept = None, []

    for x, t, i in loader:
        x = x.cuda() if not x.is_cuda else x
        ids = torch.as_tensor(i).cpu()
        t = torch.as_tensor(t).to(device=x.device, dtype=torch.int64)
        passes = [own_prototype_maps(ppnet, x, t)]
        if stability:
            passes.append(own_prototype_maps(ppnet, add_input_noise(x, ids, noise_std, seed), t))
        if device:
            if meter is None:
                meter = PartMeter(num_classes, ppc, n_parts, x.device)
            plist = torch.from_numpy(_part_list(ids.numpy(), parts, image_sizes, img_size, n_parts)[0]).to(x.device, non_blocking=True)
            tables = [_tables_for_parts(_grid_on_device(ta, own, k), plist, img_size, half_size) for ta, own in passes]
            meter.update(tables[0], plist, t.contiguous(), tables[1] if stability else None)
        else:
            kept.append((ids, t.cpu(), [(ta.float().cpu(), own.float().cpu()) for ta, own in passes]))
    if device:
        r = meter.result(part_thresh) if meter is not None else part_meter_scores(np.zeros((0, ppc, n_parts)), np.zeros((0, n_parts)), np.zeros((0, ppc)),
                                                                                   np.zeros(0), part_thresh, stability)
        r.pop("images")
        return r
    ids = torch.cat([c[0] for c in kept]).numpy() if kept else np.zeros(0, dtype=np.int64)
    targets = torch.cat([c[1] for c in kept]).numpy() if kept else np.zeros(0, dtype=np.int64)
    tables = []
    for j in range(2 if stability else 1):
        if not kept:
            tables.append(np.zeros((0, ppc, n_parts)))
            continue
        grid = _host_grid(torch.cat([c[2][j][0] for c in kept]), torch.cat([c[2][j][1] for c in kept]), k)
        tables.append(_host_tables(grid, ids, parts, image_sizes, img_size, half_size, n_parts))
    score, effects, max_parts = _score_from_tables(tables[0][0], tables[0][1], targets, num_classes, part_thresh)
    out = dict(consistency=score, effects=effects, max_parts=max_parts, stability=None, stable_fraction=None)
    if stability:
        out["stability"], out["stable_fraction"] = stability_from_tables(tables[0][0], tables[1][0], targets, num_classes)
    return out


# ------------------------------------------------------------------------------------------------ dataset-wide nearest patches
def patch_box(grid_pos, side, patch_size):
    """Pixel rectangle (x0, y0, x1, y1), end-exclusive, of cell `grid_pos` (row-major) of the side x side patch grid."""
    if not 0 <= int(grid_pos) < side * side:
        raise ValueError(f"patch_box: grid position {grid_pos} outside the {side} x {side} grid")
    row, col = int(grid_pos) // side, int(grid_pos) % side
    return col * patch_size, row * patch_size, (col + 1) * patch_size, (row + 1) * patch_size


def nearest_patches(ppnet, loader, topk=10, class_specific=True):
    """Rank the whole of `loader` per prototype: returns the filled bank.PrototypeBank (its result() holds, per prototype, the topk
    activations, image ids and grid cells; project_() pushes the prototypes onto their best patches).  loader yields (x, labels) or
    (x, labels, ids) (Cub2011(return_id=True)); without ids an image's id is its running index in loader order, so the loader must
    not shuffle.  Ids must be unique over the loader."""
    from .bank import PrototypeBank
    bank = PrototypeBank(ppnet, topk=topk, class_specific=class_specific)
    for x, y, ids in batches_with_ids(loader):
        bank.update(x.cuda() if not x.is_cuda else x, y, ids)
    return bank


# ------------------------------------------------------------------------------------------------ local analysis: explain a prediction
# ProtoPNet's "local analysis", the counterpart of the bank's global one: for one image and one class, which prototypes carry the
# logit, where on the image each of them fired, and (with a bank) which training patches each of them stands for.  Everything comes from
# what an eval forward leaves on the device (ppf_explain_topk, one launch per branch); the reference has no such pass.
EXPLAIN_BRANCHES = ("local", "global")
EXPLAIN_FIELDS = ("classes", "class_logits", "prototypes", "contributions", "activations", "cells", "evidence", "weights", "maps", "boxes")


def _host(t, dtype):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


def explain_from_outputs(act_max, weight, scale, ppc, logits, topk, classes=None, top_classes=1, sign=1, argmax=None, idx=None, act_full=None,
                         grid_cells=0, maps=False, device=True):
    """The K = topk strongest class evidences per (sample, class) of ONE branch from collected outputs: act_max [B, P] pooled
    activations, weight [C, P] the branch's last layer, scale its share of the logit, logits [B, C]; the local branch adds argmax [B, P],
    idx [B, T] and act_full [B, P, T] (with maps: maps on a grid of `grid_cells` cells).  classes int32 [B, M], or None: the top
    `top_classes` of logits.  Returns dict(classes, class_logits [B, M], prototypes, contributions, activations, cells [B, M, K], evidence
    [B, M, 2], maps [B, M, K, grid_cells] or None); the contract is ppf_explain_topk's (include/ppf_hip.h).
    device=True: one ppf_explain_topk launch on CUDA tensors (device tensors out).  device=False: the numpy referee (host arrays out) --
    the same two fp32 products, np.lexsort on (prototype id, -sign * contribution) over the finite contributions, an fp64 evidence sum."""
    if device:
        from . import ops
        return ops.explain_topk(act_max, weight, scale, ppc, logits, topk, classes=classes, top_classes=top_classes, sign=sign, argmax=argmax, idx=idx,
                                act_full=act_full, grid_cells=grid_cells, want_maps=maps)
    act_max, weight, logits = _host(act_max, np.float32), _host(weight, np.float32), _host(logits, np.float32)
    argmax, idx, act_full = _host(argmax, np.int64), _host(idx, np.int64), _host(act_full, np.float32)
    (B, P), C, K, G = act_max.shape, weight.shape[0], int(topk), int(grid_cells)
    if sign not in (1, -1) or not 1 <= K <= 64 or ppc < 1 or P % ppc:
        raise ValueError(f"explain_from_outputs: sign={sign} topk={K} ppc={ppc} P={P} outside ppf_explain_topk's limits")
    if classes is None:
        M = int(top_classes)
        cls = np.full((B, M), -1, dtype=np.int32)
        for b in range(B):
            ids = np.nonzero(~np.isnan(logits[b]))[0]
            order = ids[np.lexsort((ids, -logits[b, ids]))][:M]
            cls[b, :order.size] = order
    else:
        cls = _host(classes, np.int32).reshape(B, -1).copy()
        cls[(cls < 0) | (cls >= C)] = -1
        M = cls.shape[1]
    if not 1 <= M <= min(8, C):
        raise ValueError(f"explain_from_outputs: M={M} classes per sample outside [1, min(8, C={C})]")
    T = idx.shape[1] if idx is not None else 0
    if act_full is not None:
        act_full = act_full.reshape(B, P, T)
    out = dict(classes=cls, class_logits=np.full((B, M), -np.inf, dtype=np.float32), prototypes=np.full((B, M, K), -1, dtype=np.int32),
               contributions=np.full((B, M, K), -np.inf, dtype=np.float32), activations=np.full((B, M, K), -np.inf, dtype=np.float32),
               cells=np.full((B, M, K), -1, dtype=np.int32), evidence=np.zeros((B, M, 2), dtype=np.float32),
               maps=np.zeros((B, M, K, G), dtype=np.float32) if maps else None)
    with np.errstate(all="ignore"):
        w = np.float32(scale) * weight                                               # fp32: the first rounding
        proto_class = np.arange(P) // ppc
        for b in range(B):
            for m in range(M):
                c = int(cls[b, m])
                if c < 0:
                    continue
                out["class_logits"][b, m] = logits[b, c]
                ctr = act_max[b] * w[c]                                              # fp32: the second rounding
                own = proto_class == c
                out["evidence"][b, m] = (ctr[own].astype(np.float64).sum(), ctr[~own].astype(np.float64).sum())
                ids = np.nonzero(np.isfinite(ctr))[0]
                order = ids[np.lexsort((ids, -(np.float32(sign) * ctr[ids])))][:K]
                n = order.size
                out["prototypes"][b, m, :n], out["contributions"][b, m, :n], out["activations"][b, m, :n] = order, ctr[order], act_max[b, order]
                if argmax is None:
                    continue
                t = argmax[b, order]
                ok = (t >= 0) & (t < T)
                out["cells"][b, m, :n] = np.where(ok, idx[b, np.clip(t, 0, T - 1)], -1)
                if maps:
                    on_grid = (idx[b] >= 0) & (idx[b] < G)
                    for k in range(n):
                        out["maps"][b, m, k, idx[b][on_grid]] = act_full[b, order[k]][on_grid]
    return out


class Explanation(Record):
    """What explain() returns: per branch ('local' / 'global') the fields of EXPLAIN_FIELDS, as device tensors (or numpy arrays after
    cpu()).  classes / class_logits [B, M]: the explained classes and the model's logits for them; prototypes / contributions /
    activations / cells / weights [B, M, K]: the ranked prototypes (-1 / -inf in unfilled slots), their share of the logit, pooled
    activation, grid cell (local branch; -1 on the global one) and raw last-layer weight; evidence [B, M, 2]: the branch's share of the
    logit from the class's own prototypes and from all others; maps [B, M, K, side, side] and boxes [B, M, K, 4] (y0, y1, x0, x1): local
    branch with maps=True, else None.  ex.local / ex.global_ are the two field sets; a field name on the object itself is the local one.
    meta: ppc and scale per branch, side (cells per grid side), patch_size, img_size, against."""

    FIELDS = ("local", "global_")                           # each a dict of the EXPLAIN_FIELDS
    META = dict(ppc=dict, scale=lambda s: {k: float(v) for k, v in s.items()}, side=int, patch_size=int, img_size=int, against=bool)
    DEFAULTS = dict(against=False)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        for br in (self.local, self.global_):
            for k in EXPLAIN_FIELDS:
                br.setdefault(k, None)

    branches = property(lambda self: {"local": self.local, "global": self.global_})

    def __getattr__(self, name):
        if name in EXPLAIN_FIELDS:
            return self.__dict__["local"][name]
        raise AttributeError(name)

    def report(self, index=None, bank=None, stats=None):
        """JSON-able records, one per image (index: None = every image of the batch, or one batch position, or a sequence of them):
        {'image': b, 'against', 'classes': [{'class', 'logit', 'local': branch, 'global': branch}]} with branch = {'scale', 'evidence_own',
        'evidence_other', 'prototypes': [{'rank', 'prototype', 'prototype_class', 'weight', 'activation', 'contribution'; on the local
        branch also 'cell', 'patch_box' [x0, y0, x1, y1] and (with maps) 'activation_box' [y0, y1, x0, x1]; with `bank` (the arrays of
        prototype_bank.npz) 'nearest': that prototype's ranked training patches [{'rank', 'image_id', 'activation', 'grid_pos'}]; with
        `stats` (protostats.PrototypeStats.result() or load_stats of prototype_stats.npz) 'percentile_all' and 'percentile_own': where the
        activation stands among all / the own-class images the statistics recorded (protostats.percentile)}]}.
        Unfilled slots and classes that could not be explained (class -1) are dropped."""
        h = self.cpu()
        B = h.branches["local"]["classes"].shape[0]
        rows = range(B) if index is None else ([int(index)] if np.ndim(index) == 0 else [int(i) for i in index])
        records = []
        for b in rows:
            if not 0 <= b < B:
                raise IndexError(f"Explanation.report: image {b} outside the batch of {B}")
            classes = []
            for m in range(h.branches["local"]["classes"].shape[1]):
                c = int(h.branches["local"]["classes"][b, m])
                if c < 0:
                    continue
                entry = {"class": c, "logit": float(h.branches["local"]["class_logits"][b, m])}
                for br in EXPLAIN_BRANCHES:
                    entry[br] = h._branch_record(br, b, m, bank, stats)
                classes.append(entry)
            records.append({"image": b, "against": h.against, "classes": classes})
        return records

    def _branch_record(self, br, b, m, bank, stats=None):
        f = self.branches[br]
        protos = []
        for k in range(f["prototypes"].shape[2]):
            p = int(f["prototypes"][b, m, k])
            if p < 0:
                continue
            e = dict(rank=len(protos), prototype=p, prototype_class=p // self.ppc[br], weight=float(f["weights"][b, m, k]) if f["weights"] is not None else None,
                     activation=float(f["activations"][b, m, k]), contribution=float(f["contributions"][b, m, k]))
            if br == "local":
                cell = int(f["cells"][b, m, k])
                e["cell"] = cell if cell >= 0 else None
                e["patch_box"] = list(patch_box(cell, self.side, self.patch_size)) if cell >= 0 else None
                if f["boxes"] is not None:
                    e["activation_box"] = [int(v) for v in f["boxes"][b, m, k]]
            if bank is not None:
                n = int(bank[f"{br}_filled"][p])
                e["nearest"] = [dict(rank=r, image_id=int(bank[f"{br}_image_ids"][p, r]), activation=float(bank[f"{br}_values"][p, r]),
                                     grid_pos=int(bank[f"{br}_grid_pos"][p, r])) for r in range(n)]
            if stats is not None:
                from .protostats import percentile
                e["percentile_all"] = percentile(stats[br], p, e["activation"], "all")
                e["percentile_own"] = percentile(stats[br], p, e["activation"], "own")
            protos.append(e)
        return dict(scale=self.scale[br], evidence_own=float(f["evidence"][b, m, 0]), evidence_other=float(f["evidence"][b, m, 1]), prototypes=protos)


def _explain_classes(classes, B, C, device):
    """classes of explain() as the int32 [B, M] device tensor the kernel takes.  Host lists / arrays are range-checked here; a device
    tensor is not read back (the kernel answers a class outside [0, C) with an unfilled row)."""
    if isinstance(classes, torch.Tensor) and classes.is_cuda:
        if classes.is_floating_point():
            raise ValueError(f"explain: classes must be integers, got {classes.dtype}")
        t = classes
    else:
        a = np.asarray(classes.cpu() if isinstance(classes, torch.Tensor) else classes)
        if a.dtype.kind not in "iu":
            raise ValueError(f"explain: classes must be integers, got {a.dtype}")
        if a.size and (a.min() < 0 or a.max() >= C):
            raise ValueError(f"explain: classes must lie in [0, {C}), got {int(a.min())} .. {int(a.max())}")
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2 or t.shape[0] != B:
        raise ValueError(f"explain: classes must be [B] or [B, M] for a batch of {B}, got {tuple(t.shape)}")
    return t.to(torch.int32).contiguous()


@torch.no_grad()
def explain(ppnet, x, classes=None, top_classes=1, topk=10, against=False, maps=True):
    """Why did these images get these classes?  One eval pass of `ppnet` over the batch x, then one ppf_explain_topk launch per branch:
    the local branch picks the classes (classes=None: the top `top_classes` of the logits; else a [B] or [B, M] integer tensor or list)
    and the global branch explains the same ones.  topk prototypes per (image, class), by their share of the logit
    act * (branch share * last-layer weight); against=True ranks the strongest evidence AGAINST the class instead.  maps=True also
    returns the selected prototypes' activation maps on the patch grid and their high-activation pixel boxes (high_activation_boxes).
    Returns an Explanation (device tensors; nothing is read back here except the two order statistics per map the boxes need)."""
    from . import ops
    if not x.is_cuda:
        raise RuntimeError("explain needs a CUDA/HIP batch (no CPU fallback path; explain_from_outputs(device=False) is the host referee)")
    B, C = x.shape[0], ppnet.last_layer.weight.shape[0]
    cls = None if classes is None else _explain_classes(classes, B, C, x.device)
    r = ppnet.eval_branches(x)
    coe, sign = float(ppnet.global_coe), -1 if against else 1
    G = int(ppnet.num_patches)
    side = int(round(G ** 0.5))
    w_l, w_g = ppnet.last_layer.weight.detach().contiguous(), ppnet.last_layer_global.weight.detach().contiguous()
    logits = r.logits.contiguous()
    local = ops.explain_topk(r.act_max_local, w_l, 1.0 - coe, ppnet.num_prototypes_per_class, logits, topk, classes=cls, top_classes=top_classes,
                             sign=sign, argmax=r.argmax, idx=r.idx.contiguous(), act_full=r.act_full.contiguous(), grid_cells=G, want_maps=maps)
    glob = ops.explain_topk(r.act_max_global, w_g, coe, ppnet.global_proto_per_class, logits, topk, classes=local["classes"], sign=sign)
    for f, w in ((local, w_l), (glob, w_g)):
        f["weights"] = w[f["classes"].clamp(min=0).long()[:, :, None], f["prototypes"].clamp(min=0).long()]       # raw weights of the listed pairs
    if maps:
        local["maps"] = local["maps"].reshape(local["maps"].shape[:3] + (side, side))
        local["boxes"] = high_activation_boxes(local["maps"], ppnet.img_size)
    return Explanation(local, glob, {"local": ppnet.num_prototypes_per_class, "global": ppnet.global_proto_per_class},
                       {"local": 1.0 - coe, "global": coe}, side, ppnet.img_size // side, ppnet.img_size, against)


# ------------------------------------------------------------------------------------------------ faithfulness: is the explanation true?
# The deletion / insertion test (Petsiuk et al., RISE, 2018) on the patch grid: rank the cells of an image by their evidence for a class,
# remove them most important first (deletion) or show only them (insertion), and follow the class probability.  An explanation is
# informative when its deletion curve falls faster, and its insertion curve rises faster, than under a random order of the cells.
# Everything stays on the device: ppf_cell_order ranks, ppf_patch_perturb builds the images, the model's own forward scores them and
# ppf_class_prob reads the one probability per image (csrc/faithful.hip).  The reference has no such pass; the numpy forms below
# (device=False) are the referees.
ORDER_MODES = ("evidence", "attention", "random")
EXTRA_ORDERS = ("rise",)                # opt-in orders of faithfulness_curves / faithfulness: the black-box baseline (rise_saliency, below)
GAME_ORDERS = ("shap",)                 # opt-in order: the cells ranked by their Shapley values (kernel_shap, below); cell resolution only
CURVE_MODES = ("deletion", "insertion")

_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy: counter (..., 4) and key (..., 2) of 32-bit words -> (..., 4) uint32, the
    generator csrc/ppf_common.h implements."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(_PHILOX_W0)) & mask, (k[1] + np.uint64(_PHILOX_W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def default_counts(grid_cells, steps=14):
    """The cell counts of a curve: 0, G/steps, 2G/steps, ... G rounded half up, duplicates dropped: strictly increasing, from 0 to G."""
    G, steps = int(grid_cells), int(steps)
    if G < 1 or steps < 1:
        raise ValueError(f"default_counts: grid_cells={G} and steps={steps} must be >= 1")
    return np.unique((np.arange(steps + 1, dtype=np.int64) * 2 * G + steps) // (2 * steps)).astype(np.int32)


def cell_order_from_outputs(act_full, idx, token_attn, weight, scale, classes, grid_cells, mode="evidence", seed=0, image_ids=None, device=True):
    """A total order of the grid cells per (sample, class): (order, rank int32 [B, M, G], score fp32 [B, M, G]) with
    rank[b, m, order[b, m, r]] == r; the contract is ppf_cell_order's (include/ppf_hip.h).  act_full [B, P, T], idx [B, T] the grid cells of
    the reserved tokens, token_attn [B, G] the rollout attention, weight [C, P] the local last layer and scale its share of the logit,
    classes int32 [B, M].  mode 'evidence': reserved cells first, by their summed class evidence, then the others by attention;
    'attention': by the rollout attention; 'random': by Philox draws keyed by (seed, image id, cell) (image_ids [B]; None: 0 .. B-1).
    device=True: one ppf_cell_order launch on CUDA tensors.  device=False: the numpy referee -- the same fp32 product, an fp64 sum
    rounded once, np.lexsort, and the numpy Philox."""
    if mode not in ORDER_MODES:
        raise ValueError(f"cell_order_from_outputs: mode must be one of {ORDER_MODES}, got {mode!r}")
    G = int(grid_cells)
    if device:
        from . import ops
        ids = _image_ids(image_ids, classes.shape[0], classes.device) if mode == "random" else None
        return ops.cell_order(classes, G, mode, act_full=act_full, idx=idx, token_attn=token_attn, weight=weight, scale=scale, image_ids=ids, seed=seed)
    weight, cls = _host(weight, np.float32), _host(classes, np.int32)
    (B, M), (C, P) = cls.shape, weight.shape
    if not 1 <= G <= 1024 or not 1 <= M <= 8:
        raise ValueError(f"cell_order_from_outputs: G={G} or M={M} outside ppf_cell_order's limits (G <= 1024, 1 <= M <= 8)")
    order, rank = np.full((B, M, G), -1, dtype=np.int32), np.full((B, M, G), -1, dtype=np.int32)
    score = np.zeros((B, M, G), dtype=np.float32)
    if mode == "evidence":
        idx = _host(idx, np.int64)
        T = idx.shape[1]
        act_full = _host(act_full, np.float32).reshape(B, P, T)
        if not 1 <= T <= G:
            raise ValueError(f"cell_order_from_outputs: T={T} reserved tokens outside [1, G={G}]")
    if mode != "random":
        attn = _host(token_attn, np.float32).reshape(B, G)
    else:
        ids = np.arange(B, dtype=np.int64) if image_ids is None else _host(image_ids, np.int64).reshape(B)
        ids, sd = ids.astype(np.uint64), int(seed) & 0xFFFFFFFFFFFFFFFF
    cells = np.arange(G)
    with np.errstate(all="ignore"):
        w = (np.float32(scale) * weight).astype(np.float32)                          # fp32: the product of explain_from_outputs
        for b in range(B):
            for m in range(M):
                c = int(cls[b, m])
                if not 0 <= c < C:
                    continue
                tier = np.zeros(G, dtype=np.int64)
                if mode == "evidence":
                    tot = (w[c].astype(np.float64)[:, None] * act_full[b].astype(np.float64)).sum(axis=0).astype(np.float32)
                    tier[:], s = 1, attn[b].copy()
                    for t in range(T - 1, -1, -1):                                   # descending: a cell listed twice keeps its smallest t
                        if 0 <= idx[b, t] < G:
                            tier[idx[b, t]], s[idx[b, t]] = 0, tot[t]
                elif mode == "attention":
                    s = attn[b].copy()
                else:
                    ctr = np.stack([cells.astype(np.uint64), np.zeros(G, dtype=np.uint64), np.full(G, ids[b] & np.uint64(0xFFFFFFFF)),
                                    np.full(G, ids[b] >> np.uint64(32))], axis=-1)
                    word = philox4x32_10(ctr, np.array([sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint64))[:, 0]
                    s = (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
                nan = np.isnan(s)
                o = np.lexsort((cells, np.where(nan, np.float32(0), -s), nan, tier))   # tier, NaN last, score descending, smaller cell
                order[b, m], score[b, m] = o, s
                rank[b, m, o] = cells
    return order, rank, score


def perturb_patches(x, rank, counts, insertion=False, baseline=0.0, device=True):
    """The perturbed images [S, B, M, Cc, H, W] of x [B, Cc, H, W]: with rank [B, M, G] from cell_order_from_outputs and counts [S],
    deletion replaces the pixels of the cells with rank < counts[s] by the baseline, insertion keeps x in those cells only; a row of ranks
    -1 copies x.  baseline: a number (0 = the data-set mean colour in normalised space) or a tensor like x.  device=True: one
    ppf_patch_perturb launch (counts may be a host list); device=False: numpy."""
    if device:
        from . import ops
        counts = counts if isinstance(counts, torch.Tensor) else torch.from_numpy(np.asarray(counts, dtype=np.int32))
        return ops.patch_perturb(x, rank, counts.to(device=x.device, dtype=torch.int32).contiguous(), insertion, baseline)
    x, rank, counts = _host(x, np.float32), _host(rank, np.int64), _host(counts, np.int64).reshape(-1)
    (B, Cc, H, W), (M, G) = x.shape, rank.shape[1:]
    side = int(round(G ** 0.5))
    if H != W or side * side != G or H % side or (H // side) % 4:
        raise ValueError(f"perturb_patches: H={H} W={W} G={G}: square images, a square grid whose side divides H, patch width a multiple of 4")
    patch = H // side
    pix = rank.reshape(B, M, side, side).repeat(patch, axis=2).repeat(patch, axis=3)                # [B, M, H, W]: the rank of each pixel's cell
    keep = (pix[None] < 0) | ((pix[None] < counts[:, None, None, None, None]) == bool(insertion))   # [S, B, M, H, W]
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    return np.where(keep[:, :, :, None], x[None, :, None], base[None, :, None]).astype(np.float32)


# ---- the same test per pixel, from a blurred canvas (csrc/pixel_faithful.hip).  The metric as published removes PIXELS in saliency order,
# and its insertion curve starts from a blurred image: sharp islands on a flat canvas are out of distribution for every order alike.  The
# patch grid suits the model's own explanation and discards the resolution of the pixel maps (RISE, integrated gradients); here every
# order is a [B, M, H, W] score map, ranked by ppf_pixel_order and perturbed by ppf_pixel_perturb.  Opt-in: resolution="pixel" and
# baseline="blur" of faithfulness_curves / faithfulness.  The numpy forms (device=False) are the referees, bit for bit.
RESOLUTIONS = ("cell", "pixel")
BLUR_DEFAULTS = dict(sigma=5.0, radius=5)   # klen = 11, sigma = 5


def gauss_taps(sigma=5.0, radius=5):
    """fp32 [2 * radius + 1]: exp(-d^2 / (2 sigma^2)) for d = -radius .. radius, normalised in fp64 and cast once."""
    r, sigma = int(radius), float(sigma)
    if not 1 <= r <= 16 or not sigma > 0.0:
        raise ValueError(f"gauss_taps: radius={radius} outside [1, 16] (ppf_gauss_blur's limit) or sigma={sigma} not positive")
    d = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def _blur_axis(a, taps, axis):
    """One pass of the blur's contract along `axis` of an fp32 array: from +0, ascending d, one rounding per multiply and per add; a tap
    that falls outside the plane is skipped."""
    r, n = (taps.shape[0] - 1) // 2, a.shape[axis]
    a = np.moveaxis(a, axis, -1)
    acc = np.zeros(a.shape, dtype=np.float32)
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)                                         # the outputs whose tap d lies inside
        if lo < hi:
            acc[..., lo:hi] = acc[..., lo:hi] + (taps[d + r] * a[..., lo + d:hi + d]).astype(np.float32)
    return np.moveaxis(acc, -1, axis)


def gauss_blur(x, sigma=5.0, radius=5, device=True):
    """Every [H, W] plane of x fp32 [..., H, W] blurred separably (horizontal, then vertical) with gauss_taps(sigma, radius) and a zero
    border -- in normalised space a border of the data-set mean colour; the contract is ppf_gauss_blur's (include/ppf_hip.h).
    device=True: one launch on a CUDA tensor; device=False: numpy, a loop of rounded fp32 operations."""
    taps = gauss_taps(sigma, radius)
    if device:
        from . import ops
        return ops.gauss_blur(x, torch.from_numpy(taps).to(x.device))
    a = _host(x, np.float32)
    with np.errstate(all="ignore"):
        return _blur_axis(_blur_axis(a, taps, a.ndim - 1), taps, a.ndim - 2)


def pixel_order_from_scores(score, classes, device=True):
    """rank int32 classes.shape + (n,) of score fp32 classes.shape + (n,) (or + (H, W)): the number of pixels of the row that come before
    pixel i -- larger score first, ties by the smaller pixel index, NaN lowest, -0 == +0; a row whose class is negative is all -1.  The
    contract is ppf_pixel_order's (include/ppf_hip.h).  device=True: one launch; device=False: np.lexsort, NaN handled as
    cell_order_from_outputs handles it."""
    lead = tuple(classes.shape)
    R = int(np.prod(lead, dtype=np.int64))
    n = int(score.numel() if isinstance(score, torch.Tensor) else np.asarray(score).size) // max(R, 1)
    if device:
        from . import ops
        return ops.pixel_order(score.reshape(R, n), classes.reshape(R).contiguous()).reshape(lead + (n,))
    s, cls = _host(score, np.float32).reshape(R, n), _host(classes, np.int32).reshape(R)
    if not 1 <= n <= 65536:
        raise ValueError(f"pixel_order_from_scores: n={n} pixels outside ppf_pixel_order's limits [1, 65536]")
    rank, pixels = np.full((R, n), -1, dtype=np.int32), np.arange(n)
    with np.errstate(all="ignore"):
        for r in range(R):
            if cls[r] < 0:
                continue
            nan = np.isnan(s[r])
            rank[r, np.lexsort((pixels, np.where(nan, np.float32(0), -s[r]), nan))] = pixels     # NaN last, score descending, smaller pixel
    return rank.reshape(lead + (n,))


def pixel_random_scores(image_ids, pixels, seed=0, device=True):
    """fp32 [B, pixels]: (word >> 8) * 2^-24 of Philox4x32-10 keyed by seed at counter (pixel, 0x80000000, image id low, image id high)
    (ppf_pixel_random); a function of (seed, image id, pixel) alone.  device=False: the numpy Philox."""
    if device:
        from . import ops
        return ops.pixel_random(image_ids, pixels, seed)
    ids, n, sd = _host(image_ids, np.int64).reshape(-1).astype(np.uint64), int(pixels), int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((ids.shape[0], n, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1] = np.arange(n, dtype=np.uint64), 0x80000000
    ctr[..., 2], ctr[..., 3] = (ids & np.uint64(0xFFFFFFFF))[:, None], (ids >> np.uint64(32))[:, None]
    word = philox4x32_10(ctr, np.array([sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint64))[..., 0]
    return (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def perturb_pixels(x, rank, counts, insertion=False, baseline=0.0, device=True):
    """The perturbed images [S, B, M, Cc, H, W] of x [B, Cc, H, W]: with rank [B, M, H * W] from pixel_order_from_scores and counts [S],
    deletion replaces the pixels with rank < counts[s] by the baseline, insertion keeps x at those pixels only; a row of ranks -1 copies
    x.  baseline: a number or a tensor like x.  device=True: one ppf_pixel_perturb launch (counts may be a host list; W a multiple of 4);
    device=False: numpy."""
    if device:
        from . import ops
        counts = counts if isinstance(counts, torch.Tensor) else torch.from_numpy(np.asarray(counts, dtype=np.int32))
        return ops.pixel_perturb(x, rank, counts.to(device=x.device, dtype=torch.int32).contiguous(), insertion, baseline)
    x, rank, counts = _host(x, np.float32), _host(rank, np.int64), _host(counts, np.int64).reshape(-1)
    (B, Cc, H, W), M = x.shape, rank.shape[1]
    if rank.shape != (B, M, H * W):
        raise ValueError(f"perturb_pixels: rank must be [{B}, M, {H * W}], got {list(rank.shape)}")
    pix = rank.reshape(B, M, H, W)
    keep = (pix[None] < 0) | ((pix[None] < counts[:, None, None, None, None]) == bool(insertion))   # [S, B, M, H, W]
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    return np.where(keep[:, :, :, None], x[None, :, None], base[None, :, None]).astype(np.float32)


def _order_scores(ppnet, x, outs, cls, order, resolution, baseline, seed, image_ids, batch_size, scratch_bytes, rise, ig, shap=None):
    """(score, the Rise or None, the IntegratedGradients or None, the Shap or None) of an order at a resolution.  'pixel': score fp32
    [B, M, H, W], the map of pixel_scores.  'cell': the 'rise', 'ig' and 'shap' orders give their cell score fp32 [B, M, G]
    (_rank_cell_scores ranks it); 'evidence', 'attention' and 'random' give None: ppf_cell_order scores and ranks those in one launch
    (cell_order_from_outputs)."""
    from . import ops
    (B, _, H, W), M, G = x.shape, cls.shape[1], int(ppnet.num_patches)
    pixel = resolution == "pixel"
    if order in GAME_ORDERS:            # the one place the faithfulness code runs the KernelSHAP pass, from the curve's own baseline
        if pixel:
            raise ValueError(f"faithfulness: the {order!r} order is defined at resolution='cell' only (its players are grid cells; a "
                             "piecewise-constant pixel map is not provided)")
        found = _shap_from_classes(ppnet, x, cls, baseline=baseline, seed=seed, image_ids=image_ids, batch_size=batch_size, scratch_bytes=scratch_bytes,
                                   **{**SHAP_DEFAULTS, **(shap or {})})
        return found.cell, None, None, found
    if order in EXTRA_ORDERS + GRADIENT_ORDERS:
        if order in EXTRA_ORDERS:       # the one place the faithfulness code runs the RISE pass, from the curve's own baseline ...
            found = _rise_from_classes(ppnet, x, cls, baseline=baseline, seed=seed, image_ids=image_ids, batch_size=batch_size, scratch_bytes=scratch_bytes,
                                       **{**RISE_DEFAULTS, **(rise or {})})
            return (found.saliency.contiguous() if pixel else found.cell), found, None, None
        _refuse_pending_gradients("faithfulness_curves", ppnet)                                      # ... and integrated gradients
        found = _ig_pass(ppnet, x, outs, "logit", None, cls, baseline=baseline, batch_size=batch_size, **{**IG_DEFAULTS, **(ig or {})})
        a = found.attribution
        return (((a[:, :, 0] + a[:, :, 1]) + a[:, :, 2]).contiguous() if pixel else found.cell), None, found, None      # two rounded adds, in this order
    if not pixel:
        return None, None, None, None
    side = int(round(G ** 0.5))
    if order in ORDER_MODES[:2] and (H != W or side * side != G):
        raise ValueError(f"pixel_scores: the {order} map is up-sampled from a square grid to a square image, got G={G} and {H} x {W}")
    if order == "evidence":
        _, _, cell = cell_order_from_outputs(outs["act_full"], outs["idx"], outs["token_attn"], ppnet.last_layer.weight.detach().contiguous(),
                                             1.0 - float(ppnet.global_coe), cls, G, mode="evidence")
        idx = outs["idx"].long()
        reserved = torch.zeros((B, G + 1), dtype=torch.bool, device=x.device)
        reserved.scatter_(1, torch.where((idx >= 0) & (idx < G), idx, torch.full_like(idx, G)), True)      # entries outside the grid: the spare column
        grid = torch.where(reserved[:, None, :G], cell, torch.zeros_like(cell))
        return upsample_cubic_device(grid.reshape(B, M, side, side).contiguous(), H), None, None, None
    if order == "attention":
        up = upsample_cubic_device(outs["token_attn"].reshape(B, side, side).contiguous(), H)
        return up[:, None].expand(B, M, H, W).contiguous(), None, None, None
    if order == "random":
        s = ops.pixel_random(_image_ids(image_ids, B, x.device), H * W, seed)
        return s.reshape(B, 1, H, W).expand(B, M, H, W).contiguous(), None, None, None
    raise ValueError(f"pixel_scores: order must be one of {ORDER_MODES + EXTRA_ORDERS + GRADIENT_ORDERS}, got {order!r}")


def _rank_cell_scores(cell, cls, G, weight):
    """(order, rank int32, score fp32 [B, M, G]) of a cell score [B, M, G]: ppf_cell_order's attention mode over the B * M (sample, class)
    rows, so the total order, the NaN rule and the -1 rows of an invalid class are that kernel's."""
    from . import ops
    B, M = cls.shape
    return tuple(t.reshape(B, M, G) for t in ops.cell_order(cls.reshape(B * M, 1).contiguous(), G, "attention", token_attn=cell.reshape(B * M, G),
                                                            weight=weight))


def pixel_scores(ppnet, x, outs, cls, order, baseline=0.0, seed=0, image_ids=None, batch_size=None, scratch_bytes=1 << 30, rise=None, ig=None):
    """The map fp32 [B, M, H, W] (device) whose pixels the order `order` removes largest first, for x [B, 3, H, W], the eval outputs of its
    forward (outs) and the classes cls int32 [B, M]:
      'evidence'   the g x g grid that holds, on the reserved cells, the class evidence ppf_cell_order's mode 0 returns and 0 elsewhere,
                   up-sampled to H by upsample_cubic_device -- the map a person is shown.  The two-tier rule of the cell order (reserved
                   cells first, then the others by attention) is NOT carried over: an unreserved cell has no evidence, and the cubic
                   kernel mixes neighbouring cells anyway;
      'attention'  the rollout grid, up-sampled the same way (the same for every class);
      'random'     ppf_pixel_random of (seed, image id, pixel), the same for every class;
      'rise'       Rise.saliency of rise_saliency with this baseline, seed, image_ids (rise = dict(masks=, cells=, p=));
      'ig'         (a[:, :, 0] + a[:, :, 1]) + a[:, :, 2] of the attribution of integrated_gradients from this baseline, two rounded fp32
                   adds in that order (ig = dict(steps=, rule=)).
    The caller holds no_grad."""
    return _order_scores(ppnet, x, outs, cls, order, "pixel", baseline, seed, image_ids, batch_size, scratch_bytes, rise, ig)[0]


def _resolve_baseline(baseline, x, blur):
    """The baseline of a curve: a number or a tensor as given; the string 'blur': gauss_blur(x) with BLUR_DEFAULTS overridden by `blur`."""
    if isinstance(baseline, str):
        if baseline != "blur":
            raise ValueError(f"faithfulness: baseline must be a number, a tensor like x or 'blur', got {baseline!r}")
        return gauss_blur(x, **{**BLUR_DEFAULTS, **(blur or {})})
    return baseline


class Faithfulness(Record):
    """What faithfulness_curves returns, as device tensors (numpy arrays after cpu()): curves[mode] fp32 [B, M, S] = the probability of
    class classes[b, m] after counts[s] cells were removed ('deletion') or shown ('insertion'); counts int32 [S]; classes int32 [B, M];
    order, rank int32 and score fp32 [B, M, G] as ppf_cell_order wrote them.  grid_cells = G.  rise: the Rise the 'rise' order ranked by
    (its cell scores are `score`), None for every other order; ig: likewise the IntegratedGradients of the 'ig' order; shap: likewise the
    Shap of the 'shap' order.
    resolution 'pixel': counts are pixels, grid_cells = H * W, rank int32 and score fp32 are [B, M, H * W] as ppf_pixel_order ranked them,
    and order is None (51 MB per class column at 224^2 that nobody reads)."""
    FIELDS = ("curves", "counts", "classes", "order", "rank", "score")
    META = dict(grid_cells=int, rise=None, ig=None, resolution=str, shap=None)
    DEFAULTS = dict(rise=None, ig=None, resolution="cell", shap=None)

    def auc(self):
        """{mode: fp64 [B, M]}: the area under each curve over the removed / shown fraction counts / G (trapezoid, on the host)."""
        h = self.cpu()
        return {k: curve_auc(v, h.counts, h.grid_cells) for k, v in h.curves.items()}


def curve_auc(curves, counts, grid_cells):
    """Trapezoid of curves [..., S] over counts / grid_cells, in fp64."""
    f = np.asarray(counts, dtype=np.float64) / float(grid_cells)
    c = np.asarray(curves, dtype=np.float64)
    return ((c[..., 1:] + c[..., :-1]) * 0.5 * np.diff(f)).sum(-1)


def _eval_outputs(ppnet, x):
    """One eval forward: what the cell orders, the class pick and the focus pass need, all on the device."""
    r = ppnet.eval_branches(x)
    return dict(token_attn=r.cls_attn.reshape(x.shape[0], -1).float().contiguous(), idx=r.idx.contiguous(), act_full=r.act_full.contiguous(),
                logits=r.logits.contiguous(), act_max=r.act_max_local, act_max_global=r.act_max_global, argmax=r.argmax,
                logits_global=r.logits_global)


def _image_ids(image_ids, B, device):
    """image_ids [B], or 0 .. B-1 for None, as int64 on the device."""
    if image_ids is None:
        return torch.arange(B, dtype=torch.int64, device=device)
    return torch.as_tensor(image_ids).to(device=device, dtype=torch.int64).contiguous()


def _chunk_items(total, scratch_bytes, bytes_per_item):
    """How many of `total` items one scratch buffer of scratch_bytes holds: one at least."""
    return max(1, min(total, int(scratch_bytes) // bytes_per_item))


def _class_probs(ppnet, imgs, cols, batch_size):
    """The probabilities fp32 [R] of the classes cols[j] int32 [R] of the images imgs [R, C, H, W], per column: the model's forward in
    sub-batches of batch_size images, then one ppf_class_prob per column.  The caller holds eval mode and no_grad."""
    from . import ops
    logits = torch.cat([r.logits for r in forward_groups(ppnet, imgs, batch_size)]).contiguous()
    return [ops.class_prob(logits, c) for c in cols]


def _curves_from_outputs(ppnet, x, outs, cls, counts, modes, order, baseline, seed, image_ids, batch_size, scratch_bytes, rise=None, ig=None,
                         resolution="cell", shap=None):
    from . import ops
    B, G = x.shape[0], int(ppnet.num_patches)
    M, S = cls.shape[1], counts.shape[0]
    w_l = ppnet.last_layer.weight.detach().contiguous()
    ordr, perturb = None, ops.patch_perturb
    score, found, found_ig, found_shap = _order_scores(ppnet, x, outs, cls, order, resolution, baseline, seed, image_ids, batch_size, scratch_bytes,
                                                       rise, ig, shap)
    if resolution == "pixel":
        # every order is a [B, M, H, W] map (pixel_scores); one ppf_pixel_order launch ranks the B * M rows, ppf_pixel_perturb takes
        # ppf_patch_perturb's place below.  The chunking, the forwards and ppf_class_prob are the cell path's.
        G, perturb = x.shape[2] * x.shape[3], ops.pixel_perturb
        score = score.reshape(B, M, G)
        rank = pixel_order_from_scores(score, cls)
    elif score is not None:
        # 'rise': the cells ranked by their mean RISE saliency; 'ig': by the integrated gradients of the class logit summed over each
        # cell, along the path from the curve's own baseline; 'shap': by the Shapley value of their player, shared among its cells
        ordr, rank, score = _rank_cell_scores(score, cls, G, w_l)
    else:
        ordr, rank, score = cell_order_from_outputs(outs["act_full"], outs["idx"], outs["token_attn"], w_l, 1.0 - float(ppnet.global_coe), cls, G,
                                                    mode=order, seed=seed, image_ids=image_ids)
    # scratch: the perturbed images of one chunk of steps, steps_per_chunk * B * M images, never more than scratch_bytes (one step at least)
    chunk = _chunk_items(S, scratch_bytes, B * M * x[0].numel() * 4)
    cls_flat = cls.reshape(1, B * M).expand(chunk, B * M).reshape(-1).contiguous()
    buf = torch.empty((chunk, B, M) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    curves = {}
    with ppnet.eval_mode():
        for mode in modes:
            if mode not in CURVE_MODES:
                raise ValueError(f"faithfulness_curves: modes must come from {CURVE_MODES}, got {mode!r}")
            prob = torch.empty((S, B, M), dtype=torch.float32, device=x.device)
            for s0 in range(0, S, chunk):
                n = min(chunk, S - s0)
                imgs = perturb(x, rank, counts[s0:s0 + n].contiguous(), mode == "insertion", baseline, out=buf[:n])
                imgs = imgs.reshape((n * B * M,) + tuple(x.shape[1:]))
                prob[s0:s0 + n] = _class_probs(ppnet, imgs, [cls_flat[:n * B * M]], int(batch_size or B))[0].reshape(n, B, M)
            curves[mode] = prob.permute(1, 2, 0).contiguous()
    return Faithfulness(curves, counts, cls, ordr, rank, score, G, rise=found, ig=found_ig, resolution=resolution, shap=found_shap)


def _pick_classes(ppnet, outs, classes, top_classes, B):
    """classes as explain takes them; None: the top `top_classes` of the logits, picked as ppf_explain_topk picks them."""
    from . import ops
    C = ppnet.last_layer.weight.shape[0]
    if classes is not None:
        return _explain_classes(classes, B, C, outs["logits"].device)
    return ops.explain_topk(outs["act_max"], ppnet.last_layer.weight.detach().contiguous(), 1.0 - float(ppnet.global_coe), ppnet.num_prototypes_per_class,
                            outs["logits"], 1, top_classes=top_classes)["classes"]


@torch.no_grad()
def faithfulness_curves(ppnet, x, classes=None, top_classes=1, counts=None, modes=CURVE_MODES, order="evidence", baseline=0.0, seed=0, image_ids=None,
                        batch_size=None, scratch_bytes=1 << 30, rise=None, ig=None, resolution="cell", blur=None, shap=None):
    """Deletion / insertion curves of a batch x [B, 3, H, W] (CUDA): one eval forward, one ppf_cell_order launch, then per mode
    ppf_patch_perturb in chunks of steps, the model's forward over each chunk in sub-batches of `batch_size` images (default B; the
    images of a chunk are ordered step, sample, class) and one ppf_class_prob per chunk.  The chunk's images are the one large scratch
    buffer: steps-per-chunk = scratch_bytes // (B * M * image bytes), at least one step, so at most max(scratch_bytes, one step) bytes.
    classes: as in explain (None: the top `top_classes` of the logits).  counts: the numbers of cells removed / shown (default
    default_counts(G)).  order: 'evidence', 'attention' or 'random' (seed, image_ids: the random order's key), or 'rise': the cells ranked
    by their RISE saliency for the class (rise_saliency with the same baseline, seed, image_ids, batch_size and scratch_bytes;
    rise = dict(masks=, cells=, p=) overrides RISE_DEFAULTS; the result carries the Rise), or 'ig': by the integrated gradients of the
    class logit summed over each cell (integrated_gradients along the path from the same baseline, in the same sample groups;
    ig = dict(steps=, rule=) overrides IG_DEFAULTS; the result carries the IntegratedGradients), or 'shap': by the Shapley value of the
    cell's player for the class (kernel_shap with the same baseline, seed, image_ids, batch_size and scratch_bytes;
    shap = dict(samples=, cells=, value=) overrides SHAP_DEFAULTS; the result carries the Shap; cell resolution only).  baseline: what a removed pixel becomes, a
    number in normalised space (0 = the data-set mean colour), a tensor like x, or 'blur': gauss_blur(x) with blur = dict(sigma=, radius=)
    over BLUR_DEFAULTS, computed once and used wherever the baseline is (the rise and ig passes included).  resolution 'pixel': the
    metric as published -- the order's [B, M, H, W] map (pixel_scores) is ranked by one ppf_pixel_order launch, counts are pixels (default
    default_counts(H * W)) and ppf_pixel_perturb builds the images; everything else is the same.  Returns a Faithfulness (device
    tensors; nothing is read back here)."""
    if resolution not in RESOLUTIONS:
        raise ValueError(f"faithfulness_curves: resolution must be one of {RESOLUTIONS}, got {resolution!r}")
    if not x.is_cuda:
        raise RuntimeError("faithfulness_curves needs a CUDA/HIP batch (no CPU fallback path; cell_order_from_outputs / perturb_patches with "
                           "device=False are the host referees)")
    x = x.float().contiguous()
    G = int(ppnet.num_patches) if resolution == "cell" else x.shape[2] * x.shape[3]
    baseline = _resolve_baseline(baseline, x, blur)
    outs = _eval_outputs(ppnet, x)
    cls = _pick_classes(ppnet, outs, classes, top_classes, x.shape[0])
    counts = _device_counts(counts, G, x.device)
    return _curves_from_outputs(ppnet, x, outs, cls, counts, tuple(modes), order, baseline, seed, image_ids, batch_size, scratch_bytes, rise, ig,
                                resolution, shap)


def _device_counts(counts, G, device):
    c = default_counts(G) if counts is None else np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts)
    if c.ndim != 1 or c.size < 2 or c.dtype.kind not in "iu" or c.min() < 0 or c.max() > G or (np.diff(c) <= 0).any():
        raise ValueError(f"faithfulness: counts must be at least two strictly increasing integers in [0, {G}], got {c.tolist()}")
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(device)


@torch.no_grad()
def faithfulness(ppnet, loader, orders=ORDER_MODES, modes=CURVE_MODES, counts=None, top_classes=1, against_label=False, baseline=0.0, seed=0,
                 max_images=0, batch_size=None, scratch_bytes=1 << 30, rise=None, ig=None, resolution="cell", blur=None, shap=None):
    """The curves over a data set.  loader yields (x, labels) or (x, labels, ids); without ids an image's id is its running index.  Per
    batch one eval forward serves every order (orders may name 'rise', with rise = dict(masks=, cells=, p=), 'ig', with ig = dict(steps=, rule=), and 'shap', with shap = dict(samples=, cells=, value=)); classes are the top `top_classes` of the logits, or with against_label the image's label.
    The per-image curves stay on the device and are read back once at the end.  Returns dict(images, counts, grid_cells, orders:
    {order: {mode: dict(curve = the mean curve [S], auc = the mean area)}}, per_image: {order: {mode: fp32 [N, M, S]}}, classes [N, M],
    image_ids [N]); rows whose class could not be picked (-1) are left out of the means.  resolution, baseline = 'blur' and blur: as in
    faithfulness_curves (the blurred batch is computed once per batch and serves every order); at pixel resolution counts are pixels
    and grid_cells = H * W."""
    if resolution not in RESOLUTIONS:
        raise ValueError(f"faithfulness: resolution must be one of {RESOLUTIONS}, got {resolution!r}")
    G, kept, cls_kept, ids_kept, seen, dev_counts = int(ppnet.num_patches), {}, [], [], 0, None
    given = baseline
    for x, y, ids in batches_with_ids(loader, max_images):
        x = (x if x.is_cuda else x.cuda()).float().contiguous()
        B, ids = x.shape[0], ids.to(x.device)               # on the device once: the random / rise orders key by them, the closing read takes them
        if resolution == "pixel":
            G = x.shape[2] * x.shape[3]
        baseline = _resolve_baseline(given, x, blur)
        outs = _eval_outputs(ppnet, x)
        cls = _pick_classes(ppnet, outs, torch.as_tensor(y).to(x.device) if against_label else None, top_classes, B)
        if dev_counts is None:
            dev_counts = _device_counts(counts, G, x.device)
        for order in orders:
            f = _curves_from_outputs(ppnet, x, outs, cls, dev_counts, tuple(modes), order, baseline, seed, ids, batch_size, scratch_bytes, rise, ig,
                                     resolution, shap)
            for mode in modes:
                kept.setdefault((order, mode), []).append(f.curves[mode])
        cls_kept.append(cls); ids_kept.append(ids)
        seen += B
    if not seen:
        raise ValueError("faithfulness: the loader gave no image")
    keys = list(kept)
    read = read_once(dict(curves=torch.stack([torch.cat(kept[k]) for k in keys]), classes=torch.cat(cls_kept), counts=dev_counts,
                          image_ids=torch.cat(ids_kept)))                                    # the one read; curves: [orders * modes, N, M, S]
    host, classes, cnt = read["curves"], read["classes"], read["counts"]
    valid = classes >= 0
    out = dict(images=seen, counts=cnt.tolist(), grid_cells=G, orders={}, per_image={}, classes=classes, image_ids=read["image_ids"])
    for j, (order, mode) in enumerate(keys):
        rows = host[j][valid].astype(np.float64)                                             # [rows, S]
        out["orders"].setdefault(order, {})[mode] = dict(curve=rows.mean(0).tolist(), auc=float(curve_auc(rows, cnt, G).mean()))
        out["per_image"].setdefault(order, {})[mode] = host[j]
    return out


# ------------------------------------------------------------------------------------------------ RISE: the black-box baseline of the faithfulness test
# RISE (Petsiuk et al., 2018) is the saliency the deletion / insertion metric was published with: N random masks per image, the class
# probability of every masked image, saliency = the probability-weighted mean mask.  It needs forwards alone, so it answers whether the
# prototype evidence is as faithful as what a model-agnostic method finds.  The masks are integer-exact (the contract is in
# include/ppf_hip.h): ppf_rise_nodes draws the node tables, ppf_rise_apply writes the masked images of a chunk of masks, the model's
# forward and ppf_class_prob score them, ppf_rise_accumulate regenerates the masks and sums (csrc/rise.hip).  The numpy forms below
# (device=False) are the referees, bit for bit.  The reference has no such pass.
RISE_DEFAULTS = dict(masks=512, cells=7, p=0.5)


def rise_threshold(p):
    """The integer keep threshold round(p * 2^24) in [1, 2^24]: a node is on when its 24-bit draw lies below it."""
    thr = int(round(float(p) * (1 << 24)))
    if not 1 <= thr <= 1 << 24:
        raise ValueError(f"rise: the keep probability p={p} gives thr={thr} outside [1, 2^24]")
    return thr


def _rise_sizes(size, cells):
    """(H, s, c, L) of the mask contract: node spacing c = ceil(H / s), L = s + 2 nodes per side."""
    H, s = int(size), int(cells)
    if not 1 <= s <= 14 or H < 4 or H % 4:
        raise ValueError(f"rise: cells={s} outside [1, 14] or size={H} no positive multiple of 4")
    c = -(-H // s)
    if c > 4096:
        raise ValueError(f"rise: node spacing c={c} = ceil({H} / {s}) exceeds 4096")
    return H, s, c, s + 2


def rise_nodes_from_ids(image_ids, size, masks=512, cells=7, p=0.5, seed=0, device=True):
    """(nodes uint8 [B, N, (cells + 2)^2] of 0 / 1, shift int32 [B, N, 2] = (dy, dx)) of the N = masks RISE masks of the images image_ids
    [B] at size x size pixels: a function of (seed, image id, mask) alone, not of the batch.  device=True: one ppf_rise_nodes launch
    (image_ids a CUDA tensor or anything torch.as_tensor takes, then put on the current device); device=False: the numpy Philox."""
    H, s, c, L = _rise_sizes(size, cells)
    N, thr = int(masks), rise_threshold(p)
    if not 1 <= N <= 2 ** 31 - 2:
        raise ValueError(f"rise: masks={N} outside [1, 2^31 - 2]")
    if device:
        from . import ops
        ids = torch.as_tensor(image_ids)
        ids = ids.to(device=ids.device if ids.is_cuda else "cuda", dtype=torch.int64).contiguous()
        return ops.rise_nodes(ids, H, N, s, thr, seed)
    ids = _host(image_ids, np.int64).reshape(-1).astype(np.uint64)
    B, LL = ids.shape[0], L * L
    Q, sd = (LL + 3) // 4, int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((B, N, Q + 1, 4), dtype=np.uint64)
    ctr[..., 0] = np.concatenate([np.arange(Q), [0xFFFFFFFF]]).astype(np.uint64)                  # the call after the node words: the shift
    ctr[..., 1] = (1 + np.arange(N, dtype=np.uint64))[None, :, None]
    ctr[..., 2], ctr[..., 3] = (ids & np.uint64(0xFFFFFFFF))[:, None, None], (ids >> np.uint64(32))[:, None, None]
    w = philox4x32_10(ctr, np.array([sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint64)) >> np.uint32(8)    # [B, N, Q + 1, 4], 24 bits each
    nodes = (w[:, :, :Q].reshape(B, N, Q * 4)[:, :, :LL] < np.uint32(thr)).astype(np.uint8)
    shift = ((w[:, :, Q, :2].astype(np.uint64) * np.uint64(c)) >> np.uint64(24)).astype(np.int32)
    return nodes, shift


def rise_masks(nodes, shift, size, cells):
    """The integer numerators K int32 [B, N, H, H] of the masks (mask value = K / c^2): bilinear interpolation of the L x L node grid with
    spacing c, shifted by (dy, dx), in integers."""
    H, s, c, L = _rise_sizes(size, cells)
    nodes, shift = _host(nodes, np.int64), _host(shift, np.int64)
    B, N = nodes.shape[:2]
    g = nodes.reshape(B, N, L, L)
    if (shift < 0).any() or (shift >= c).any():
        raise ValueError(f"rise_masks: shifts outside [0, c={c})")
    u = np.arange(H)[None, None, :, None] + shift[:, :, None, :]                                  # [B, N, H, 2]: (y + dy, x + dx)
    (i, j), (ry, rx) = np.moveaxis(u // c, -1, 0), np.moveaxis(u % c, -1, 0)
    bi, ni = np.arange(B)[:, None, None, None], np.arange(N)[None, :, None, None]
    I, J, RY, RX = i[:, :, :, None], j[:, :, None, :], ry[:, :, :, None], rx[:, :, None, :]
    K = (c - RY) * ((c - RX) * g[bi, ni, I, J] + RX * g[bi, ni, I, J + 1]) + RY * ((c - RX) * g[bi, ni, I + 1, J] + RX * g[bi, ni, I + 1, J + 1])
    return K.astype(np.int32)


def rise_apply(x, nodes, shift, cells, n0=0, count=None, baseline=0.0, device=True, out=None):
    """The masked images [Nc, B, Cc, H, W] of x [B, Cc, H, W] under masks n0 .. n0 + count - 1 (default: to the last):
    m * x + (1 - m) * baseline with m = K / c^2, every operation rounded once to fp32.  baseline: a number or a tensor like x.
    device=True: one ppf_rise_apply launch; device=False: numpy."""
    if device:
        from . import ops
        return ops.rise_apply(x, nodes, shift, cells, n0, count, baseline, out=out)
    x, nodes, shift = _host(x, np.float32), _host(nodes, np.uint8), _host(shift, np.int32)
    H, s, c, L = _rise_sizes(x.shape[2], cells)
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"rise_apply: H={x.shape[2]} W={x.shape[3]}: square images only")
    n0, N = int(n0), nodes.shape[1]
    Nc = N - n0 if count is None else int(count)
    if n0 < 0 or Nc < 1 or n0 + Nc > N:
        raise ValueError(f"rise_apply: masks {n0} .. {n0 + Nc - 1} outside [0, {N})")
    K = rise_masks(nodes[:, n0:n0 + Nc], shift[:, n0:n0 + Nc], H, s)
    m = (K.astype(np.float32) / np.float32(c * c)).transpose(1, 0, 2, 3)[:, :, None]              # [Nc, B, 1, H, W], one rounding
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    with np.errstate(all="ignore"):
        return (m * x[None] + (np.float32(1) - m) * base[None]).astype(np.float32)


def rise_accumulate(nodes, shift, prob, size, cells, grid_cells, p=0.5, device=True):
    """(sal fp32 [B, M, H, H], cell fp32 [B, M, G]) from the node tables and prob fp32 [N, B, M]: sal = (fp64 sum over n ascending of
    prob * K) / norm with norm = N * (thr / 2^24) * c^2, cell = (fp64 sum over n ascending of prob * W) / (norm * patch^2) with W = K summed
    over the cell's pixels; each rounded once to fp32.  device=True: ppf_rise_accumulate; device=False: numpy, mask by mask."""
    H, s, c, L = _rise_sizes(size, cells)
    thr, G = rise_threshold(p), int(grid_cells)
    if device:
        from . import ops
        return ops.rise_accumulate(nodes, shift, prob, H, s, G, thr)
    prob = _host(prob, np.float32)
    N, B, M = prob.shape
    side = int(round(G ** 0.5))
    if side * side != G or H % side or not 1 <= M <= 8:
        raise ValueError(f"rise_accumulate: G={G} must be a square grid whose side divides H={H}, and M={M} lie in [1, 8]")
    patch = H // side
    if patch * patch * c * c > 1 << 29:
        raise ValueError(f"rise_accumulate: cell mass patch^2 * c^2 = {patch * patch * c * c} exceeds 2^29")
    K = rise_masks(nodes, shift, H, s)                                                            # [B, N, H, H]
    W = K.reshape(B, N, side, patch, side, patch).sum(axis=(3, 5), dtype=np.int64).reshape(B, N, G)
    norm = float(N) * (thr / 16777216.0) * float(c * c)
    acc, acc_w = np.zeros((B, M, H, H), dtype=np.float64), np.zeros((B, M, G), dtype=np.float64)
    with np.errstate(all="ignore"):
        for n in range(N):                                                                        # ascending: the order is the contract
            pn = prob[n].astype(np.float64)
            acc += pn[:, :, None, None] * K[:, n, None].astype(np.float64)
            acc_w += pn[:, :, None] * W[:, n, None].astype(np.float64)
        return (acc / norm).astype(np.float32), (acc_w / (norm * float(patch * patch))).astype(np.float32)


class Rise(Record):
    """What rise_saliency returns, as device tensors (numpy arrays after cpu()): saliency fp32 [B, M, H, W], cell fp32 [B, M, G] (the mean
    saliency of each grid cell), prob fp32 [N, B, M] (the class probabilities of the masked images), nodes uint8 [B, N, L*L], shift int32
    [B, N, 2], classes int32 [B, M]; cells, p: the mask parameters."""
    FIELDS = ("saliency", "cell", "prob", "shift", "classes", "nodes")
    META = dict(cells=int, p=float)


def _rise_from_classes(ppnet, x, cls, masks, cells, p, baseline, seed, image_ids, batch_size, scratch_bytes):
    from . import ops
    B, G, H = x.shape[0], int(ppnet.num_patches), x.shape[2]
    M, N, thr = cls.shape[1], int(masks), rise_threshold(p)
    nodes, shift = ops.rise_nodes(_image_ids(image_ids, B, x.device), H, N, cells, thr, seed)
    # scratch: the masked images of one chunk of masks, masks_per_chunk * B images, never more than scratch_bytes (one mask at least)
    chunk = _chunk_items(N, scratch_bytes, x.numel() * 4)
    cols = [cls[:, m].reshape(1, B).expand(chunk, B).reshape(-1).contiguous() for m in range(M)]
    buf = torch.empty((chunk,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    prob = torch.empty((N, B, M), dtype=torch.float32, device=x.device)
    with ppnet.eval_mode():
        for n0 in range(0, N, chunk):
            n = min(chunk, N - n0)
            imgs = ops.rise_apply(x, nodes, shift, cells, n0, n, baseline, out=buf[:n]).reshape((n * B,) + tuple(x.shape[1:]))
            # the mask does not depend on the class: one image serves all M columns
            for m, pr in enumerate(_class_probs(ppnet, imgs, [c[:n * B] for c in cols], int(batch_size or B))):
                prob[n0:n0 + n, :, m] = pr.reshape(n, B)
    sal, cell = ops.rise_accumulate(nodes, shift, prob, H, cells, G, thr)
    return Rise(sal, cell, prob, shift, cls, nodes, cells, p)


@torch.no_grad()
def rise_saliency(ppnet, x, classes=None, top_classes=1, masks=512, cells=7, p=0.5, baseline=0.0, seed=0, image_ids=None, batch_size=None,
                  scratch_bytes=1 << 30):
    """RISE saliency of a batch x [B, 3, H, W] (CUDA) for the classes of explain (None: the top `top_classes` of the logits): one eval
    forward and the class pick, one ppf_rise_nodes launch, then per chunk of masks ppf_rise_apply into the one scratch buffer
    (masks-per-chunk = scratch_bytes // (B * image bytes), at least one), the model's forward over the chunk in sub-batches of
    `batch_size` images (default B; the images of a chunk are ordered mask, sample) and ppf_class_prob once per class column; one
    ppf_rise_accumulate at the end.  masks = N, cells = s low-resolution cells per side, p the keep probability, baseline what a masked
    pixel tends to (a number in normalised space or a tensor like x); seed, image_ids [B] (None: 0 .. B-1) key the masks, so an image's
    result does not depend on its batch.  Returns a Rise (device tensors; nothing is read back here)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("rise_saliency needs a CUDA/HIP batch (no CPU fallback path; rise_nodes_from_ids / rise_apply / rise_accumulate with "
                           "device=False are the host referees)")
    x = x.float().contiguous()
    outs = _eval_outputs(ppnet, x)
    cls = _pick_classes(ppnet, outs, classes, top_classes, x.shape[0])
    return _rise_from_classes(ppnet, x, cls, masks, cells, p, baseline, seed, image_ids, batch_size, scratch_bytes)


# ------------------------------------------------------------------------------------------------ KernelSHAP: Shapley values of grid cells
# KernelSHAP (Lundberg & Lee, 2017) is the baseline a reader of the faithfulness table asks for after RISE and integrated gradients.  Its
# players are d = cells x cells square blocks of grid cells, the resolution of the 'evidence' order; it needs forwards alone, as RISE;
# and it is efficient by construction: the attributions add up to f(x) - f(baseline) exactly (to rounding), even across the jumps of the
# token reservation, where the `delta` of integrated gradients does not fall with more steps.  N coalitions are drawn in complementary
# pairs (Covert & Lee, 2021) with sizes from the Shapley kernel's distribution, so the weighted regression becomes a plain one: A = Z^T Z,
# b = Z^T (v - v0), solved under sum phi = v1 - v0.  Coalitions, masked images and A are integer-exact (the contract is in
# include/ppf_hip.h): ppf_shap_coalitions draws, ppf_shap_apply writes the masked images of a chunk of samples, the model's forward scores
# them, ppf_shap_gram sums and ppf_shap_solve factors in fp64 (csrc/shap.hip).  The numpy forms below (device=False) are the referees.
# The reference has no such pass, and nobody has run this one on a trained checkpoint.
SHAP_DEFAULTS = dict(samples=512, cells=7, value="prob")
SHAP_VALUES = ("prob", "logit")


def _shap_sizes(cells, samples=None):
    """(s, d, Wd) of the coalition contract: d = s^2 players in ceil(d / 32) words; samples, when given, even and in [2, 2^30]."""
    s = int(cells)
    if not 2 <= s <= 14:
        raise ValueError(f"shap: cells={s} outside [2, 14]")
    if samples is not None and (int(samples) % 2 or not 2 <= int(samples) <= 1 << 30):
        raise ValueError(f"shap: samples={int(samples)} must be even and lie in [2, 2^30] (coalitions are drawn in complementary pairs)")
    return s, s * s, (s * s + 31) // 32


def shap_size_table(d):
    """int32 [d - 1]: table[t] = round(2^24 * P(size <= t + 1)) under the Shapley kernel's distribution of coalition sizes,
    P(size = k) ~ 1 / (k (d - k)) for k = 1 .. d - 1, in exact rational arithmetic (halves round up); non-decreasing, table[d - 2] = 2^24."""
    from fractions import Fraction
    d = int(d)
    if not 4 <= d <= 196:
        raise ValueError(f"shap_size_table: d={d} outside [4, 196]")
    w = [Fraction(1, k * (d - k)) for k in range(1, d)]
    total, run, table = sum(w), Fraction(0), []
    for wk in w:
        run += wk
        table.append(int((run / total * (1 << 25) + 1) // 2))
    return np.asarray(table, dtype=np.int32)


def shap_members(coal, cells):
    """bool [B, N, d]: the membership bits of coal [B, N, Wd] (uint32 words, or the int32 a device tensor holds them in), unpacked."""
    s, d, Wd = _shap_sizes(cells)
    w = _host(coal, np.int32).view(np.uint32)
    return (((w[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(w.shape[:2] + (Wd * 32,))[..., :d]).astype(bool)


def _shap_player_maps(size, cells, grid_cells=None):
    """The player of every pixel [H, H], or of every grid cell [G] with r = side / cells."""
    s, d, _ = _shap_sizes(cells)
    if grid_cells is None:
        H = int(size)
        if H % s or (H // s) % 4:
            raise ValueError(f"shap: cells={s} must divide H={H} into players whose width is a multiple of 4")
        q = np.arange(H) // (H // s)
        return q[:, None] * s + q[None, :]
    G = int(grid_cells)
    side = int(round(G ** 0.5))
    if side * side != G or side % s or G > 1024:
        raise ValueError(f"shap: cells={s} must divide the side of a square grid of at most 1024 cells, got G={G}")
    q = np.arange(side) // (side // s)
    return (q[:, None] * s + q[None, :]).reshape(G)


def shap_coalitions_from_ids(image_ids, cells, samples, seed=0, device=True):
    """coal [B, N, ceil(d / 32)]: bit q % 32 of word q / 32 says whether player q of d = cells^2 is in coalition n of image image_ids[b];
    coalition 2j + 1 is the complement of coalition 2j, whose size follows shap_size_table(d) and whose members are a uniform subset, from
    Philox draws keyed by (seed, image id, j): a function of (seed, image id, n, d) alone, not of the batch.  device=True: one
    ppf_shap_coalitions launch, an int32 CUDA tensor holding the uint32 words (image_ids a CUDA tensor or anything torch.as_tensor
    takes, then put on the current device); device=False: the numpy Philox, uint32."""
    s, d, Wd = _shap_sizes(cells, samples)
    N, table = int(samples), shap_size_table(d)
    if device:
        from . import ops
        ids = torch.as_tensor(image_ids)
        ids = ids.to(device=ids.device if ids.is_cuda else "cuda", dtype=torch.int64).contiguous()
        return ops.shap_coalitions(ids, s, N, table, seed)
    ids = _host(image_ids, np.int64).reshape(-1).astype(np.uint64)
    B, P, Q, sd = ids.shape[0], N // 2, (d + 3) // 4, int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((B, P, Q + 1, 4), dtype=np.uint64)
    ctr[..., 0] = np.concatenate([np.arange(Q), [0xFFFFFFFF]]).astype(np.uint64)                  # the call after the key words: the size
    ctr[..., 1] = (np.uint64(0x80000001) + np.arange(P, dtype=np.uint64))[None, :, None]
    ctr[..., 2], ctr[..., 3] = (ids & np.uint64(0xFFFFFFFF))[:, None, None], (ids >> np.uint64(32))[:, None, None]
    w = philox4x32_10(ctr, np.array([sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint64))                # [B, P, Q + 1, 4]
    keys = w[:, :, :Q].reshape(B, P, Q * 4)[:, :, :d]
    u = (w[:, :, Q, 0] >> np.uint32(8)).astype(np.int64)
    size = 1 + (table[None, None, :d - 2].astype(np.int64) <= u[..., None]).sum(-1)                # [B, P], in [1, d - 1]
    order = np.argsort(keys, axis=-1, kind="stable")                                              # (key, player) ascending
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(d), order.shape), axis=-1)
    even = rank < size[..., None]
    z = np.stack([even, ~even], axis=2).reshape(B, N, d)
    bits = np.zeros((B, N, Wd * 32), dtype=np.uint64)
    bits[..., :d] = z
    return (bits.reshape(B, N, Wd, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def shap_apply(x, coal, cells, n0=0, count=None, baseline=0.0, device=True, out=None):
    """The masked images [Nc, B, Cc, H, W] of x [B, Cc, H, W] under coalitions n0 .. n0 + count - 1 (default: to the last): a pixel is x
    when its player is in the coalition, else the baseline (a number or a tensor like x).  device=True: one ppf_shap_apply launch;
    device=False: numpy."""
    if device:
        from . import ops
        return ops.shap_apply(x, coal, cells, n0, count, baseline, out=out)
    x = _host(x, np.float32)
    if x.shape[2] != x.shape[3]:
        raise ValueError(f"shap_apply: H={x.shape[2]} W={x.shape[3]}: square images only")
    qmap, z = _shap_player_maps(x.shape[2], cells), shap_members(coal, cells)
    n0, N = int(n0), z.shape[1]
    Nc = N - n0 if count is None else int(count)
    if n0 < 0 or Nc < 1 or n0 + Nc > N:
        raise ValueError(f"shap_apply: samples {n0} .. {n0 + Nc - 1} outside [0, {N})")
    keep = z[:, n0:n0 + Nc][:, :, qmap].transpose(1, 0, 2, 3)[:, :, None]                          # [Nc, B, 1, H, W]
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    return np.where(keep, x[None], base[None]).astype(np.float32)


def shap_gram(coal, val, v0, cells, device=True):
    """(A int32 [B, d, d], bvec fp64 [B, M, d]) of the regression: A[b, i, j] = the number of samples that hold players i and j;
    bvec[b, m, i] = the fp64 sum over n ascending, over the samples that hold player i only, of (double)val[n, b, m] - (double)v0[b, m],
    from +0.  device=True: one ppf_shap_gram launch; device=False: numpy, sample by sample."""
    if device:
        from . import ops
        return ops.shap_gram(coal, val, v0, cells)
    z, val, v0 = shap_members(coal, cells), _host(val, np.float32), _host(v0, np.float32)
    (B, N, d), M = z.shape, val.shape[2]
    if val.shape != (N, B, M) or v0.shape != (B, M) or not 1 <= M <= 8:
        raise ValueError(f"shap_gram: val must be [{N}, {B}, M] and v0 [{B}, M] with M in [1, 8], got {list(val.shape)} and {list(v0.shape)}")
    zi = z.astype(np.int64)
    A = np.einsum("bni,bnj->bij", zi, zi).astype(np.int32)
    bvec, from_ = np.zeros((B, M, d), dtype=np.float64), v0.astype(np.float64)
    with np.errstate(all="ignore"):
        for n in range(N):                                                                        # ascending: the order is the contract
            term = val[n].astype(np.float64) - from_                                              # [B, M]
            bvec = np.where(z[:, n, None, :], bvec + term[:, :, None], bvec)
    return A, bvec


def shap_solve(A, bvec, v0, v1, cells, grid_cells, device=True):
    """(phi fp64 [B, M, d], cell fp32 [B, M, G], bad int32 [B]): per image A = L L^T, x_m = A^-1 bvec_m, y = A^-1 1 and
    phi_m = x_m - y (sum x_m - delta_m) / sum y with delta_m = (double)v1 - (double)v0, the least-squares attributions that add up to
    delta_m; cell = (float)(phi[player of the cell] / r^2), a player's value shared among its r x r cells.  An image whose A is not positive
    definite has bad = 1 and NaN rows; a row whose bvec or delta is not finite is NaN.  device=True: one ppf_shap_solve launch;
    device=False: numpy's Cholesky, in fp64 too but not bit for bit (the device's error is held to a forward-error bound of it)."""
    if device:
        from . import ops
        return ops.shap_solve(A, bvec, v0, v1, cells, grid_cells)
    s, d, _ = _shap_sizes(cells)
    cmap = _shap_player_maps(None, s, grid_cells)
    A, bvec = _host(A, np.int32).astype(np.float64), _host(bvec, np.float64)
    delta = _host(v1, np.float32).astype(np.float64) - _host(v0, np.float32).astype(np.float64)
    (B, M, _), r = bvec.shape, int(round(int(grid_cells) ** 0.5)) // s
    phi, bad = np.full((B, M, d), np.nan), np.zeros(B, dtype=np.int32)
    with np.errstate(all="ignore"):
        for b in range(B):
            try:
                L = np.linalg.cholesky(A[b])
            except np.linalg.LinAlgError:
                bad[b] = 1
                continue
            y = np.linalg.solve(L.T, np.linalg.solve(L, np.ones(d)))
            for m in range(M):
                if not (np.isfinite(bvec[b, m]).all() and np.isfinite(delta[b, m])):
                    continue
                xm = np.linalg.solve(L.T, np.linalg.solve(L, bvec[b, m]))
                phi[b, m] = xm - y * ((xm.sum() - delta[b, m]) / y.sum())
        return phi, (phi[:, :, cmap] / float(r * r)).astype(np.float32), bad


class Shap(Record):
    """What kernel_shap returns, as device tensors (numpy arrays after cpu()): phi fp64 [B, M, d], the Shapley values of the d = cells^2
    players; cell fp32 [B, M, G], a player's value shared equally among its grid cells; value fp32 [N, B, M], the value of every masked
    image; value_base, value_full fp32 [B, M], the values of the all-baseline image and of x; gram int32 [B, d, d] and bvec fp64
    [B, M, d], the regression's sums; bad int32 [B] (1: the image's system was singular, its rows are NaN); classes int32 [B, M]; coal
    int32 [B, N, Wd], the coalition words.  cells, kind: the settings (kind: what `value` holds, 'prob' or 'logit')."""
    FIELDS = ("phi", "cell", "value", "value_base", "value_full", "gram", "bvec", "bad", "classes", "coal")
    META = dict(cells=int, kind=str)

    def delta(self):
        """sum phi - (value_full - value_base) [B, M] in fp64: the efficiency gap, rounding error alone."""
        wide = (lambda t: t.astype(np.float64)) if self.on_host else (lambda t: t.double())
        return self.phi.sum(-1) - (wide(self.value_full) - wide(self.value_base))


def _shap_check(samples, cells, value, grid_cells):
    s, d, _ = _shap_sizes(cells, samples)
    if value not in SHAP_VALUES:
        raise ValueError(f"kernel_shap: value must be one of {SHAP_VALUES}, got {value!r}")
    if int(samples) < 4 * d:
        raise ValueError(f"kernel_shap: samples={int(samples)} is below 4 * cells^2 = {4 * d}: the regression of {d} players is likely singular")
    side = int(round(int(grid_cells) ** 0.5))
    if side * side != int(grid_cells) or side % s:
        raise ValueError(f"kernel_shap: cells={s} does not divide the grid side {side} (G={int(grid_cells)})")
    return s


def _shap_values(ppnet, imgs, cols, value, batch_size):
    """The values fp32 [R] of the classes cols[j] int32 [R] of imgs [R, C, H, W], per column: 'prob' the class probability of the curves
    (_class_probs), 'logit' the class logit (NaN for a class outside the model's).  The caller holds eval mode and no_grad."""
    if value == "prob":
        return _class_probs(ppnet, imgs, cols, batch_size)
    logits = torch.cat([r.logits for r in forward_groups(ppnet, imgs, batch_size)]).float()
    C, nan = logits.shape[1], torch.full((), float("nan"), dtype=torch.float32, device=logits.device)
    return [torch.where((c >= 0) & (c < C), logits.gather(1, c.clamp(0, C - 1).long()[:, None])[:, 0], nan) for c in cols]


def _shap_from_classes(ppnet, x, cls, samples, cells, value, baseline, seed, image_ids, batch_size, scratch_bytes):
    from . import ops
    B, G = x.shape[0], int(ppnet.num_patches)
    M, N = cls.shape[1], int(samples)
    s = _shap_check(N, cells, value, G)
    coal = ops.shap_coalitions(_image_ids(image_ids, B, x.device), s, N, shap_size_table(s * s), seed)
    # scratch: the masked images of one chunk of samples, samples_per_chunk * B images, never more than scratch_bytes (one sample at least)
    chunk = _chunk_items(N, scratch_bytes, x.numel() * 4)
    cols = [cls[:, m].reshape(1, B).expand(max(chunk, 2), B).reshape(-1).contiguous() for m in range(M)]
    buf = torch.empty((chunk,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    val = torch.empty((N, B, M), dtype=torch.float32, device=x.device)
    ends = torch.empty((2, B, M), dtype=torch.float32, device=x.device)
    bs = int(batch_size or B)
    with ppnet.eval_mode():
        for n0 in range(0, N, chunk):
            n = min(chunk, N - n0)
            imgs = ops.shap_apply(x, coal, s, n0, n, baseline, out=buf[:n]).reshape((n * B,) + tuple(x.shape[1:]))
            # a coalition does not depend on the class: one image serves all M columns
            for m, v in enumerate(_shap_values(ppnet, imgs, [c[:n * B] for c in cols], value, bs)):
                val[n0:n0 + n, :, m] = v.reshape(n, B)
        # the two ends of the game: x itself and the all-baseline image
        blank = baseline if isinstance(baseline, torch.Tensor) else torch.full_like(x, float(baseline))
        for m, v in enumerate(_shap_values(ppnet, torch.cat([x, blank.to(x.dtype)]), [c[:2 * B] for c in cols], value, bs)):
            ends[:, :, m] = v.reshape(2, B)
    v1, v0 = ends[0].contiguous(), ends[1].contiguous()
    A, bvec = ops.shap_gram(coal, val, v0, s)
    phi, cell, bad = ops.shap_solve(A, bvec, v0, v1, s, G)
    return Shap(phi, cell, val, v0, v1, A, bvec, bad, cls, coal, s, value)


@torch.no_grad()
def kernel_shap(ppnet, x, classes=None, top_classes=1, samples=512, cells=7, value="prob", baseline=0.0, seed=0, image_ids=None, batch_size=None,
                scratch_bytes=1 << 30):
    """KernelSHAP attributions of a batch x [B, 3, H, W] (CUDA) for the classes of explain (None: the top `top_classes` of the logits): one
    eval forward and the class pick, one ppf_shap_coalitions launch, then per chunk of samples ppf_shap_apply into the one scratch buffer
    (samples-per-chunk = scratch_bytes // (B * image bytes), at least one) and the model's forward over the chunk in sub-batches of
    `batch_size` images (default B; the images of a chunk are ordered sample, sample-of-the-batch); the forwards of x and of the
    all-baseline image; one ppf_shap_gram and one ppf_shap_solve launch.  samples = N coalitions per image, even and at least 4 * cells^2
    (at N = 2 d about half of the systems tried were singular, at 4 d none); cells = s players per side, which must divide the grid side;
    value: 'prob', the class probability of the curves (ppf_class_prob), or 'logit', the class logit; baseline: what a pixel outside
    the coalition becomes (a number in normalised space or a tensor like x); seed, image_ids [B] (None: 0 .. B-1) key the coalitions, so
    an image's coalitions do not depend on its batch.  Nothing image-sized or d^2-sized passes through the host.  Returns a Shap (device
    tensors; nothing is read back here)."""
    _shap_check(samples, cells, value, ppnet.num_patches)
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("kernel_shap needs a CUDA/HIP batch (no CPU fallback path; shap_coalitions_from_ids / shap_apply / shap_gram / shap_solve "
                           "with device=False are the host referees)")
    x = x.float().contiguous()
    outs = _eval_outputs(ppnet, x)
    cls = _pick_classes(ppnet, outs, classes, top_classes, x.shape[0])
    return _shap_from_classes(ppnet, x, cls, samples, cells, value, baseline, seed, image_ids, batch_size, scratch_bytes)


# ------------------------------------------------------------------------------------------------ spatial alignment: does a cell's activation depend on its pixels?
# Every token of a transformer backbone has attended to every other token before the prototype layer sees it, so a prototype's
# activation at a grid cell need not depend on the pixels of that cell.  The spatial-misalignment benchmark (Sacha et al., AAAI 2024)
# tests it: perturb only the pixels OUTSIDE the prototype's box and follow its activation (PAC, the relative activation change) and
# its peak (PLC, the peak's displacement); next to it, the share of the pixel gradient that falls inside the box.  All of it rests on
# the gradient with respect to the image, which the backbone's backward hands out when the image requires one (backbone.embed_bwd,
# precise._embed_bwd: dcols = dtok W and ppf_col2im_patch_f32).  ppf_grad_box_mass and ppf_pgd_step_box (csrc/alignment.hip) do the
# rest on the device; the numpy forms below (device=False) are the referees.  The reference has no such pass.
def _refuse_pending_gradients(who, ppnet):
    """Raises if a parameter holds a pending gradient: a .grad with a non-zero (or NaN) element.  The all-zero views the flat store
    attaches when it is built (the first forward) hold nothing and do not count.  One fused norm over the attached gradients and one
    read, only when gradients are attached at all."""
    held = [(n, p.grad) for n, p in ppnet.named_parameters() if p.grad is not None]
    if held:
        pending = (torch.stack(torch._foreach_norm([g.detach().float().reshape(-1) for _, g in held])) != 0).cpu().numpy()
        if pending.any():
            first = held[int(np.nonzero(pending)[0][0])][0]
            raise RuntimeError(f"{who}: {int(pending.sum())} parameters already hold a .grad ({first}, ...): its backward accumulates into "
                               "the same buffers; finish the training step and drop the gradients (zero_grad(set_to_none=True)) first")


def _parse_target(who, ppnet, target, B, device, or_none=False):
    """(kind, branch, ids int32 [B, M]) of a target ("logit", classes) or ("proto", "local" | "global", prototypes): branch None for a
    logit; ids [B] or [B, M], host values range-checked against the output's width (_explain_classes), device tensors not read back.
    or_none: None stands for the logits of classes still to be picked, ("logit", None, None)."""
    if target is None and or_none:
        return "logit", None, None
    kind = target[0] if isinstance(target, (tuple, list)) and target else None
    if kind == "logit" and len(target) == 2:
        branch, sel, n_out = None, target[1], ppnet.last_layer.weight.shape[0]
    elif kind == "proto" and len(target) == 3 and target[1] in EXPLAIN_BRANCHES:
        branch, sel = target[1], target[2]
        n_out = ppnet.prototype_vectors.shape[0] if branch == "local" else ppnet.prototype_vectors_global.shape[0]
    else:
        raise ValueError(f'{who}: target must be {"None, " if or_none else ""}("logit", classes) or ("proto", "local" | "global", prototypes)')
    return kind, branch, _explain_classes(sel, B, n_out, device)


def input_gradient(ppnet, x, target):
    """Gradient of a model output with respect to the image: (grad fp32 [B, 3, H, W], value fp32 [B]) of x [B, 3, H, W] (CUDA).
    target = ("logit", classes [B]): value = logits[b, classes[b]]; ("proto", "local" | "global", protos [B]): value = the prototype's
    pooled activation act_max[b, protos[b]] of that branch.  Eval mode (DropPath off), ppnet.precise honoured; the backward of the
    summed values is taken -- samples are independent, so row b is sample b's own gradient.
    A backward accumulates weight gradients into the flat store and attaches .grad as any backward does, so this raises if a
    parameter holds a pending gradient on entry -- a .grad with a non-zero (or NaN) element; the all-zero views the flat store attaches
    when it is built do not count -- since a training step in flight would be corrupted, and sets every .grad back to None on exit."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError("input_gradient needs a CUDA/HIP batch [B, 3, H, W] (no CPU fallback path)")
    _refuse_pending_gradients("input_gradient", ppnet)
    B = x.shape[0]
    _, branch, sel = _parse_target("input_gradient", ppnet, target, B, x.device)
    if sel.shape[1] != 1:
        raise ValueError(f"input_gradient: one target per sample expected, got {tuple(sel.shape)}")
    xg = x.detach().float().contiguous().requires_grad_(True)
    try:
        with ppnet.eval_mode(), torch.enable_grad():
            r = ppnet._branches(xg, want_dist=False)
            out = {None: r.logits, "local": r.act_max_local, "global": r.act_max_global}[branch]
            if out.grad_fn is None:
                raise RuntimeError("input_gradient: the forward recorded no graph for the target")
            value = out.gather(1, sel.long()).reshape(B)
            value.sum().backward()
    finally:
        for p in ppnet.parameters():
            p.grad = None
    return xg.grad, value.detach()


def _boxes_host(peaks_yx, half_size, size):
    y, x = np.asarray(peaks_yx)[..., 0].astype(np.int64), np.asarray(peaks_yx)[..., 1].astype(np.int64)
    return np.stack([np.maximum(y - half_size, 0), np.minimum(y + half_size, size), np.maximum(x - half_size, 0), np.minimum(x + half_size, size)],
                    axis=-1).astype(np.int32)


def _boxes_around(yx, half_size, size):
    """int32 [R, 4] = (y0, y1, x0, x1), half-open: [peak - half_size, peak + half_size) clipped to the image, from peaks yx int32 [R, 2]."""
    y, x = yx[:, 0], yx[:, 1]
    return torch.stack([(y - half_size).clamp(min=0), (y + half_size).clamp(max=size), (x - half_size).clamp(min=0), (x + half_size).clamp(max=size)],
                       dim=1).to(torch.int32).contiguous()


def _proto_peaks(ppnet, outs, protos):
    """The up-sampled peaks (values [R], yx int32 [R, 2]) of the local prototypes protos [B, K] on eval outputs: row r = b * K + j."""
    from . import ops
    B, K = protos.shape
    k = ppnet.reserve_token_nums[0]
    s = int(round(k ** 0.5))
    act = outs["act_full"].reshape(B, -1, k)
    own = torch.gather(act, 1, protos.long()[:, :, None].expand(B, K, k)).reshape(B, K, s, s)
    grid = _grid_on_device(outs["token_attn"], own, k)
    val, yx, _ = ops.act_peak(grid.reshape(B * K, grid.shape[-2], grid.shape[-1]), ppnet.img_size)
    return val, yx


def _proto_ids(who, ppnet, protos, B, device):
    P = ppnet.prototype_vectors.shape[0]
    t = protos if isinstance(protos, torch.Tensor) and protos.is_cuda else torch.as_tensor(np.asarray(protos)).to(device)
    if t.is_floating_point() or t.dim() not in (1, 2) or t.shape[0] != B:
        raise ValueError(f"{who}: protos must be integers [B] or [B, K] for a batch of {B}, got {tuple(t.shape)} {t.dtype}")
    return (t[:, None] if t.dim() == 1 else t).to(torch.int32).contiguous(), P


def prototype_boxes(ppnet, x_outputs, protos, half_size=36):
    """int32 [R, 4] boxes (y0, y1, x0, x1), half-open, of the local prototypes protos [B] or [B, K] (row r = b * K + j): half_size pixels
    to each side of the peak of the prototype's up-sampled activation map, clipped to the image -- the box rule of the consistency
    score (prototype_part_table).  x_outputs: what one eval forward leaves (_eval_outputs: token_attn, act_full).  expand_to_grid of
    the selected maps + one ppf_act_peak launch; stays on the device."""
    protos, _ = _proto_ids("prototype_boxes", ppnet, protos, x_outputs["act_full"].shape[0], x_outputs["act_full"].device)
    _, yx = _proto_peaks(ppnet, x_outputs, protos)
    return _boxes_around(yx, int(half_size), int(ppnet.img_size))


def box_mass_host(g, boxes):
    """The numpy referee of ppf_grad_box_mass: (inside fp64 [R], total fp64 [R], nonfinite int32 [R]) of g [R, C, H, W], boxes [R, 4]."""
    g, boxes = np.asarray(g, dtype=np.float32), np.asarray(boxes)
    R, C, H, W = g.shape
    fin = np.isfinite(g)
    a = np.where(fin, np.abs(g), np.float32(0)).astype(np.float64)
    ys, xs = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    m = (ys >= boxes[:, 0, None, None]) & (ys < boxes[:, 1, None, None]) & (xs >= boxes[:, 2, None, None]) & (xs < boxes[:, 3, None, None])
    return (a * m[:, None]).sum((1, 2, 3)), a.sum((1, 2, 3)), (~fin).sum((1, 2, 3)).astype(np.int32)


def gradient_locality(grad, boxes, device=True):
    """(inside, total, share) fp64 [R] of grad fp32 [R, C, H, W] and boxes int32 [R, 4]: the L1 mass of the gradient inside the box, its
    total, and their ratio (NaN where total == 0); non-finite elements count as 0.  device=True: one ppf_grad_box_mass launch, device
    tensors; device=False: the numpy referee."""
    if not device:
        g = grad.detach().cpu().numpy() if isinstance(grad, torch.Tensor) else grad
        b = boxes.cpu().numpy() if isinstance(boxes, torch.Tensor) else boxes
        inside, total, _ = box_mass_host(g, b)
        with np.errstate(invalid="ignore", divide="ignore"):
            return inside, total, np.where(total == 0, np.nan, inside / np.where(total == 0, 1.0, total))
    from . import ops
    inside, total, _ = ops.grad_box_mass(grad, boxes, want_nonfinite=False)
    return inside, total, torch.where(total == 0, torch.full_like(total, float("nan")), inside / total)


def pgd_step_box(x, x0, g, boxes, alpha, eps, lo, hi, direction, device=True):
    """One projected signed-gradient step outside the boxes, the original pixel inside (ppf_pgd_step_box): per channel c
    x <- min(max(x + direction * alpha_c * sign(g), max(x0 - eps_c, lo_c)), min(x0 + eps_c, hi_c)), sign(+-0) = sign(NaN) = 0.
    device=True: in place on the CUDA tensor x, returns it.  device=False: the numpy referee, returns a new array (fp32 throughout,
    every operation rounded once; for finite x and x0 bit-identical to the kernel)."""
    if device:
        from . import ops
        return ops.pgd_step_box(x, x0, g, boxes, alpha, eps, lo, hi, direction)
    if direction not in (1, -1):
        raise ValueError(f"pgd_step_box: direction must be +1 or -1, got {direction!r}")
    x, x0, g, boxes = (np.asarray(a) for a in (x, x0, g, boxes))
    R, C, H, W = x.shape
    a, e, l, h = (np.asarray(v, dtype=np.float32).reshape(1, C, 1, 1) for v in (alpha, eps, lo, hi))
    x, x0, g = x.astype(np.float32), x0.astype(np.float32), g.astype(np.float32)
    with np.errstate(invalid="ignore"):
        sign = (g > 0).astype(np.float32) - (g < 0).astype(np.float32)
    moved = x + (np.float32(direction) * a) * sign
    out = np.minimum(np.maximum(moved, np.maximum(x0 - e, l)), np.minimum(x0 + e, h)).astype(np.float32)
    ys, xs = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    m = (ys >= boxes[:, 0, None, None]) & (ys < boxes[:, 1, None, None]) & (xs >= boxes[:, 2, None, None]) & (xs < boxes[:, 3, None, None])
    return np.where(m[:, None], x0, out)


def attack_bounds(eps, alpha, steps, device=None, mean=None, std=None):
    """The per-channel constants of the attack in normalised space, fp32 [3] each: (alpha, eps, lo, hi).  eps and alpha are in pixel
    units ([0, 1] images) and are divided by the data-set std per channel; alpha defaults to 2.5 * eps / steps; lo / hi are the
    normalised values of 0 and 1.  device None: numpy arrays."""
    from .data import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
    mean = np.asarray(IMAGENET_DEFAULT_MEAN if mean is None else mean, dtype=np.float64)
    std = np.asarray(IMAGENET_DEFAULT_STD if std is None else std, dtype=np.float64)
    if not (eps >= 0) or steps < 1:
        raise ValueError(f"misalignment_attack: eps={eps} must be >= 0 and steps={steps} >= 1")
    alpha = 2.5 * eps / steps if alpha is None else alpha
    out = [(v).astype(np.float32) for v in (alpha / std, eps / std, (0.0 - mean) / std, (1.0 - mean) / std)]
    return out if device is None else [torch.from_numpy(v).to(device) for v in out]


def misalignment_attack(ppnet, x, protos, boxes, steps=10, eps=8 / 255, alpha=None, seed=None, return_images=False):
    """The spatial-misalignment attack on local prototypes: `steps` signed-gradient steps that LOWER the prototype's activation, changing
    only pixels outside its box, within eps (pixel units, L-inf) of the image and inside the valid pixel range.
    x [B, 3, H, W] (CUDA, normalised); protos [B] or [B, K]; boxes int32 [R, 4] with row r = b * K + j (prototype_boxes).  Every row is
    an attack of its own on a copy of its image.  seed None: start at the image; else a uniform start inside the eps-ball keyed by it.
    Per step one input_gradient (a forward and a backward of R images) and one ppf_pgd_step_box launch with dir = -1.
    Returns a dict of device tensors [R]: act_before, act_after, pac = (a0 - aT) / |a0|, peak_before / peak_after int32 [R, 2] (y, x of
    the up-sampled peak), plc = their Chebyshev distance in pixels (int32), left_box (bool: the peak after lies outside the box),
    boxes, protos; with return_images also images [R, 3, H, W]."""
    from . import ops
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError("misalignment_attack needs a CUDA/HIP batch [B, 3, H, W] (no CPU fallback path)")
    B = x.shape[0]
    protos, _ = _proto_ids("misalignment_attack", ppnet, protos, B, x.device)
    K = protos.shape[1]
    R = B * K
    ops._dev_tensor("misalignment_attack", "boxes", boxes, torch.int32, (R, 4), x.device)
    a3, e3, lo3, hi3 = attack_bounds(eps, alpha, steps, x.device)
    x0 = x.detach().float().repeat_interleave(K, dim=0).contiguous()
    rows = protos.reshape(R)
    xr = x0.clone()
    if seed is not None:
        gen = torch.Generator(device=x.device).manual_seed(int(seed))
        xr += (torch.rand(xr.shape, generator=gen, device=x.device) * 2 - 1) * e3.reshape(1, -1, 1, 1)
        ops.pgd_step_box(xr, x0, ops.zeros(xr.shape, torch.float32, x.device), boxes, a3, e3, lo3, hi3, -1)       # a zero gradient: projection only
    def measure(images):
        with torch.no_grad():
            outs = _eval_outputs(ppnet, images)
            return outs["act_max"].gather(1, rows.long()[:, None]).reshape(R), _proto_peaks(ppnet, outs, rows[:, None])[1]
    act0, yx0 = measure(x0)
    for _ in range(int(steps)):
        g, _ = input_gradient(ppnet, xr, ("proto", "local", rows))
        ops.pgd_step_box(xr, x0, g, boxes, a3, e3, lo3, hi3, -1)
    act1, yx1 = measure(xr)
    plc = (yx1 - yx0).abs().max(dim=1)[0].to(torch.int32)
    y, xx = yx1[:, 0], yx1[:, 1]
    left = ~((y >= boxes[:, 0]) & (y < boxes[:, 1]) & (xx >= boxes[:, 2]) & (xx < boxes[:, 3]))
    out = dict(act_before=act0, act_after=act1, pac=(act0.double() - act1.double()) / act0.double().abs(), peak_before=yx0, peak_after=yx1, plc=plc,
               left_box=left, boxes=boxes, protos=rows)
    if return_images:
        out["images"] = xr
    return out


ALIGNMENT_STATS = ("share", "area", "pac", "plc", "left_box")


def alignment_rows(ppnet, x, protos_per_image=3, half_size=36, attack=True, attack_steps=10, eps=8 / 255, alpha=None):
    """The spatial-alignment measurements of one batch x [B, 3, H, W]: per image the predicted class's local prototypes ranked by
    pooled activation (larger first, equal ones by smaller id), the first protos_per_image of them; one row per (image, prototype)
    pair, row r = b * K + j.  Returns (protos int32 [R], stats fp64 [R, 5] on the device, columns ALIGNMENT_STATS: the gradient's share
    inside the box (NaN for a zero gradient), box area / image area, PAC, PLC, peak left the box (0 / 1); the last three NaN without
    the attack)."""
    with torch.no_grad():
        outs = _eval_outputs(ppnet, x)
    B, ppc = x.shape[0], int(ppnet.num_prototypes_per_class)
    K = min(int(protos_per_image), ppc)                    # this pass's clamp: min(k, ppc), at most ppc and no lower bound
    protos = select_prototypes("top", ppc, outs["logits"].argmax(1), outs["act_max"], K).to(torch.int32).contiguous()
    boxes = prototype_boxes(ppnet, outs, protos, half_size)
    rows = protos.reshape(-1)
    grad, _ = input_gradient(ppnet, x.repeat_interleave(K, dim=0).contiguous(), ("proto", "local", rows))
    _, _, share = gradient_locality(grad, boxes)
    b64 = boxes.double()
    area = (b64[:, 1] - b64[:, 0]) * (b64[:, 3] - b64[:, 2]) / float(x.shape[-1] * x.shape[-2])
    nan = torch.full_like(share, float("nan"))
    pac = plc = left = nan
    if attack:
        r = misalignment_attack(ppnet, x, protos, boxes, steps=attack_steps, eps=eps, alpha=alpha)
        pac, plc, left = r["pac"], r["plc"].double(), r["left_box"].double()
    return rows, torch.stack([share, area, pac, plc, left], dim=1)


def alignment_summary(protos, stats):
    """The report of spatial_alignment from all rows (device tensors protos [N], stats fp64 [N, 5]): fp64 sums on the device -- overall one
    reduction over the rows in pair order, per prototype a one-hot product (no atomics: the same rows give the same bits) -- and ONE
    read-back.  NaN entries (a zero gradient; no attack) are left out of their mean and counted out of its denominator."""
    ok = ~torch.isnan(stats)
    val = torch.where(ok, stats, torch.zeros_like(stats))
    uniq, inv = torch.unique(protos.long(), return_inverse=True)                            # the prototypes that occurred, ascending
    P, n = int(uniq.shape[0]), len(ALIGNMENT_STATS)
    onehot = torch.nn.functional.one_hot(inv, P).double()                                    # [N, P]
    packed = torch.cat([val.sum(0, keepdim=True), ok.double().sum(0, keepdim=True), onehot.t() @ val, onehot.t() @ ok.double(),
                        uniq.double()[:, None].expand(P, n)]).cpu().numpy()

    def means(s, c):
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.where(c > 0, s / np.where(c > 0, c, 1.0), np.nan)
        d = {f"mean_{k}": m[..., i] for i, k in enumerate(ALIGNMENT_STATS)}
        with np.errstate(invalid="ignore", divide="ignore"):
            d["share_over_area"] = d["mean_share"] / d["mean_area"]
        d["rows"] = c[..., 1]                                                                # the area is never NaN: every row counts
        return d
    overall = {k: float(v) for k, v in means(packed[0], packed[1]).items()}
    per = means(packed[2:2 + P], packed[2 + P:2 + 2 * P])
    ids = packed[2 + 2 * P:, 0].astype(np.int64)
    return dict(rows=int(overall.pop("rows")), overall=overall,
                per_prototype={int(p): {k: (int(v[j]) if k == "rows" else float(v[j])) for k, v in per.items()} for j, p in enumerate(ids)})


def spatial_alignment(ppnet, loader, protos_per_image=3, half_size=36, attack=True, attack_steps=10, eps=8 / 255, alpha=None, max_images=0,
                      pass_images=16):
    """The spatial-alignment test over a data set.  loader yields (x, ...); its images are regrouped into passes of pass_images images
    (tooling.regroup), so the result does not depend on the loader's batch size, and each pass is measured by alignment_rows.  The rows
    stay on the device; their fp64 means are taken once at the end (alignment_summary) and read back once.  Returns dict(images, rows,
    overall: mean_share, mean_area (box area / image area, the share a spatially blind gradient would reach), share_over_area, mean_pac,
    mean_plc, mean_left_box; per_prototype: the same per prototype id that occurred, with its row count)."""
    ids, stats, images = [], [], 0
    for x, in regroup(((x.float(),) for x, in take_images(((b[0],) for b in loader), int(max_images))), int(pass_images)):
        x = x if x.is_cuda else x.cuda()
        p, s = alignment_rows(ppnet, x, protos_per_image, half_size, attack, attack_steps, eps, alpha)
        ids.append(p); stats.append(s)
        images += x.shape[0]
    if not images:
        raise ValueError("spatial_alignment: the loader gave no image")
    out = alignment_summary(torch.cat(ids), torch.cat(stats))
    out["images"] = images
    return out


# ------------------------------------------------------------------------------------------------ integrated gradients: the gradient baseline of the faithfulness test
# Integrated gradients (Sundararajan et al., "Axiomatic Attribution for Deep Networks", 2017): attribution = (x - baseline) times the
# gradient averaged along the straight path from the baseline to x.  No noise level to pick, and a property that can be checked: the
# attributions of an image sum to f(x) - f(baseline) (completeness) -- for a model that is continuous along the path; the token
# reservation's top-k is not, so here the sum rule holds between its jumps and the gap (IntegratedGradients.delta) is reported, not
# gated.  One step with the end-point rule is plain gradient x input.  The gradients are input_gradient's; between the model's passes
# ppf_ig_point makes the path point, ppf_ig_accumulate adds the weighted gradient and ppf_ig_finish multiplies by (x - baseline) and sums
# per grid cell (csrc/ig.hip): no image-sized tensor passes through the host.  The numpy forms below (device=False) are the referees,
# bit for bit (the contract is in include/ppf_hip.h).  The reference has no such pass.
GRADIENT_ORDERS = ("ig",)               # opt-in order of faithfulness_curves / faithfulness: the cells ranked by their integrated gradients
IG_RULES = ("midpoint", "trapezoid", "endpoint")
IG_DEFAULTS = dict(steps=32, rule="midpoint")


def ig_rule(steps, rule="midpoint"):
    """(alphas fp32 [n], weights fp32 [n]) of a quadrature of the path integral over [0, 1] with S = steps intervals, computed in fp64
    and cast once.  'midpoint': alphas (s + 0.5) / S, weights 1 / S; 'trapezoid': alphas s / S for s = 0 .. S, weights 1 / (2 S) at both
    ends and 1 / S inside; 'endpoint': alphas (s + 1) / S, weights 1 / S -- with S = 1 gradient x (x - baseline)."""
    S = int(steps)
    if S < 1 or S != steps:
        raise ValueError(f"ig_rule: steps={steps!r} must be an integer >= 1")
    if rule == "midpoint":
        a, w = (np.arange(S, dtype=np.float64) + 0.5) / S, np.full(S, 1.0 / S)
    elif rule == "trapezoid":
        a, w = np.arange(S + 1, dtype=np.float64) / S, np.full(S + 1, 1.0 / S)
        w[0] = w[-1] = 1.0 / (2 * S)
    elif rule == "endpoint":
        a, w = (np.arange(S, dtype=np.float64) + 1.0) / S, np.full(S, 1.0 / S)
    else:
        raise ValueError(f"ig_rule: rule must be one of {IG_RULES}, got {rule!r}")
    return a.astype(np.float32), w.astype(np.float32)


def ig_point(x, alpha, baseline=0.0, device=True, out=None):
    """The path point baseline + alpha * (x - baseline), fp32, every operation rounded once.  baseline: a number or a tensor like x.
    device=True: one ppf_ig_point launch (out: a buffer like x to write into); device=False: numpy."""
    if device:
        from . import ops
        return ops.ig_point(x, alpha, baseline, out=out)
    x = _host(x, np.float32)
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    with np.errstate(all="ignore"):
        return (base + np.float32(alpha) * (x - base)).astype(np.float32)


def ig_accumulate(g, w, acc, first=False, device=True):
    """acc = w * g (first) or acc + w * g, fp32, every operation rounded once; acc has g's shape.  device=True: ppf_ig_accumulate in place
    on the CUDA tensor acc (its rows may lie apart: ops.ig_accumulate), returns it; device=False: numpy, returns a new array (acc is
    not read when first is set and may be None)."""
    if device:
        from . import ops
        return ops.ig_accumulate(g, w, acc, first)
    g = _host(g, np.float32)
    with np.errstate(all="ignore"):
        wg = (np.float32(w) * g).astype(np.float32)
        return wg if first else (_host(acc, np.float32) + wg).astype(np.float32)


def ig_finish(acc, x, baseline, patch, device=True):
    """(attr fp32 [B, M, C, H, W], cell64 fp64 [B, M, G]) of acc fp32 [B, M, C, H, W] and x [B, C, H, W]: attr = (x - baseline) * acc in
    fp32, each operation rounded once; cell64 = the fp64 sum of attr over the channels and the pixels of every patch x patch cell,
    G = (H / patch) * (W / patch), cells row-major.  device=True: one ppf_ig_finish launch; device=False: numpy (np.sum in fp64)."""
    if device:
        from . import ops
        return ops.ig_finish(acc, x, baseline, patch)
    acc, x, patch = _host(acc, np.float32), _host(x, np.float32), int(patch)
    B, M, C, H, W = acc.shape
    if patch < 1 or H % patch or W % patch or not 1 <= M <= 8 or (H // patch) * (W // patch) > 1024:
        raise ValueError(f"ig_finish: patch={patch} must divide H={H} and W={W}, M={M} lie in [1, 8] and the grid hold at most 1024 cells")
    base = np.broadcast_to(_host(baseline, np.float32), x.shape)
    with np.errstate(all="ignore"):
        attr = ((x - base)[:, None] * acc).astype(np.float32)
        cells = attr.reshape(B, M, C, H // patch, patch, W // patch, patch).astype(np.float64)
        return attr, np.sum(cells, axis=(2, 4, 6)).reshape(B, M, -1)


class IntegratedGradients(Record):
    """What integrated_gradients returns, as device tensors (numpy arrays after cpu()): attribution fp32 [B, M, 3, H, W]; cell fp32
    [B, M, G] = the attribution summed over each grid cell (the fp64 sums rounded once); total fp64 [B, M] = the fp64 cell sums added up,
    the whole attribution of the image; value, value_base fp32 [B, M] = the target at x and at the baseline image; targets int32 [B, M];
    alphas, weights fp32 [n] of the rule.  target = ("logit",) or ("proto", branch); steps, rule."""
    FIELDS = ("attribution", "cell", "total", "value", "value_base", "targets", "alphas", "weights")
    META = dict(target=tuple, steps=int, rule=str)

    def delta(self):
        """The completeness gap fp64 [B, M]: total - (value - value_base), the fp32 values widened first."""
        if self.on_host:
            return self.total - (self.value.astype(np.float64) - self.value_base.astype(np.float64))
        return self.total - (self.value.double() - self.value_base.double())


def _ig_pass(ppnet, x, outs, kind, branch, ids, steps, rule, baseline, batch_size):
    """integrated_gradients after the forward of x (outs) and the pick of the targets ids int32 [B, M]."""
    from . import ops
    B, M = ids.shape
    if not 1 <= M <= 8:
        raise ValueError(f"integrated_gradients: M={M} targets per image outside [1, 8] (ppf_ig_finish's and ppf_cell_order's limit)")
    G = int(ppnet.num_patches)
    side = int(round(G ** 0.5))
    if side * side != G or x.shape[2] % side or x.shape[2] != x.shape[3]:
        raise ValueError(f"integrated_gradients: a square image and a square grid whose side divides it expected, got {tuple(x.shape)} and G={G}")
    alphas, weights = ig_rule(steps, rule)
    if isinstance(baseline, torch.Tensor):
        baseline = baseline.to(device=x.device, dtype=torch.float32).expand_as(x).contiguous()
    gather = ids.clamp(min=0).long()                                                              # a row whose class could not be picked (-1) follows class 0
    out_of = {None: "logits", "local": "act_max", "global": "act_max_global"}[branch]
    value = outs[out_of].float().gather(1, gather)
    buf = ops.ig_point(x, 0.0, baseline)                                                          # the baseline image, by the kernel that makes every path point
    value_base = _eval_outputs(ppnet, buf)[out_of].float().gather(1, gather)
    acc = torch.empty((B, M) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    bs = int(batch_size or B)
    cols = [gather[:, m].to(torch.int32) for m in range(M)]
    for s, (a, w) in enumerate(zip(alphas.tolist(), weights.tolist())):                           # ascending: the order of the sum is the contract
        ops.ig_point(x, a, baseline, out=buf)
        for m in range(M):
            for b0 in range(0, B, bs):
                sel = cols[m][b0:b0 + bs]
                g, _ = input_gradient(ppnet, buf[b0:b0 + bs], (kind, sel) if branch is None else (kind, branch, sel))
                ops.ig_accumulate(g, w, acc[b0:b0 + bs, m], first=s == 0)
    attr, cell64 = ops.ig_finish(acc, x, baseline, x.shape[2] // side)
    dev = x.device
    return IntegratedGradients(attr, cell64.float(), cell64.sum(-1), value, value_base, ids, torch.from_numpy(alphas).to(dev), torch.from_numpy(weights).to(dev),
                               (kind,) if branch is None else (kind, branch), steps, rule)


def integrated_gradients(ppnet, x, target=None, top_classes=1, steps=32, rule="midpoint", baseline=0.0, batch_size=None):
    """Integrated gradients of a batch x [B, 3, H, W] (CUDA).  target None: the logits of the top `top_classes` classes, picked as
    explain picks them; ("logit", classes) or ("proto", "local" | "global", prototypes): ids [B] or [B, M], M <= 8, validated as
    input_gradient validates them.  baseline: the path's start, a number in normalised space (0 = the data-set mean colour) or a tensor
    like x.  steps, rule: the quadrature (ig_rule); steps=1 with rule='endpoint' is gradient x (x - baseline).
    One eval forward of x (the class pick and `value`), one of the baseline image (ppf_ig_point at alpha 0: `value_base`), then per step
    in ascending order one ppf_ig_point launch into the one [B, 3, H, W] buffer and, per target column m and consecutive group of
    batch_size samples (default B), one input_gradient call and one ppf_ig_accumulate into column m; one ppf_ig_finish at the end.  The
    grouping depends on batch_size alone, so a result repeats bit for bit.  input_gradient's guard holds: pending parameter gradients
    are refused and none are left behind; ppnet.precise is honoured; the training mode is left as found.
    Returns an IntegratedGradients (device tensors; nothing is read back here)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError("integrated_gradients needs a CUDA/HIP batch [B, 3, H, W] (no CPU fallback path; ig_point / ig_accumulate / ig_finish with "
                           "device=False are the host referees)")
    ig_rule(steps, rule)                                                                          # a bad rule is refused before anything runs
    _refuse_pending_gradients("integrated_gradients", ppnet)
    x = x.detach().float().contiguous()
    kind, branch, ids = _parse_target("integrated_gradients", ppnet, target, x.shape[0], x.device, or_none=True)
    M = int(top_classes) if ids is None else ids.shape[1]
    if not 1 <= M <= 8:
        raise ValueError(f"integrated_gradients: M={M} targets per image outside [1, 8] (ppf_ig_finish's and ppf_cell_order's limit)")
    with torch.no_grad():
        outs = _eval_outputs(ppnet, x)
        if ids is None:
            ids = _pick_classes(ppnet, outs, None, top_classes, x.shape[0])
        return _ig_pass(ppnet, x, outs, kind, branch, ids, steps, rule, baseline, batch_size)


# ------------------------------------------------------------------------------------------------ "this looks like that, because ...": colour, texture or shape?
# Two patches a human finds alike can be far apart for the model, and the reverse; an overlay does not show which.  Nauta et al., "This
# Looks Like That, Because ... Explaining Prototypes for Interpretable Image Recognition" (2021), answer by perturbation: suppress one
# visual characteristic of the image -- hue, saturation, contrast, texture or shape --, run the model again, and measure how far the
# prototype's similarity at the same patch falls.  That is a local importance per (image, prototype, characteristic); weighted over a
# prototype's own-class images it is a global one per prototype.  Hue, saturation and contrast are one 3 x 3 colour transform
# (ppf_color_affine; contrast pivots on the image's mean luma, ppf_gray_sum + ppf_contrast_offset), texture is a joint bilateral filter
# guided by the 8-bit luma (ppf_bilateral: edge-preserving, so contours survive), shape a smooth integer warp (ppf_warp_nodes,
# ppf_warp_apply); ppf_because_score reads the perturbed forward (csrc/because.hip).  The arithmetic is a written contract
# (include/ppf_hip.h): the numpy forms below (device=False) are the referees, bit for bit.  The reference has no such pass.
CHARACTERISTICS = ("hue", "saturation", "contrast", "texture", "shape")
LUMA_WEIGHTS = (0.299, 0.587, 0.114)
_RGB_TO_YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))
# The strengths are choices, not tuned values: nobody has run this on a trained checkpoint.  hue: the turn of the IQ plane as a fraction
# of a full turn; saturation / contrast: the factor that is left (0 = none); texture: window radius and the two Gaussian widths (pixels;
# 8-bit luma steps); shape: grid cells per side and the largest node displacement in pixels.
BECAUSE_DEFAULTS = dict(hue=0.5, saturation=0.0, contrast=0.25, radius=4, sigma_space=3.0, sigma_range=25.0, cells=4, amplitude=6.0, mean=None, std=None)


def because_params(params=None):
    """BECAUSE_DEFAULTS overridden by `params`, checked; mean / std default to the data set's normalisation (ImageNet's)."""
    from .data import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
    unknown = set(params or {}) - set(BECAUSE_DEFAULTS)
    if unknown:
        raise ValueError(f"because: unknown parameters {sorted(unknown)} (known: {sorted(BECAUSE_DEFAULTS)})")
    p = {**BECAUSE_DEFAULTS, **(params or {})}
    p["mean"] = np.asarray(IMAGENET_DEFAULT_MEAN if p["mean"] is None else p["mean"], dtype=np.float32).reshape(3)
    p["std"] = np.asarray(IMAGENET_DEFAULT_STD if p["std"] is None else p["std"], dtype=np.float32).reshape(3)
    p["radius"], p["cells"] = int(p["radius"]), int(p["cells"])
    if not 1 <= p["radius"] <= 8 or not 1 <= p["cells"] <= 16:
        raise ValueError(f"because: radius={p['radius']} outside [1, 8] or cells={p['cells']} outside [1, 16]")
    if not (p["sigma_space"] > 0 and p["sigma_range"] > 0 and 0 <= p["amplitude"] <= 128 and (p["std"] > 0).all()):
        raise ValueError("because: sigma_space and sigma_range must be > 0, amplitude in [0, 128] pixels, std > 0")
    return p


def saturation_matrix(f):
    """fp32 [3, 3]: f I + (1 - f) [w; w; w], formed in fp64 and rounded once.  f = 0: three equal rows, the grey image."""
    return (float(f) * np.eye(3) + (1.0 - float(f)) * np.tile(np.asarray(LUMA_WEIGHTS, dtype=np.float64), (3, 1))).astype(np.float32)


def hue_matrix(theta):
    """fp32 [3, 3]: T^-1 R(theta) T with T = RGB -> YIQ and R the rotation of the IQ plane, formed in fp64 and rounded once.  The first
    row of T is the luma, which the turn keeps; colours that leave [0, 1] are clamped by the transform."""
    t = np.asarray(_RGB_TO_YIQ, dtype=np.float64)
    c, s = np.cos(float(theta)), np.sin(float(theta))
    return (np.linalg.inv(t) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]) @ t).astype(np.float32)


def contrast_matrix(f):
    """fp32 [3, 3]: f I; the pivot (1 - f) * mean luma is the per-image offset (contrast_offset)."""
    return (float(f) * np.eye(3)).astype(np.float32)


def bilateral_tables(radius, sigma_space, sigma_range):
    """(ws fp32 [(2r + 1), (2r + 1)], wr fp32 [256]): exp(-(dy^2 + dx^2) / (2 sigma_space^2)) and exp(-d^2 / (2 sigma_range^2)) over the
    8-bit luma difference d, in fp64, rounded once."""
    r = int(radius)
    d = np.arange(-r, r + 1, dtype=np.float64)
    ws = np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(sigma_space) ** 2))
    wr = np.exp(-np.arange(256, dtype=np.float64) ** 2 / (2.0 * float(sigma_range) ** 2))
    return ws.astype(np.float32), wr.astype(np.float32)


def _norm3(mean, std):
    return np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1), np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)


def _clamp01(v):
    return np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)       # NaN -> 0, as the kernels


def _denorm(x, mean, std):
    """clamp(fl(fl(x * std) + mean)): the de-normalised pixel of the contract."""
    m, s = _norm3(mean, std)
    with np.errstate(all="ignore"):
        return _clamp01((_host(x, np.float32) * s).astype(np.float32) + m)


def _renorm(u, mean, std):
    m, s = _norm3(mean, std)
    with np.errstate(all="ignore"):
        return ((_clamp01(u) - m).astype(np.float32) / s).astype(np.float32)


def _luma_q8(v):
    """int32 [B, H, W]: the 8-bit luma of clamped pixels v [B, 3, H, W], operation for operation as the contract."""
    w = [np.float32(a) for a in LUMA_WEIGHTS]
    y = ((w[0] * v[:, 0]).astype(np.float32) + (w[1] * v[:, 1]).astype(np.float32)).astype(np.float32) + (w[2] * v[:, 2]).astype(np.float32)
    q = np.floor((np.float32(255) * y).astype(np.float32) + np.float32(0.5)).astype(np.int32)
    return np.clip(q, 0, 255)


def color_affine(x, matrix, mean, std, offset=None, device=True, out=None):
    """The 3 x 3 colour transform of x [B, 3, H, W] in de-normalised space (the contract is ppf_color_affine's, include/ppf_hip.h): matrix
    [3, 3] on the host, offset [B, 3] optional.  device=True: one launch on CUDA tensors; device=False: the numpy referee."""
    if device:
        from . import ops
        return ops.color_affine(x, matrix, mean, std, offset, out)
    v, M = _denorm(x, mean, std), np.asarray(matrix, dtype=np.float32).reshape(3, 3)
    with np.errstate(all="ignore"):
        u = np.stack([((M[k, 0] * v[:, 0]).astype(np.float32) + (M[k, 1] * v[:, 1]).astype(np.float32)).astype(np.float32)
                      + (M[k, 2] * v[:, 2]).astype(np.float32) for k in range(3)], axis=1).astype(np.float32)
        if offset is not None:
            u = (u + _host(offset, np.float32).reshape(-1, 3, 1, 1)).astype(np.float32)
    return _renorm(u, mean, std)


def gray_sum(x, mean, std, device=True):
    """int32 [B]: the integer sum of the 8-bit luma over each image (ppf_gray_sum)."""
    if device:
        from . import ops
        return ops.gray_sum(x, mean, std)
    return _luma_q8(_denorm(x, mean, std)).sum(axis=(1, 2), dtype=np.int64).astype(np.int32)


def contrast_offset(total, size, f, device=True):
    """fp32 [B, 3]: fl(fl32(1 - f) * fl(fl(sum / (H W)) / 255)) in every channel, from gray_sum's sums (ppf_contrast_offset); size = (H, W).
    1 - f is formed in fp64 and rounded once."""
    g = np.float32(1.0 - float(f))
    if device:
        from . import ops
        return ops.contrast_offset(total, size, float(g))
    m = (_host(total, np.int32).astype(np.float32) / np.float32(int(size[0]) * int(size[1]))).astype(np.float32) / np.float32(255)
    return np.repeat((g * m.astype(np.float32)).astype(np.float32)[:, None], 3, axis=1)


def bilateral(x, ws, wr, mean, std, device=True, out=None):
    """The joint bilateral filter of x [B, 3, H, W] guided by the 8-bit luma (the contract is ppf_bilateral's): ws [(2r + 1), (2r + 1)]
    spatial and wr [256] range weights; taps in row-major window order, those outside the image skipped.  device=False: numpy."""
    ws = np.asarray(ws, dtype=np.float32)
    D = int(round(ws.size ** 0.5))
    r = (D - 1) // 2
    if D * D != ws.size or D != 2 * r + 1 or not 1 <= r <= 8:
        raise ValueError(f"bilateral: ws must hold (2r + 1)^2 weights with 1 <= r <= 8, got {ws.size}")
    ws, wr = ws.reshape(D, D), np.asarray(wr, dtype=np.float32).reshape(256)
    if device:
        from . import ops
        return ops.bilateral(x, ws, wr, r, mean, std, out)
    v = _denorm(x, mean, std)
    B, _, H, W = v.shape
    q = _luma_q8(v)
    vp = np.pad(v, ((0, 0), (0, 0), (r, r), (r, r)))
    qp = np.pad(q, ((0, 0), (r, r), (r, r)), constant_values=-1)
    sw, s = np.zeros((B, 1, H, W), dtype=np.float32), np.zeros((B, 3, H, W), dtype=np.float32)
    for dy in range(D):
        for dx in range(D):
            qq = qp[:, dy:dy + H, dx:dx + W]
            w = np.where(qq >= 0, (ws[dy, dx] * wr[np.minimum(np.abs(q - qq), 255)]).astype(np.float32), np.float32(0))[:, None]
            sw = (sw + w).astype(np.float32)                      # a skipped tap adds an exact zero to both sums
            s = (s + (w * vp[:, :, dy:dy + H, dx:dx + W]).astype(np.float32)).astype(np.float32)
    with np.errstate(all="ignore"):
        return _renorm((s / sw).astype(np.float32), mean, std)


def _warp_sizes(size, cells, amp256):
    H, s, A = int(size), int(cells), int(amp256)
    c = -(-H // max(s, 1))
    if not 1 <= s <= 16 or not 0 <= A <= 1 << 15 or H < 1 or c > 2048 or c * c * max(A, 1) > 2 ** 31 - 1:
        raise ValueError(f"warp: cells={s} outside [1, 16], amplitude {A}/256 outside [0, 2^15/256] or c={c}: c <= 2048, c^2 * amplitude <= 2^31 - 1")
    return H, s, c, A


def warp_amplitude(pixels):
    """The node amplitude in 1/256 pixel units."""
    return int(round(float(pixels) * 256))


def warp_nodes_from_ids(image_ids, cells, amp256, seed=0, device=True):
    """int32 [B, (cells + 1)^2, 2]: the displacements (dy, dx) of the warp's nodes in 1/256 pixel, uniform in [-amp256, amp256]: a function
    of (seed, image id, node) alone (ppf_warp_nodes).  device=False: the numpy Philox."""
    s, A = int(cells), int(amp256)
    if not 1 <= s <= 16 or not 0 <= A <= 1 << 15:
        raise ValueError(f"warp: cells={s} outside [1, 16] or amplitude {A}/256 outside [0, 2^15/256]")
    if device:
        from . import ops
        ids = torch.as_tensor(image_ids)
        return ops.warp_nodes(ids.to(device=ids.device if ids.is_cuda else "cuda", dtype=torch.int64).contiguous(), s, A, seed)
    ids = _host(image_ids, np.int64).reshape(-1).astype(np.uint64)
    B, Q, sd = ids.shape[0], (s + 1) ** 2, int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.empty((B, Q, 4), dtype=np.uint64)
    ctr[..., 0], ctr[..., 1] = np.arange(Q, dtype=np.uint64)[None, :], np.uint64(0x80000000)
    ctr[..., 2], ctr[..., 3] = (ids & np.uint64(0xFFFFFFFF))[:, None], (ids >> np.uint64(32))[:, None]
    w = (philox4x32_10(ctr, np.array([sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint64))[..., :2] >> np.uint32(8)).astype(np.uint64)
    return (((w * np.uint64(2 * A + 1)) >> np.uint64(24)).astype(np.int64) - A).astype(np.int32)


def warp_apply(x, nodes, cells, amp256, device=True, out=None):
    """x [B, Cc, H, H] resampled under the smooth integer warp of the node table (the contract is ppf_warp_apply's): the displacement of a
    pixel is the bilinear interpolation of its four nodes in integers, the blend has weights n / 256 and skips zero weights, so amplitude
    0 is the identity bit for bit.  device=False: numpy."""
    if device:
        from . import ops
        return ops.warp_apply(x, nodes, cells, amp256, out)
    x, nd = _host(x, np.float32), _host(nodes, np.int64)
    B, Cc, H, W = x.shape
    if H != W:
        raise ValueError(f"warp_apply: H={H} W={W}: square images only")
    H, s, c, A = _warp_sizes(H, cells, amp256)
    L = s + 1
    nd = np.clip(nd.reshape(B, L, L, 2), -A, A)
    p = np.arange(H)
    i, ry = p // c, p % c
    I, J, RY, RX = i[:, None], i[None, :], ry[:, None], ry[None, :]
    D = ((c - RY) * (c - RX))[None, :, :, None] * nd[:, I, J] + ((c - RY) * RX)[None, :, :, None] * nd[:, I, J + 1] \
        + (RY * (c - RX))[None, :, :, None] * nd[:, I + 1, J] + (RY * RX)[None, :, :, None] * nd[:, I + 1, J + 1]
    d = D // (c * c)                                                                              # floor division, [B, H, W, 2]
    Y = np.clip(256 * p[None, :, None] + d[..., 0], 0, 256 * (H - 1))
    X = np.clip(256 * p[None, None, :] + d[..., 1], 0, 256 * (W - 1))
    sy, fy, sx, fx = Y >> 8, Y & 255, X >> 8, X & 255
    sy1, sx1 = np.minimum(sy + 1, H - 1), np.minimum(sx + 1, W - 1)
    bi = np.arange(B)[:, None, None, None]
    ci = np.arange(Cc)[None, :, None, None]
    g = lambda yy, xx: x[bi, ci, yy[:, None], xx[:, None]]
    a, e = (fx.astype(np.float32) / np.float32(256))[:, None], (fy.astype(np.float32) / np.float32(256))[:, None]
    one = np.float32(1)
    with np.errstate(all="ignore"):
        mix = lambda w, lo, hi: ((one - w) * lo).astype(np.float32) + (w * hi).astype(np.float32)
        top = np.where(fx[:, None] != 0, mix(a, g(sy, sx), g(sy, sx1)), g(sy, sx))
        bot = np.where(fx[:, None] != 0, mix(a, g(sy1, sx), g(sy1, sx1)), g(sy1, sx))
        return np.where(fy[:, None] != 0, mix(e, top, bot), top).astype(np.float32)


def because_score(act_max, protos, grid_cells=0, act_full=None, idx=None, cells=None, device=True):
    """(same, best fp32 [B, K], lost int32 [B, K]) of a perturbed forward for the rows protos / cells [B, K] (the contract is
    ppf_because_score's): same = the prototype's activation at the clean forward's cell, 0 with lost = 1 when the perturbed image no
    longer reserves it; best = its pooled activation wherever it is.  idx None: the global branch, (None, best, None)."""
    if device:
        from . import ops
        return ops.because_score(act_max, protos, grid_cells, act_full=act_full, idx=idx, cells=cells)
    am, pr = _host(act_max, np.float32), _host(protos, np.int64)
    (B, P), K = am.shape, pr.shape[1]
    ok = (pr >= 0) & (pr < P)
    best = np.where(ok, am[np.arange(B)[:, None], np.where(ok, pr, 0)], np.float32(np.nan)).astype(np.float32)
    if idx is None:
        return None, best, None
    ix, ce = _host(idx, np.int64), _host(cells, np.int64)
    T, G = ix.shape[1], int(grid_cells)
    af = _host(act_full, np.float32).reshape(B, P, T)
    same, lost = np.zeros((B, K), dtype=np.float32), np.ones((B, K), dtype=np.int32)
    for b in range(B):
        for k in range(K):
            if ok[b, k] and 0 <= ce[b, k] < G:
                t = np.flatnonzero(ix[b] == ce[b, k])
                if t.size:
                    same[b, k], lost[b, k] = af[b, pr[b, k], t[0]], 0
    return same, best, lost


def because_perturb(x, characteristic, params=None, seed=0, image_ids=None, device=True, out=None):
    """The image batch x [B, 3, H, W] with one characteristic suppressed at the strengths of because_params(params): 'hue', 'saturation'
    or 'contrast' (one colour transform; contrast after the luma sum and its offset), 'texture' (the bilateral filter) or 'shape' (the
    warp, keyed by seed and image_ids, None: 0 .. B-1).  device=True: launches only, into `out` when given; device=False: numpy."""
    p = because_params(params)
    mean, std = p["mean"], p["std"]
    B, H = x.shape[0], x.shape[2]
    if characteristic == "hue":
        return color_affine(x, hue_matrix(2.0 * np.pi * float(p["hue"])), mean, std, device=device, out=out)
    if characteristic == "saturation":
        return color_affine(x, saturation_matrix(p["saturation"]), mean, std, device=device, out=out)
    if characteristic == "contrast":
        off = contrast_offset(gray_sum(x, mean, std, device=device), x.shape[2:], p["contrast"], device=device)
        return color_affine(x, contrast_matrix(p["contrast"]), mean, std, offset=off, device=device, out=out)
    if characteristic == "texture":
        ws, wr = bilateral_tables(p["radius"], p["sigma_space"], p["sigma_range"])
        return bilateral(x, ws, wr, mean, std, device=device, out=out)
    if characteristic == "shape":
        A = warp_amplitude(p["amplitude"])
        _warp_sizes(H, p["cells"], A)
        ids = _image_ids(image_ids, B, x.device) if device else (np.arange(B, dtype=np.int64) if image_ids is None else _host(image_ids, np.int64))
        return warp_apply(x, warp_nodes_from_ids(ids, p["cells"], A, seed, device=device), p["cells"], A, device=device, out=out)
    raise ValueError(f"because: characteristics must come from {CHARACTERISTICS}, got {characteristic!r}")


class Because(Record):
    """What because returns, as device tensors (numpy arrays after cpu()): protos int32 [B, K]; base fp32 [B, K] the clean pooled
    activation of each prototype; cell int32 [B, K] the grid cell it was found at (-1 on the global branch); per characteristic n:
    same fp32 [n, B, K] its activation at that cell after the perturbation (0 where lost), best fp32 [n, B, K] its pooled activation
    wherever it is, lost int32 [n, B, K] = 1 where the perturbed image no longer reserves the cell.  On the global branch same and lost
    are None."""
    FIELDS = ("base", "cell", "same", "best", "lost", "protos")
    META = dict(characteristics=tuple, branch=None)

    def local(self):
        """The local importance [n, B, K] = base - same: how far the similarity at the same patch fell (best on the global branch)."""
        return self.base[None] - (self.best if self.same is None else self.same)

    def report(self, index):
        """The JSON records of image `index`: per prototype its id, cell, clean activation and per characteristic the local importance,
        the location-free one (base - best) and whether the cell was lost."""
        h = self.cpu()
        loc = h.local()
        out = []
        for k in range(h.protos.shape[1]):
            per = {}
            for n, name in enumerate(h.characteristics):
                per[name] = dict(importance=float(loc[n, index, k]), importance_best=float(h.base[index, k] - h.best[n, index, k]),
                                 lost=None if h.lost is None else bool(h.lost[n, index, k]))
            out.append(dict(prototype=int(h.protos[index, k]), cell=int(h.cell[index, k]), activation=float(h.base[index, k]), characteristics=per))
        return out


def _because_forward(ppnet, imgs, batch_size):
    """The model's eval forward over imgs in sub-batches of batch_size images: (act_full [R, P, T], idx [R, T], act_max local [R, P],
    act_max global [R, Pg]) on the device.  The caller holds eval mode and no_grad."""
    rs = forward_groups(ppnet, imgs, batch_size)
    cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts)
    return (cat([r.act_full.reshape(r.act_max_local.shape[0], r.act_max_local.shape[1], -1) for r in rs]).contiguous(),
            cat([r.idx for r in rs]).contiguous(), cat([r.act_max_local for r in rs]).contiguous(), cat([r.act_max_global for r in rs]).contiguous())


def _because_rows(ppnet, outs, protos, branch, B, device):
    """(protos int32 [B, K], base fp32 [B, K], cell int32 [B, K]) of the clean forward; protos None: the predicted class's."""
    local = branch == "local"
    act = outs["act_max"] if local else outs["act_max_global"]
    ppc = int(ppnet.num_prototypes_per_class) if local else act.shape[1] // outs["logits"].shape[1]
    if protos is None:
        protos = select_prototypes("predicted", ppc, outs["logits"].argmax(1)).to(torch.int32).contiguous()
    else:
        t = protos if isinstance(protos, torch.Tensor) and protos.is_cuda else torch.as_tensor(np.asarray(protos)).to(device)
        if t.is_floating_point() or t.dim() not in (1, 2) or t.shape[0] != B:
            raise ValueError(f"because: protos must be integers [B] or [B, K] for a batch of {B}, got {tuple(t.shape)} {t.dtype}")
        protos = (t[:, None] if t.dim() == 1 else t).to(torch.int32).contiguous()
    valid = (protos >= 0) & (protos < act.shape[1])               # an id outside the branch: NaN rows, nothing read (as the score kernel)
    protos_in = protos.long().clamp(0, act.shape[1] - 1)
    base = torch.where(valid, act.detach().gather(1, protos_in), torch.full_like(act[:, :1], float("nan")).expand(protos.shape)).contiguous()
    if not local:
        return protos, base, torch.full_like(protos, -1)
    idx = outs["idx"]
    tok = outs["argmax"].gather(1, protos_in).long() if outs["argmax"] is not None else torch.zeros_like(protos, dtype=torch.int64)
    ok = valid & (tok >= 0) & (tok < idx.shape[1])
    cell = torch.where(ok, idx.gather(1, tok.clamp(0, idx.shape[1] - 1)), torch.full_like(protos, -1)).to(torch.int32).contiguous()
    return protos, base, cell


@torch.no_grad()
def because(ppnet, x, protos=None, branch="local", characteristics=CHARACTERISTICS, params=None, seed=0, image_ids=None, batch_size=None,
            scratch_bytes=1 << 30):
    """Why does this patch look like that prototype: its hue, saturation, contrast, texture or shape?  For a batch x [B, 3, H, W] (CUDA)
    one eval forward; then per characteristic the perturbed images are written into ONE scratch buffer (as many images at a time as
    scratch_bytes holds, one at least), the model runs over them in sub-batches of batch_size images (default B), and one
    ppf_because_score launch reads the prototype's activation at the clean forward's cell.  No perturbed image and no activation map
    passes through the host.  protos: int [B] or [B, K], None: the prototypes of the predicted class; branch 'local' or 'global' (no
    cells: the pooled activation only); params: overrides of BECAUSE_DEFAULTS; seed, image_ids [B] (None: 0 .. B-1) key the warp, so an
    image warps the same way in every batch.  Returns a Because (device tensors; nothing is read back here)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError("because needs a CUDA/HIP batch [B, 3, H, W] (no CPU fallback path; color_affine / bilateral / warp_apply / because_score "
                           "with device=False are the host referees)")
    if branch not in EXPLAIN_BRANCHES:
        raise ValueError(f"because: branch must be one of {EXPLAIN_BRANCHES}, got {branch!r}")
    names = tuple(characteristics)
    if not names or any(n not in CHARACTERISTICS for n in names):
        raise ValueError(f"because: characteristics must come from {CHARACTERISTICS}, got {names}")
    from . import ops
    p = because_params(params)
    x = x.float().contiguous()
    B, G = x.shape[0], int(ppnet.num_patches)
    outs = _eval_outputs(ppnet, x)
    protos, base, cell = _because_rows(ppnet, outs, protos, branch, B, x.device)
    ids = _image_ids(image_ids, B, x.device)
    chunk = _chunk_items(B, scratch_bytes, x[0].numel() * 4)
    buf = torch.empty((chunk,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    same, best, lost = [], [], []
    with ppnet.eval_mode():
        for name in names:
            parts = []
            for i in range(0, B, chunk):
                n = min(chunk, B - i)
                imgs = because_perturb(x[i:i + n], name, p, seed, ids[i:i + n], out=buf[:n])
                parts.append(_because_forward(ppnet, imgs, int(batch_size or B)))
            act_full, idx, act_l, act_g = (parts[0][j] if len(parts) == 1 else torch.cat([q[j] for q in parts]) for j in range(4))
            if branch == "local":
                s, b, l = ops.because_score(act_l, protos, G, act_full=act_full, idx=idx, cells=cell)
                same.append(s); lost.append(l)
            else:
                b = ops.because_score(act_g, protos)[1]
            best.append(b)
    return Because(base, cell, torch.stack(same) if same else None, torch.stack(best), torch.stack(lost) if lost else None, protos, names, branch)


def _ordered_sum(v):
    """The fp64 sum of v in index order (one addition after the other: the order is part of the result)."""
    return float(np.cumsum(np.asarray(v, dtype=np.float64))[-1]) if len(v) else 0.0


def importance_from_rows(image_ids, protos, base, same, best, lost, characteristics):
    """The global importances from the rows of a data set, in fp64 on the host: image_ids [N], protos [N, K], base [N, K], same / best /
    lost [n, N, K] (same, lost None on the global branch: best stands in).  Per prototype that occurred, over its rows in image-id order
    (equal ids in row order): importance[i] = sum g (g - g_i) / sum g, the paper's weighted form with g = base and g_i = same;
    mean[i] = the unweighted mean of g - g_i; importance_best[i] = the same with best; lost[i] = the share of lost cells; rows; and
    dominant = the characteristic of the largest importance (ties: the earlier name).  Everything is None when there are no rows or
    sum g == 0.  Returns dict(per_prototype={id: ...}, overall=...), overall over all rows."""
    names = tuple(characteristics)
    ids, pr = np.asarray(image_ids).reshape(-1), np.asarray(protos)
    N, K = pr.shape if pr.ndim == 2 else (0, 0)
    g = np.asarray(base, dtype=np.float64).reshape(N, K)
    be = np.asarray(best, dtype=np.float64).reshape(len(names), N, K)
    sa = be if same is None else np.asarray(same, dtype=np.float64).reshape(len(names), N, K)
    lo = None if lost is None else np.asarray(lost, dtype=np.float64).reshape(len(names), N, K)
    order = np.argsort(np.repeat(ids, K), kind="stable") if N else np.zeros(0, dtype=np.int64)
    pf, gf = pr.reshape(-1)[order], g.reshape(-1)[order]
    saf, bef = sa.reshape(len(names), -1)[:, order], be.reshape(len(names), -1)[:, order]
    lof = None if lo is None else lo.reshape(len(names), -1)[:, order]

    def summary(sel):
        rows = int(sel.sum())
        gs = gf[sel]
        tot = _ordered_sum(gs)
        out = dict(rows=rows, importance={}, mean={}, importance_best={}, lost={}, dominant=None)
        for i, name in enumerate(names):
            live = rows > 0 and tot != 0.0
            out["importance"][name] = _ordered_sum(gs * (gs - saf[i][sel])) / tot if live else None
            out["importance_best"][name] = _ordered_sum(gs * (gs - bef[i][sel])) / tot if live else None
            out["mean"][name] = _ordered_sum(gs - saf[i][sel]) / rows if rows else None
            out["lost"][name] = None if lof is None or not rows else _ordered_sum(lof[i][sel]) / rows
        vals = [out["importance"][n] for n in names]
        if all(v is not None and v == v for v in vals) and vals:
            out["dominant"] = names[int(np.argmax(vals))]                  # the first of equal maxima: the earlier name
        return out
    return dict(per_prototype={int(p): summary(pf == p) for p in np.unique(pf)}, overall=summary(np.ones(pf.shape, dtype=bool)))


def characteristic_importance(ppnet, loader, protos="own", branch="local", characteristics=CHARACTERISTICS, params=None, seed=0, max_images=0,
                              pass_images=16, protos_per_image=3, scratch_bytes=1 << 30, per_image=False):
    """The importance of every characteristic for every prototype over a data set.  loader yields (x, labels) or (x, labels, ids); its
    images are regrouped into passes of pass_images images, so the result does not depend on the loader's batch size, and each pass is
    one `because` call.  protos 'own': all prototypes of the image's label class (the paper's own-class images); 'top': the
    protos_per_image strongest prototypes of the predicted class (larger pooled activation first, equal ones by smaller id).  The rows
    stay on the device and are read once at the end; the sums are importance_from_rows's.  Returns its dict plus images, characteristics,
    branch and, with per_image, rows = dict(image_ids, labels, protos, cell, base, same, best, lost) as numpy arrays."""
    if protos not in ("own", "top"):
        raise ValueError(f"characteristic_importance: protos must be 'own' or 'top', got {protos!r}")
    names, local = tuple(characteristics), branch == "local"
    keep = []
    fields = ((x.float(), torch.as_tensor(y).to(x.device, torch.int64), ids.to(x.device)) for x, y, ids in batches_with_ids(loader, int(max_images)))
    for x, y, ids in regroup(fields, int(pass_images)):
        x = x if x.is_cuda else x.cuda()
        y, ids = y.to(x.device), ids.to(x.device)
        C = ppnet.last_layer.weight.shape[0]
        ppc = int(ppnet.num_prototypes_per_class) if local else ppnet.prototype_vectors_global.shape[0] // C
        if protos == "own":
            pr = select_prototypes("own", ppc, y, num_classes=C)
        else:
            outs = _eval_outputs(ppnet, x.float().contiguous())                            # the pick's own forward; because runs another
            K = min(int(protos_per_image), ppc)            # this pass's clamp: min(k, ppc), at most ppc and no lower bound
            pr = select_prototypes("top", ppc, outs["logits"].argmax(1), outs["act_max"] if local else outs["act_max_global"], K)
        r = because(ppnet, x, pr.to(torch.int32), branch, names, params, seed, ids, None, scratch_bytes)
        keep.append(dict(image_ids=ids, labels=y, protos=r.protos, cell=r.cell, base=r.base, same=r.same, best=r.best, lost=r.lost))
    rows = read_rows(keep, "characteristic_importance", dict(same=1, best=1, lost=1))                      # the one read; [n, N, K]: images on dim 1
    out = importance_from_rows(rows["image_ids"], rows["protos"], rows["base"], rows["same"], rows["best"], rows["lost"], names)
    out.update(images=int(rows["image_ids"].shape[0]), characteristics=list(names), branch=branch)
    if per_image:
        out["rows"] = rows
    return out


# ------------------------------------------------------------------------------------------------ foreground focus: does the model look at the object?
# ProtoPFormer's argument is about where the model looks: the rollout reservation is to keep the object's tokens, the local prototypes
# are to fire on its parts.  With an annotated object box per image (CUB's bounding_boxes.txt) three questions have numbers: are the
# reserved tokens on the object, do the prototype maps peak and carry their positive mass there (the pointing game and its energy-based
# form, Wang et al., Score-CAM, 2020), and how much of the class evidence comes from cells on the object.  Each is reported next to
# `chance`, the object's share of the image area: what a spatially blind map, reservation or evidence would score.  The kernels:
# ppf_act_focus, ppf_focus_box_terms, ppf_reserve_focus (csrc/interp.hip) and ppf_evidence_focus (csrc/explain.hip); the numpy forms
# below (device=False) are the referees (the contract is in include/ppf_hip.h).  The reference has no such pass.
FOCUS_PROTOS = ("own", "top")
FOCUS_FIELDS = ("protos", "classes", "peak_val", "peak_yx", "hit", "inside", "total", "nonfinite", "box", "terms", "reserve", "attn", "ev", "cnt",
                "global_ev", "obj", "labels")


def scaled_boxes(ids, boxes, image_sizes, img_size):
    """The object boxes of a batch in pixels of the square img_size x img_size view (Resize((S, S)): a linear map per axis): int32
    [B, 4] rows (Y0, Y1, X0, X1), half-open.  boxes {img_id: (x0, y0, x1, y1)} in pixels of the original file, image_sizes {img_id:
    (width, height)}.  In integers: X0 = (S * x0) // w, X1 = min(S, max(X0 + 1, ceil(S * x1 / w))), likewise in y: the scaled box covers
    every view pixel the source box touches and is never empty for a non-empty source box.  The host referee and the device path both
    take their boxes from here (as scaled_parts for the parts)."""
    S = int(img_size)
    out = np.zeros((len(ids), 4), dtype=np.int32)
    for j, i in enumerate(ids):
        x0, y0, x1, y1 = (int(v) for v in boxes[int(i)])
        w, h = (int(v) for v in image_sizes[int(i)])
        X0, Y0 = (S * x0) // w, (S * y0) // h
        X1, Y1 = min(S, max(X0 + 1, -((-S * x1) // w))), min(S, max(Y0 + 1, -((-S * y1) // h)))
        out[j] = (Y0, Y1, X0, X1)
    return out


def _clipped(box, size):
    return np.clip(np.asarray(box, dtype=np.int64).reshape(-1, 4), 0, int(size))


def act_focus(grids, size, obj, device=True):
    """Peak and positive mass of every up-sampled map against its image's object box: dict(peak_val [M] fp32, peak_yx [M, 2] int32, hit
    [M] int32, inside / total [M] fp64, nonfinite [M] int32); grids [M, g, g] fp32, obj int32 [M_img, 4] (y0, y1, x0, x1), half-open, map m
    belonging to image m // (M / M_img).  device=True: one ppf_act_focus launch, device tensors.  device=False: the numpy referee:
    resize_cubic per map, then np.where / np.sum in fp64."""
    if device:
        from . import ops
        return ops.act_focus(grids, size, obj)
    grids, S = _host(grids, np.float32), int(size)
    M = grids.shape[0]
    ob = _clipped(_host(obj, np.int32), S)
    if M and (ob.shape[0] == 0 or M % ob.shape[0]):
        raise ValueError(f"act_focus: {M} maps do not divide over {ob.shape[0]} object boxes")
    per = M // ob.shape[0] if M else 1
    out = dict(peak_val=np.zeros(M, dtype=np.float32), peak_yx=np.zeros((M, 2), dtype=np.int32), hit=np.zeros(M, dtype=np.int32),
               inside=np.zeros(M), total=np.zeros(M), nonfinite=np.zeros(M, dtype=np.int32))
    for m in range(M):
        with np.errstate(invalid="ignore"):                                         # inf - inf of a map with non-finite entries
            up = resize_cubic(grids[m], S)
        y0, y1, x0, x1 = ob[m // per]
        seen = ~np.isnan(up)
        top = up[seen].max() if seen.any() else np.float32(-np.inf)                # a NaN never wins; only NaNs: (0, 0), -inf
        ys, xs = np.where(up == top)
        y, x = (int(ys[0]), int(xs[0])) if ys.size else (0, 0)
        fin = np.isfinite(up)
        with np.errstate(invalid="ignore"):
            pos = np.where(fin & (up > 0), up, np.float32(0)).astype(np.float64)
        out["peak_val"][m], out["peak_yx"][m], out["hit"][m] = top, (y, x), int(y0 <= y < y1 and x0 <= x < x1)
        out["inside"][m], out["total"][m], out["nonfinite"][m] = np.sum(pos[y0:max(y1, y0), x0:max(x1, x0)]), np.sum(pos), int((~fin).sum())
    return out


def focus_box_terms(box, obj, size, device=True):
    """int32 [M, 4] = (intersection, box, object, union) areas of box [M, 4] (high_activation_boxes) against obj [M_img, 4], both clipped
    to the size x size image.  device=True: one ppf_focus_box_terms launch; device=False: integer numpy."""
    if device:
        from . import ops
        return ops.focus_box_terms(box, obj, size)
    a, o = _clipped(_host(box, np.int32), size), _clipped(_host(obj, np.int32), size)
    M = a.shape[0]
    if M and (o.shape[0] == 0 or M % o.shape[0]):
        raise ValueError(f"focus_box_terms: {M} boxes do not divide over {o.shape[0]} object boxes")
    o = np.repeat(o, M // o.shape[0], axis=0) if M else o[:0]
    area = lambda b: np.maximum(b[:, 1] - b[:, 0], 0) * np.maximum(b[:, 3] - b[:, 2], 0)
    inter = (np.maximum(np.minimum(a[:, 1], o[:, 1]) - np.maximum(a[:, 0], o[:, 0]), 0)
             * np.maximum(np.minimum(a[:, 3], o[:, 3]) - np.maximum(a[:, 2], o[:, 2]), 0))
    inter = np.where((area(a) > 0) & (area(o) > 0), inter, 0)
    return np.stack([inter, area(a), area(o), area(a) + area(o) - inter], axis=1).astype(np.int32)


def _centre_inside(cells, grid_side, patch, ob):
    """Is the centre pixel (cy * patch + patch // 2, cx * patch + patch // 2) of each grid cell inside the clipped box ob?"""
    cy, cx = cells // grid_side, cells % grid_side
    py, px = cy * patch + patch // 2, cx * patch + patch // 2
    return (py >= ob[0]) & (py < ob[1]) & (px >= ob[2]) & (px < ob[3])


def reserve_focus(idx, obj, grid_side, patch, token_attn=None, device=True):
    """The reserved tokens against the object box: (out int32 [B, 4], attn fp64 [B, 2] or None).  idx int32 [B, T] the grid cells of the
    reserved tokens on the grid_side x grid_side grid of patch x patch pixel cells; out = (pixels of the reserved cells inside the box,
    reserved cells whose centre pixel is inside, all cells whose centre is inside, idx entries inside [0, grid_side^2): the others are
    skipped); attn, with token_attn [B, grid_side^2]: the rollout score over the cells with centre inside and over all cells, non-finite
    scores counting 0.  device=True: one ppf_reserve_focus launch; device=False: the numpy referee."""
    if device:
        from . import ops
        return ops.reserve_focus(idx, obj, grid_side, patch, token_attn)
    idx, g, patch = _host(idx, np.int64), int(grid_side), int(patch)
    B, G = idx.shape[0], g * g
    ob = _clipped(_host(obj, np.int32), g * patch)
    ta = None if token_attn is None else _host(token_attn, np.float32).reshape(B, G)
    out, attn = np.zeros((B, 4), dtype=np.int32), None if ta is None else np.zeros((B, 2))
    cells = np.arange(G)
    for b in range(B):
        c = idx[b][(idx[b] >= 0) & (idx[b] < G)]
        cy, cx = c // g, c % g
        oy = np.maximum(np.minimum((cy + 1) * patch, ob[b, 1]) - np.maximum(cy * patch, ob[b, 0]), 0)
        ox = np.maximum(np.minimum((cx + 1) * patch, ob[b, 3]) - np.maximum(cx * patch, ob[b, 2]), 0)
        on = _centre_inside(cells, g, patch, ob[b])
        out[b] = (int((oy * ox).sum()), int(_centre_inside(c, g, patch, ob[b]).sum()), int(on.sum()), c.size)
        if ta is not None:
            v = np.where(np.isfinite(ta[b]), ta[b], np.float32(0)).astype(np.float64)
            attn[b] = (np.sum(v[on]), np.sum(v))
    return out, attn


def evidence_focus(act_max, weight, scale, ppc, classes, obj, grid_side, patch, idx, argmax=None, device=True):
    """The local branch's class evidence against the object box: (ev fp64 [B, M, 4], cnt int32 [B, M, 4]) for classes int32 [B, M]: the
    sums and the term counts of the contributions fl(act_max[b][p] * fl(scale * weight[c][p])) over (own class and cell centre inside,
    own class and not inside, other classes and inside, other classes and not inside); the cell of p is idx[b][argmax[b][p]] (argmax
    None: idx[b][0]), and a prototype without a valid cell counts as not inside.  A class outside [0, C): zeros.  device=True: one
    ppf_evidence_focus launch; device=False: the numpy referee (the same fp32 products, np.sum in fp64)."""
    if device:
        from . import ops
        return ops.evidence_focus(act_max, weight, scale, ppc, classes, obj, grid_side, patch, idx=idx, argmax=argmax)
    act_max, weight, idx = _host(act_max, np.float32), _host(weight, np.float32), _host(idx, np.int64)
    argmax, cls = _host(argmax, np.int64), _host(classes, np.int32)
    (B, P), C, T, g, patch = act_max.shape, weight.shape[0], idx.shape[1], int(grid_side), int(patch)
    cls = cls.reshape(B, -1)
    M = cls.shape[1]
    ob = _clipped(_host(obj, np.int32), g * patch)
    ev, cnt = np.zeros((B, M, 4)), np.zeros((B, M, 4), dtype=np.int32)
    proto_class = np.arange(P) // int(ppc)
    with np.errstate(all="ignore"):
        w = np.float32(scale) * weight                                               # fp32: the first rounding
        for b in range(B):
            t = np.zeros(P, dtype=np.int64) if argmax is None else argmax[b]
            ok = (t >= 0) & (t < T)
            cell = np.where(ok, idx[b, np.clip(t, 0, T - 1)], -1)
            ok &= (cell >= 0) & (cell < g * g)
            inside = ok & _centre_inside(np.where(ok, cell, 0), g, patch, ob[b])
            for m in range(M):
                c = int(cls[b, m])
                if c < 0 or c >= C:
                    continue
                ctr = (act_max[b] * w[c]).astype(np.float64)                         # fp32: the second rounding; then exact in fp64
                own = proto_class == c
                for j, sel in enumerate((own & inside, own & ~inside, ~own & inside, ~own & ~inside)):
                    ev[b, m, j], cnt[b, m, j] = np.sum(ctr[sel]), int(sel.sum())
    return ev, cnt


class Focus(Record):
    """What focus_rows returns, as device tensors (numpy arrays after cpu()), K prototypes per image: protos int32 [B, K]; classes int32
    [B] the predicted class; peak_val fp32, hit / nonfinite int32, inside / total fp64 [B, K], peak_yx int32 [B, K, 2] (ppf_act_focus);
    box int32 [B, K, 4] the top-percentile box and terms int32 [B, K, 4] its (intersection, box, object, union) areas; reserve int32
    [B, 4] and attn fp64 [B, 2] (ppf_reserve_focus); ev fp64 [B, 4] and cnt int32 [B, 4] the predicted class's local evidence
    (ppf_evidence_focus); global_ev fp64 [B] the global branch's share of the predicted logit (it has no cells: unlocated), or None;
    obj int32 [B, 4]; labels int64 [B] or None.  img_size, grid_side, patch, mode, percentile: the settings."""

    FIELDS = FOCUS_FIELDS
    META = dict(img_size=int, grid_side=int, patch=int, mode=None, percentile=None)


def focus_from_outputs(outs, obj, weight, scale, ppc, k, img_size, labels=None, protos="own", protos_per_image=3, percentile=95, global_coe=None,
                       device=True):
    """focus_rows on what one eval forward left (outs: token_attn [B, G], idx [B, T], act_full [B, P, T], logits [B, C], act_max [B, P],
    argmax [B, P] or None, optionally logits_global [B, C]: _eval_outputs); weight [C, P] and scale: the local last layer and its share of the logit; k:
    the reserved tokens per image.  device=True: CUDA tensors in, the kernels, a Focus of device tensors.  device=False: the referee
    pipeline on host copies -- the same selection, expand_to_grid, then the numpy referees with find_high_activation_crop of
    resize_cubic for the boxes -- and a Focus of numpy arrays."""
    if protos not in FOCUS_PROTOS:
        raise ValueError(f"focus: protos must be 'own' or 'top', got {protos!r}")
    if protos == "own" and labels is None:
        raise ValueError("focus: protos='own' takes the prototypes of labels[b]: labels are needed")
    place = (lambda t: t) if device else (lambda t: None if t is None else torch.as_tensor(t).detach().cpu())
    o = {n: place(v) for n, v in outs.items()}
    obj_t, weight = place(obj), place(weight)
    B, P = o["act_max"].shape
    C, ppc, S, dev = weight.shape[0], int(ppc), int(img_size), o["act_max"].device
    G = o["token_attn"].shape[1]
    g = int(round(G ** 0.5))
    patch = S // g
    pred = o["logits"].argmax(1)
    if protos == "own":
        lab = torch.as_tensor(labels).to(dev, torch.int64)
        pr = select_prototypes("own", ppc, lab, num_classes=C)
    else:
        lab = None if labels is None else torch.as_tensor(labels).to(dev, torch.int64)
        K = max(1, min(int(protos_per_image), ppc))        # this pass's clamp: max(1, min(k, ppc)), at most ppc and at least one
        pr = select_prototypes("top", ppc, pred, o["act_max"], K)
    K, s = pr.shape[1], int(round(int(k) ** 0.5))
    sel = torch.gather(o["act_full"].reshape(B, P, -1), 1, pr[:, :, None].expand(B, K, int(k))).reshape(B, K, s, s)
    grid = patch_grid(o["token_attn"], sel, int(k)).contiguous()                         # expand_to_grid of the selected prototypes only
    maps = grid.reshape(B * K, g, g)
    cls = pred.to(torch.int32)[:, None].contiguous()
    if device:
        f = act_focus(maps, S, obj_t)
        box = high_activation_boxes(grid, S, percentile).reshape(B * K, 4)
    else:
        f = act_focus(maps.numpy(), S, obj_t.numpy(), device=False)
        box = np.array([find_high_activation_crop(resize_cubic(a, S), percentile) for a in maps.numpy()], dtype=np.int32).reshape(B * K, 4)
    terms = focus_box_terms(box, obj_t, S, device=device)
    reserve, attn = reserve_focus(o["idx"], obj_t, g, patch, o["token_attn"], device=device)
    ev, cnt = evidence_focus(o["act_max"], weight, scale, ppc, cls, obj_t, g, patch, o["idx"], o["argmax"], device=device)
    glob = None
    if o.get("logits_global") is not None and global_coe is not None:
        glob = float(global_coe) * o["logits_global"].double().gather(1, pred[:, None]).reshape(B)
    host = (lambda t: t) if device else (lambda t: None if t is None else (t.numpy() if isinstance(t, torch.Tensor) else t))
    shape = lambda t, *tail: t.reshape((B, K) + tail)
    fields = dict(protos=host(pr.to(torch.int32)), classes=host(cls.reshape(B)), peak_val=shape(f["peak_val"]), peak_yx=shape(f["peak_yx"], 2),
                  hit=shape(f["hit"]), inside=shape(f["inside"]), total=shape(f["total"]), nonfinite=shape(f["nonfinite"]), box=shape(box, 4),
                  terms=shape(terms, 4), reserve=reserve, attn=attn, ev=ev.reshape(B, 4), cnt=cnt.reshape(B, 4), global_ev=host(glob),
                  obj=host(obj_t), labels=host(lab))
    return Focus(**fields, img_size=S, grid_side=g, patch=patch, mode=protos, percentile=percentile)


@torch.no_grad()
def focus_rows(ppnet, x, obj, labels=None, protos="own", protos_per_image=3, percentile=95):
    """The foreground-focus measurements of one batch x [B, 3, S, S] against obj int32 [B, 4] = (y0, y1, x0, x1), half-open, in pixels of
    the model input (scaled_boxes).  One eval forward, expand_to_grid of the selected local prototypes only, one ppf_act_focus, the
    order-statistics and box launches of high_activation_boxes (which reads its two order statistics per map back), ppf_focus_box_terms,
    ppf_reserve_focus, and ppf_evidence_focus for the predicted class.  protos 'own': the prototypes of labels[b]; 'top': the
    protos_per_image strongest local prototypes of the predicted class by pooled activation (equal ones by smaller id).  Returns a Focus
    of device tensors; .cpu() is one host read."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError("focus_rows needs a CUDA/HIP batch [B, 3, S, S] (no CPU fallback path; focus_from_outputs(device=False) is the host referee)")
    obj = obj if isinstance(obj, torch.Tensor) and obj.is_cuda else torch.as_tensor(np.asarray(obj)).to(x.device)
    obj = obj.to(torch.int32).contiguous()
    coe = float(ppnet.global_coe)
    return focus_from_outputs(_eval_outputs(ppnet, x.float().contiguous()), obj, ppnet.last_layer.weight.detach().contiguous(), 1.0 - coe,
                              ppnet.num_prototypes_per_class, ppnet.reserve_token_nums[0], ppnet.img_size, labels, protos, protos_per_image,
                              percentile, coe)


def _ordered_mean(v):
    """(fp64 mean of v in index order, or None for no value; how many values)."""
    v = np.asarray(v, dtype=np.float64)
    return (_ordered_sum(v) / v.size if v.size else None), int(v.size)


def _ratio_mean(num, den):
    """_ordered_mean of num / den over the entries with den > 0."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = den > 0
    return _ordered_mean(num[live] / den[live])


def focus_summary(rows, img_size, patch, per_prototype=True):
    """The report of foreground_focus from all rows, on the host: rows = dict of numpy arrays, image_ids [N] and the fields of Focus
    (protos, hit, inside, total, nonfinite, terms [N, K, ...]; reserve, attn, ev, cnt, global_ev, obj, classes, labels [N, ...]).  The
    rows are put into image-id order first (equal ids keep their order) and every mean is an fp64 sum in that order, or a ratio of
    integer sums: the result does not depend on how the images were batched or on the order they arrived in.
    Prototype maps: pointing = hits / rows; energy = the mean of inside / total over the rows with total > 0 (energy_rows of them;
    zero_total_rows and nonfinite_rows are counted, not hidden); iou, box_inside = intersection / union and intersection / box area of
    the top-percentile box; chance = the mean object area / S^2, what a spatially blind map scores in pointing and energy.
    Reservation: reserved_on_object = reserved pixels inside / (valid reserved cells * patch^2) against the same chance; object_recall =
    reserved cells with centre inside / grid cells with centre inside (images_without_object_cells counted separately);
    attention_on_object = the rollout score on cells with centre inside / over all cells.  Evidence of the predicted class:
    own_inside = own-class evidence located inside / own-class evidence, over the images where the latter is > 0 (own_images);
    other_inside likewise for the other classes' prototypes; global_branch_share = the global branch's part of (global + local)
    evidence, unlocated since that branch has no cells.  Returns dict(images, rows, overall, per_class {class: ...}, per_prototype
    {prototype: the prototype-map measures} or None); a class is the image's label when labels are given, else the predicted class."""
    S, patch = int(img_size), int(patch)
    ids = np.asarray(rows["image_ids"]).reshape(-1)
    order = np.argsort(ids, kind="stable")
    r = {k: (None if v is None else np.asarray(v)[order]) for k, v in rows.items()}
    N = ids.size
    K = r["protos"].shape[1] if N else 0
    cls_img = r["labels"] if r.get("labels") is not None else r["classes"]
    cls_row = np.repeat(cls_img, K)
    flat = {k: r[k].reshape((N * K,) + r[k].shape[2:]) for k in ("protos", "hit", "inside", "total", "nonfinite", "terms")}

    def maps(sel):
        hit, ins, tot, nf, t = (flat[k][sel] for k in ("hit", "inside", "total", "nonfinite", "terms"))
        n = int(hit.shape[0])
        energy, energy_rows = _ratio_mean(ins, tot)
        return dict(rows=n, pointing=(int(hit.astype(np.int64).sum()) / n if n else None), energy=energy, energy_rows=energy_rows,
                    zero_total_rows=int((tot == 0).sum()), nonfinite_rows=int((nf > 0).sum()), iou=_ratio_mean(t[:, 0], t[:, 3])[0],
                    box_inside=_ratio_mean(t[:, 0], t[:, 1])[0], chance=_ordered_mean(t[:, 2].astype(np.float64) / float(S * S))[0])

    def images(sel):
        res, ob, ev = r["reserve"][sel].astype(np.int64), _clipped(r["obj"][sel], S), r["ev"][sel]
        n = int(res.shape[0])
        recall, with_cells = _ratio_mean(res[:, 1], res[:, 2])
        out = dict(images=n, reserved_on_object=_ratio_mean(res[:, 0], res[:, 3] * patch * patch)[0], object_recall=recall,
                   images_without_object_cells=n - with_cells,
                   attention_on_object=None if r.get("attn") is None else _ratio_mean(r["attn"][sel][:, 0], r["attn"][sel][:, 1])[0],
                   chance=_ordered_mean((ob[:, 1] - ob[:, 0]).clip(0) * (ob[:, 3] - ob[:, 2]).clip(0) / float(S * S))[0])
        own, own_images = _ratio_mean(ev[:, 0], ev[:, 0] + ev[:, 1])
        other, other_images = _ratio_mean(ev[:, 2], ev[:, 2] + ev[:, 3])
        ge = None
        if r.get("global_ev") is not None:
            ge = _ratio_mean(r["global_ev"][sel], r["global_ev"][sel] + ev.sum(1))[0]
        return out, dict(own_inside=own, own_images=own_images, other_inside=other, other_images=other_images, global_branch_share=ge)

    def group(sel_rows, sel_img):
        reservation, evidence = images(sel_img)
        return dict(prototype_maps=maps(sel_rows), reservation=reservation, evidence=evidence)
    all_rows, all_img = np.ones(N * K, dtype=bool), np.ones(N, dtype=bool)
    return dict(images=int(N), rows=int(N * K), overall=group(all_rows, all_img),
                per_class={int(c): group(cls_row == c, cls_img == c) for c in np.unique(cls_img)} if N else {},
                per_prototype={int(p): maps(flat["protos"] == p) for p in np.unique(flat["protos"])} if per_prototype and N else None)


def foreground_focus(ppnet, loader, boxes, image_sizes, protos="own", protos_per_image=3, percentile=95, max_images=0, per_image=False):
    """Foreground focus over a data set.  loader yields (x, targets, img_ids) in the square view (Resize((S, S))); boxes {img_id: (x0, y0,
    x1, y1)} in pixels of the original file, image_sizes {img_id: (width, height)} (scaled_boxes maps them into the view).  Per batch one
    focus_rows; the rows stay on the device and are read once at the end; the summaries are focus_summary's, taken in image-id order.
    Returns its dict plus settings and, with per_image, per_image = the rows as numpy arrays (image_ids and the fields of Focus)."""
    if protos not in FOCUS_PROTOS:
        raise ValueError(f"foreground_focus: protos must be 'own' or 'top', got {protos!r}")
    keep, meta = [], None
    for x, y, ids in batches_with_ids(loader, max_images):
        x = x if x.is_cuda else x.cuda()
        obj = torch.from_numpy(scaled_boxes(ids.cpu().tolist(), boxes, image_sizes, ppnet.img_size)).to(x.device)
        f = focus_rows(ppnet, x, obj, torch.as_tensor(y).to(x.device, torch.int64), protos, protos_per_image, percentile)
        keep.append(dict(f.fields(), image_ids=ids.to(x.device)))
        meta = f
    rows = read_rows(keep, "foreground_focus")                                                             # the one read
    out = focus_summary(rows, meta.img_size, meta.patch, per_prototype=protos == "own")
    out["settings"] = dict(protos=protos, protos_per_image=int(protos_per_image), percentile=percentile, img_size=meta.img_size, patch=meta.patch)
    if per_image:
        out["per_image"] = rows
    return out


# ------------------------------------------------------------------------------------------------ part interventions on PartsWorld
# Every faithfulness number above removes content by painting over it.  On PartsWorld the scene table is the render's input: a row edited
# (ppf_synth_edit) and rendered again under the same id is the same image without part k, without the distractors or with another class's
# part, noise included -- so what a part is worth to the model can be measured exactly, and an explanation held to it (the protocol of
# FunnyBirds, Hesse et al., ICCV 2023).  ppf_part_mass says how much of a score map lies on each primitive, through the view rule of
# include/ppf_hip.h.  The numpy forms (device=False) are the referees.  The reference has no such pass.
PART_ORDERS = ("evidence", "attention", "random", "rise", "ig")
PART_VALUES = ("prob", "logit")
EDIT_COUNTERFACTUAL = 5             # in Interventions.edits only: the chain of PART_ATTR edits towards class `arg`; ppf_synth_edit never sees it


def part_mass(score, partmap, rows_per_img, K, device=True):
    """(pos fp64 [R, 3 + K], neg fp64 [R, 3 + K], count int32 [R, 3 + K], nonfinite int32 [R]) of score fp32 [R, S, S] (or [B, M, S, S]
    with rows_per_img = M) and partmap uint8 [R / rows_per_img, H, W]: the sums of max(s, 0) and max(-s, 0) over the view pixels of each
    primitive code (0 background, 1 distractor, 2 body, 3 + k part k; the view rule of include/ppf_hip.h), the pixels per code, and the
    pixels that are non-finite (they add 0 and stay counted under their code) or carry a code above 2 + K (counted nowhere else).
    device=True: one ppf_part_mass launch on CUDA tensors (no fallback); device=False: the numpy referee, its sums exactly rounded (math.fsum)."""
    if device:
        from . import ops
        return ops.part_mass(score.reshape((-1,) + tuple(score.shape[-2:])), partmap, rows_per_img, K)
    from .data import partsworld_view_partmap
    s = np.asarray(score.cpu() if isinstance(score, torch.Tensor) else score, dtype=np.float32)
    s = s.reshape((-1,) + s.shape[-2:])
    R, S, nb = s.shape[0], s.shape[-1], 3 + int(K)
    if s.shape[-2] != S or rows_per_img < 1 or R % rows_per_img:
        raise ValueError(f"part_mass: score must be [R, S, S] with R a multiple of rows_per_img={rows_per_img}, got {s.shape}")
    codes = partsworld_view_partmap(partmap, S)
    pos, neg = np.zeros((R, nb), dtype=np.float64), np.zeros((R, nb), dtype=np.float64)
    count, bad = np.zeros((R, nb), dtype=np.int32), np.zeros(R, dtype=np.int32)
    for r in range(R):
        code, fin = codes[r // rows_per_img], np.isfinite(s[r])
        bad[r] = int((~fin | (code >= nb)).sum())
        v = np.where(fin, s[r], np.float32(0)).astype(np.float64)
        for c in range(nb):
            sel = code == c
            count[r, c] = int(sel.sum())
            pos[r, c], neg[r, c] = math.fsum(np.maximum(v[sel], 0.0).tolist()), math.fsum(np.maximum(-v[sel], 0.0).tolist())     # exactly rounded
    return pos, neg, count, bad


class Interventions(Record):
    """What part_interventions returns, as device tensors (numpy arrays after cpu()): edits int32 [B, E, 2] = (op, arg) as ppf_synth_edit
    takes them (the counterfactual column reads (EDIT_COUNTERFACTUAL, target class)); changed int32 [B, E]; value fp32 [B, E, M], the
    probability or the logit of class classes[b, m] on the image of edit e; classes int32 [B, M]; scene int32 [B, SYNTH_WORDS], the unedited
    table; pred int32 [B, E], the arg-max class on the image of edit e."""
    FIELDS = ("edits", "changed", "value", "classes", "scene", "pred")
    META = dict(kind=str)


def standard_edits(spec):
    """The edit list of part_interventions as host rows [(op, arg)], E - 1 = K + 4 of them; the counterfactual follows as the last column.
    COPY, PARTS_OFF 1 << k for every k, PARTS_OFF of all, DISTRACTORS_OFF of all, BACKGROUND (128, 128, 128)."""
    from . import data as D
    K = spec.parts
    return ([(D.EDIT_COPY, 0)] + [(D.EDIT_PARTS_OFF, 1 << k) for k in range(K)] + [(D.EDIT_PARTS_OFF, (1 << K) - 1)]
            + [(D.EDIT_DISTRACTORS_OFF, (1 << spec.distractors) - 1), (D.EDIT_BACKGROUND, 128 | 128 << 8 | 128 << 16)])


def _counterfactual_rows(spec, scene, ids):
    """(rows int32 [B, SYNTH_WORDS], changed int32 [B], target int32 [B]): every image's row turned into the row of class (label + 1) % C
    with the same geometry: PART_ATTR for every part k with the other class's attribute, one ppf_synth_edit call per k on the previous
    call's rows (where the two classes agree the edit changes nothing).  The chain lives here, not in the kernel."""
    from . import data as D
    from . import ops
    C, K = spec.classes, spec.parts
    table = torch.from_numpy(D.partsworld_class_table(spec)).to(scene.device)
    target = ((ids % C + 1) % C).to(torch.int64)
    rows, changed = scene, torch.zeros(scene.shape[0], dtype=torch.int32, device=scene.device)
    for k in range(K):
        arg = (table[target, k].to(torch.int32) << 8) | k
        edit = torch.stack([torch.full_like(arg, D.EDIT_PART_ATTR), arg], dim=1)[:, None, :].contiguous()
        out, ch = ops.synth_edit(spec, rows, edit, check=False)
        rows, changed = out[:, 0].contiguous(), torch.maximum(changed, ch[:, 0])
    return rows, changed, target.to(torch.int32)


@torch.no_grad()
def part_interventions(ppnet, spec, ids, classes=None, top_classes=1, value="prob", edits=None, batch_size=None, scratch_bytes=1 << 30):
    """What every edit of the scene is worth to the model, for PartsWorld images ids int64 [B]: ppf_synth_scene, ppf_synth_edit, then
    ppf_synth_render of the B * E edited rows under ids.repeat_interleave(E) in chunks into one scratch buffer of at most scratch_bytes
    (one frame at least), data.partsworld_view, the model's forward in groups of batch_size images (default B) and ppf_class_prob (value
    'prob') or the logit column ('logit').  Nothing image-sized passes through the host; ppnet.precise is honoured.
    edits None: the standard list, E = K + 5 -- standard_edits(spec), then the counterfactual (the image of class (label + 1) % C with
    the same geometry and noise, _counterfactual_rows); else int32 [B, E, 2] of ppf_synth_edit's ops (an invalid one raises after the
    one read of `changed`).  classes: as in explain; None: the top `top_classes` of the unedited image's logits (_pick_classes).
    Returns an Interventions of device tensors; .cpu() is one host read."""
    from . import data as D
    from . import ops
    if value not in PART_VALUES:
        raise ValueError(f"part_interventions: value must be one of {PART_VALUES}, got {value!r}")
    ids = D._device_ids(ids).contiguous()
    B, H, W, S = ids.shape[0], spec.height, spec.width, int(ppnet.img_size)
    scene = ops.synth_scene(spec, ids)
    if edits is None:
        std = torch.tensor(standard_edits(spec), dtype=torch.int32, device=ids.device)[None].expand(B, -1, -1).contiguous()
        rows, changed = ops.synth_edit(spec, scene, std, check=False)
        cf_rows, cf_changed, target = _counterfactual_rows(spec, scene, ids)
        rows, changed = torch.cat([rows, cf_rows[:, None]], dim=1), torch.cat([changed, cf_changed[:, None]], dim=1)
        edits = torch.cat([std, torch.stack([torch.full_like(target, EDIT_COUNTERFACTUAL), target], dim=1)[:, None]], dim=1)
    else:
        edits = edits if isinstance(edits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(edits, dtype=np.int32))
        edits = edits.to(device=ids.device, dtype=torch.int32).contiguous()
        rows, changed = ops.synth_edit(spec, scene, edits, check=True)
    E = rows.shape[1]
    rows, ids_rep = rows.reshape(B * E, -1).contiguous(), ids.repeat_interleave(E)
    finisher, frame = D.GpuFinisher(re_prob=0.0), H * W * 3
    chunk = _chunk_items(B * E, scratch_bytes, frame)
    buf, ws = torch.empty(chunk * frame, dtype=torch.uint8, device=ids.device), None
    Cn = ppnet.last_layer.weight.shape[0]
    logits = torch.empty((B * E, Cn), dtype=torch.float32, device=ids.device)
    with ppnet.eval_mode():
        if classes is None:                               # the predicted class of the unedited image
            x0 = []
            for s0 in range(0, B, chunk):
                n = min(chunk, B - s0)
                f = ops.synth_render(spec, scene[s0:s0 + n], ids[s0:s0 + n].contiguous(), out=buf[:n * frame])
                x0.append(D.partsworld_view(spec, f.view(n, H, W, 3), S, finisher))
            cls = _pick_classes(ppnet, _eval_outputs(ppnet, torch.cat(x0)), None, top_classes, B)
            del x0
        else:
            cls = _explain_classes(classes, B, Cn, ids.device)
        for s0 in range(0, B * E, chunk):
            n = min(chunk, B * E - s0)
            f = ops.synth_render(spec, rows[s0:s0 + n], ids_rep[s0:s0 + n].contiguous(), out=buf[:n * frame])
            x = D.partsworld_view(spec, f.view(n, H, W, 3), S, finisher)
            logits[s0:s0 + n] = torch.cat([r.logits for r in forward_groups(ppnet, x, int(batch_size or B))])
    M = cls.shape[1]
    cols = cls[:, None, :].expand(B, E, M).reshape(B * E, M)
    if value == "prob":
        val = torch.stack([ops.class_prob(logits, cols[:, m].contiguous()) for m in range(M)], dim=1)
    else:
        val = torch.where(cols >= 0, logits.gather(1, cols.clamp(min=0).long()), torch.full((), float("nan"), device=ids.device))
    return Interventions(edits, changed, val.reshape(B, E, M).contiguous(), cls, scene, logits.argmax(1).to(torch.int32).reshape(B, E), kind=value)


def _attribution_mass(ppnet, x, outs, partmap, K, cls, order, ids, **order_kwargs):
    if order not in PART_ORDERS:
        raise ValueError(f"part_attribution: order must be one of {PART_ORDERS}, got {order!r}"
                         + (" (the 'shap' players are grid cells: no pixel map is provided, as pixel_scores says)" if order in GAME_ORDERS else ""))
    score = pixel_scores(ppnet, x, outs, cls, order, image_ids=ids, **order_kwargs)
    return part_mass(score.contiguous(), partmap, cls.shape[1], K, device=True)


@torch.no_grad()
def part_attribution(ppnet, x, ids, spec, cls, order, **order_kwargs):
    """(pos, neg fp64 [B * M, 3 + K], count int32 [B * M, 3 + K], nonfinite int32 [B * M]): the mass of the order's pixel map
    (pixel_scores: 'evidence', 'attention', 'random', 'rise' or 'ig'; 'shap' is refused by name) for the classes cls int32 [B, M] on every
    primitive of the PartsWorld images ids, x [B, 3, S, S] being their square view.  One eval forward, pixel_scores, one
    ppf_synth_render(partmap=True) of the ids, one ppf_part_mass.  order_kwargs: baseline, seed, batch_size, scratch_bytes, rise, ig."""
    from . import data as D
    from . import ops
    if order not in PART_ORDERS:
        _attribution_mass(ppnet, x, None, None, spec.parts, cls, order, None)
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 4:
        raise RuntimeError("part_attribution needs a CUDA/HIP batch [B, 3, S, S] (no CPU fallback path; part_mass(device=False) is the host referee)")
    x, ids = x.float().contiguous(), D._device_ids(ids).contiguous()
    _, partmap = ops.synth_render(spec, ops.synth_scene(spec, ids), ids, partmap=True)
    return _attribution_mass(ppnet, x, _eval_outputs(ppnet, x), partmap, spec.parts, cls, order, ids, **order_kwargs)


def _avg_ranks(v):
    """fp64 ranks 1 .. n of v, equal values sharing the mean of their ranks."""
    v = np.asarray(v, dtype=np.float64)
    order = np.argsort(v, kind="stable")
    ranks, sv = np.empty(v.size, dtype=np.float64), v[order]
    i = 0
    while i < v.size:
        j = i
        while j + 1 < v.size and sv[j + 1] == sv[i]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return ranks


def spearman(a, b):
    """Spearman's rho of two vectors (Pearson of the average ranks, fp64); None when there are fewer than two entries or either is constant."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size < 2 or a.size != b.size or (a == a[0]).all() or (b == b[0]).all():
        return None
    ra, rb = _avg_ranks(a) - (a.size + 1) / 2.0, _avg_ranks(b) - (b.size + 1) / 2.0
    return float(_ordered_sum(ra * rb) / np.sqrt(_ordered_sum(ra * ra) * _ordered_sum(rb * rb)))


def _descending(key, live):
    """The live indices by descending key, equal keys by smaller index."""
    idx = np.flatnonzero(live)
    return idx[np.argsort(-np.asarray(key, dtype=np.float64)[idx], kind="stable")]


def _deletion_area(v0, values, V):
    """Trapezoid over j / V of the V + 1 values (the unedited one, then after j = 1 .. V parts were hidden), fp64."""
    c = np.concatenate([[float(v0)], np.asarray(values, dtype=np.float64)[:V]])
    return float(((c[1:] + c[:-1]) * 0.5).sum() / V)


def part_agreement_from_rows(rows):
    """The report of part_agreement from all rows, on the host (numpy, fp64, image-id order: the result does not depend on the order the
    rows arrive in).  rows: image_ids [N], labels [N], value fp [N, E], pred [N, E] and changed [N, E] of the standard edit list (E = K + 5:
    COPY, part k off, all parts off, distractors off, flat background, counterfactual), visible [N, K], class_parts [C, K], view S, and
    orders {order: dict(pos, neg fp64 [N, 3 + K], count [N, 3 + K], nonfinite [N], deleted fp [N, K])} with deleted[:, j] the value after
    the j + 1 parts of largest mass were hidden; oracle, reverse [N, K] the same for descending and ascending importance.
    model: importance[k] = the mean of v - v(part k off) over the images where that edit changed the image (importance_images[k] of
    them) next to discriminative_parts (the columns of class_parts that are not constant); parts_share = (v - v(all parts off)) / v;
    distractor_effect, background_effect = |v - v(edit)| and how often the arg-max class changes under each; counterfactual_follows =
    the share predicted as (label + 1) % C on the counterfactual among the images predicted as their label whose counterfactual differs.
    per_order: single_deletion = the mean Spearman rho between the signed part mass pos - neg and the importance over an image's visible
    parts (images where it is undefined are counted, not hidden); top_part_match; mass_share of the positive mass on parts, body,
    distractors and background next to area_share = count / S^2; part_deletion = the mean areas of the order, the oracle and its reverse
    and normalised = (A_reverse - A_order) / (A_reverse - A_oracle), None when the denominator is 0."""
    ids = np.asarray(rows["image_ids"]).reshape(-1)
    at = np.argsort(ids, kind="stable")
    take = lambda v: np.asarray(v)[at]
    value, pred, changed = take(rows["value"]).astype(np.float64), take(rows["pred"]).astype(np.int64), take(rows["changed"]).astype(np.int64)
    labels, visible = take(rows["labels"]).astype(np.int64), take(rows["visible"]) != 0
    table, S = np.asarray(rows["class_parts"]), int(rows["view"])
    N, K, C = ids.size, visible.shape[1], table.shape[0]
    if value.shape != (N, K + 5):
        raise ValueError(f"part_agreement_from_rows: value must be [N, K + 5] = [{N}, {K + 5}] (the standard edit list), got {value.shape}")
    v0, a_all, a_dist, a_bg, a_cf = value[:, 0], K + 1, K + 2, K + 3, K + 4
    imp = v0[:, None] - value[:, 1:K + 1]                                     # [N, K]
    live = visible & (changed[:, 1:K + 1] == 1)
    mean = lambda v: _ordered_mean(v)[0]
    eligible = (pred[:, 0] == labels) & (changed[:, a_cf] == 1)
    model = dict(importance=[mean(imp[live[:, k], k]) for k in range(K)], importance_images=[int(live[:, k].sum()) for k in range(K)],
                 discriminative_parts=[int(k) for k in range(K) if (table[:, k] != table[0, k]).any()],
                 parts_share=_ratio_mean(v0 - value[:, a_all], v0)[0],
                 distractor_effect=mean(np.abs(v0 - value[:, a_dist])), background_effect=mean(np.abs(v0 - value[:, a_bg])),
                 distractor_changes_prediction=mean(pred[:, a_dist] != pred[:, 0]), background_changes_prediction=mean(pred[:, a_bg] != pred[:, 0]),
                 accuracy=mean(pred[:, 0] == labels), counterfactual_images=int(eligible.sum()),
                 counterfactual_follows=mean(pred[eligible, a_cf] == (labels[eligible] + 1) % C))
    nvis = live.sum(1)
    areas = lambda dv: np.array([_deletion_area(v0[i], dv[i], nvis[i]) for i in range(N) if nvis[i] > 0], dtype=np.float64)
    a_oracle, a_reverse = mean(areas(take(rows["oracle"]))), mean(areas(take(rows["reverse"])))
    per_order = {}
    for order, f in rows["orders"].items():
        pos, neg, cnt = take(f["pos"]).astype(np.float64), take(f["neg"]).astype(np.float64), take(f["count"]).astype(np.float64)
        signed = pos[:, 3:] - neg[:, 3:]
        rho, undefined, match = [], 0, []
        for i in range(N):
            k = np.flatnonzero(live[i])
            r = spearman(signed[i, k], imp[i, k])
            undefined += r is None
            rho += [] if r is None else [r]
            if k.size:
                match.append(_descending(signed[i], live[i])[0] == _descending(imp[i], live[i])[0])
        total = pos.sum(1)
        groups = dict(parts=pos[:, 3:].sum(1), body=pos[:, 2], distractors=pos[:, 1], background=pos[:, 0])
        area = dict(parts=cnt[:, 3:].sum(1), body=cnt[:, 2], distractors=cnt[:, 1], background=cnt[:, 0])
        a_order = mean(areas(take(f["deleted"])))
        den = None if a_oracle is None or a_reverse is None else a_reverse - a_oracle
        per_order[order] = dict(
            single_deletion=mean(rho), defined=len(rho), undefined=int(undefined), top_part_match=mean(match),
            mass_share={g: _ratio_mean(v, total)[0] for g, v in groups.items()}, zero_mass_images=int((total <= 0).sum()),
            area_share={g: mean(v / float(S * S)) for g, v in area.items()}, distractor_mass=_ratio_mean(groups["distractors"], total)[0],
            distractor_effect=model["distractor_effect"], nonfinite_images=int((take(f["nonfinite"]) > 0).sum()),
            part_deletion=dict(order=a_order, oracle=a_oracle, reverse=a_reverse, normalised=None if not den else (a_reverse - a_order) / den))
    return dict(images=int(N), parts=int(K), model=model, per_order=per_order)


def _cumulative_masks(key, live):
    """int32 [B, K] PARTS_OFF masks: entry j hides the j + 1 live parts of largest key (equal keys: the smaller k); the parts that are not
    live follow (hiding them changes nothing), so entry V - 1 and every later one hide all V live parts."""
    k = torch.where(live, key.double(), torch.full((), float("-inf"), dtype=torch.float64, device=key.device))
    order = torch.sort(k, dim=1, descending=True, stable=True)[1]
    return torch.cumsum(torch.ones_like(order) << order, dim=1).to(torch.int32)        # distinct bits: the sum is the union


@torch.no_grad()
def part_agreement(ppnet, loader, spec, orders=("evidence", "attention", "random"), value="prob", against_label=False, max_images=0, per_image=False,
                   pass_images=16, rise=None, ig=None, seed=0, batch_size=None, scratch_bytes=1 << 30):
    """Explanations against the truth over a PartsWorld split.  loader yields (x, labels, ids) in the square view; the images are
    regrouped into passes of pass_images (tooling.regroup), so the result does not depend on the loader's batch size.  Per pass: one eval
    forward and the class pick (the predicted class, or the label with against_label), part_interventions with the standard list, one
    partmap render, per order one pixel_scores + ppf_part_mass, then one more part_interventions over the cumulative PARTS_OFF masks of
    every order, the oracle (descending importance) and its reverse.  The rows stay on the device and are read once at the end;
    part_agreement_from_rows holds the arithmetic.  Returns its dict plus settings and, with per_image, per_image = the rows."""
    from . import data as D
    from . import ops
    orders = tuple(orders)
    for order in orders:
        if order not in PART_ORDERS:
            _attribution_mass(ppnet, None, None, None, spec.parts, None, order, None)
    K, keep = spec.parts, []
    for x, y, ids in regroup(batches_with_ids(loader, max_images), int(pass_images)):
        x = (x if x.is_cuda else x.cuda()).float().contiguous()
        ids, y = ids.to(x.device).contiguous(), torch.as_tensor(y).to(x.device, torch.int64)
        B = x.shape[0]
        outs = _eval_outputs(ppnet, x)
        cls = _pick_classes(ppnet, outs, y if against_label else None, 1, B)
        iv = part_interventions(ppnet, spec, ids, classes=cls, value=value, batch_size=batch_size, scratch_bytes=scratch_bytes)
        _, partmap = ops.synth_render(spec, iv.scene, ids, partmap=True)
        val = iv.value[:, :, 0]
        live = iv.changed[:, 1:K + 1] == 1
        imp = val[:, :1] - val[:, 1:K + 1]
        row = dict(image_ids=ids, labels=y, classes=cls[:, 0], value=val, pred=iv.pred, changed=iv.changed,
                   visible=iv.scene[:, D.SYNTH_PART0:D.SYNTH_PART0 + D.SYNTH_PRIM_WORDS * K:D.SYNTH_PRIM_WORDS].contiguous())
        masks = [_cumulative_masks(imp, live), _cumulative_masks(-imp, live)]
        for order in orders:
            pos, neg, cnt, bad = _attribution_mass(ppnet, x, outs, partmap, K, cls, order, ids, seed=seed, batch_size=batch_size,
                                                   scratch_bytes=scratch_bytes, rise=rise, ig=ig)
            row.update({f"{order}.pos": pos, f"{order}.neg": neg, f"{order}.count": cnt, f"{order}.nonfinite": bad})
            masks.append(_cumulative_masks(pos[:, 3:] - neg[:, 3:], live))
        m = torch.cat(masks, dim=1)                                           # [B, (2 + orders) * K]
        dele = part_interventions(ppnet, spec, ids, classes=cls, value=value, batch_size=batch_size, scratch_bytes=scratch_bytes,
                                  edits=torch.stack([torch.full_like(m, D.EDIT_PARTS_OFF), m], dim=2)).value[:, :, 0]
        row.update(oracle=dele[:, :K], reverse=dele[:, K:2 * K], **{f"{o}.deleted": dele[:, (2 + j) * K:(3 + j) * K] for j, o in enumerate(orders)})
        keep.append(row)
    flat = read_rows(keep, "part_agreement")                                  # the one read
    rows = {k: v for k, v in flat.items() if "." not in k}
    rows.update(orders={o: {k: flat[f"{o}.{k}"] for k in ("pos", "neg", "count", "nonfinite", "deleted")} for o in orders},
                class_parts=D.partsworld_class_table(spec), view=int(ppnet.img_size))
    out = part_agreement_from_rows(rows)
    out["settings"] = dict(orders=list(orders), value=value, against_label=bool(against_label), pass_images=int(pass_images), seed=int(seed),
                           rise={**RISE_DEFAULTS, **(rise or {})} if "rise" in orders else None, ig={**IG_DEFAULTS, **(ig or {})} if "ig" in orders else None,
                           img_size=int(ppnet.img_size))
    if per_image:
        out["per_image"] = rows
    return out
