"""Prototype bank: for every prototype, the K image patches of a whole data set that activate it most, and the projection of each
prototype onto the nearest of them (the ranking and the "push" step ProtoPNet-family tools offer; the reference has neither).

The ranking is a running top-K kept on the device: per batch one `ppf_proto_topk_merge` launch per branch folds the pooled
activations `ppf_proto_fwd` already produced (and the token each max-pool selected) into per-prototype lists, and captures the latent
token of the best entry in the same pass.  Nothing of size [B, P] is read back and no latent token is kept beyond the winners.

    python -m protopformer_amd.bank --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--topk 10] [--split train]
                                    [--all-classes] [--gallery] [--project [--save-projected PATH]]   + the model flags of train.py

writes OUT/prototype_bank.npz (the arrays of PrototypeBank.result) and OUT/prototype_bank.json (per prototype: branch, class, and the
ranked entries with image path, label, activation, grid cell and pixel box)."""
import argparse
import json
import math
import os

import numpy as np
import torch

from . import ops

BRANCHES = ("local", "global")
PARAM_OF = {"local": "prototype_vectors", "global": "prototype_vectors_global"}
MAX_BATCH = 1024                       # ppf_proto_topk_merge accepts 1 <= B <= 1024: larger batches are merged in slices


class PrototypeBank:
    """Running per-prototype top-K over everything passed to update() / merge().

    Order: larger activation first, equal activations by smaller image id, so the result does not depend on the batch size or on the
    order of the batches.  Image ids must be non-negative int32 and unique across all updates (not checked).
    class_specific: an image is offered only to the prototypes of its own class (ProtoPNet's push)."""

    def __init__(self, ppnet, topk=10, class_specific=True):
        if not 1 <= int(topk) <= 64:
            raise ValueError(f"PrototypeBank: topk={topk} outside [1, 64]")
        self.ppnet, self.topk, self.class_specific = ppnet, int(topk), bool(class_specific)
        dev = ppnet.prototype_vectors.device
        if dev.type != "cuda":
            raise RuntimeError("PrototypeBank lives on the GPU: move the model to cuda first (no CPU fallback path)")
        Dp = ppnet.prototype_shape[1]
        self.num = {"local": ppnet.num_prototypes, "global": ppnet.num_prototypes_global}
        self.ppc = {"local": ppnet.num_prototypes_per_class, "global": ppnet.global_proto_per_class}
        self.side = int(round(math.sqrt(ppnet.num_patches)))
        self.state = {}
        for br in BRANCHES:
            P = self.num[br]
            s = dict(val=torch.empty((P, self.topk), dtype=torch.float32, device=dev), img=torch.empty((P, self.topk), dtype=torch.int32, device=dev),
                     pos=torch.empty((P, self.topk), dtype=torch.int32, device=dev), best_feat=ops.zeros((P, Dp), torch.float32, dev))
            ops.proto_topk_init(s["val"], s["img"], s["pos"])
            self.state[br] = s

    # ---------------------------------------------------------------------------------------------- feeding
    def _ids(self, ids, B, device):
        ids = torch.as_tensor(ids)
        if ids.shape != (B,):
            raise ValueError(f"PrototypeBank: {B} image ids expected, got shape {tuple(ids.shape)}")
        return ids.to(device=device, dtype=torch.int32).contiguous()

    @torch.no_grad()
    def update(self, x, labels, ids):
        """One batch through the model's eval branch (PPNet.eval_branches), then both branches into the lists."""
        r = self.ppnet.eval_branches(x)
        self.merge("local", r.act_max_local, r.argmax, r.idx, r.f, labels, ids)
        self.merge("global", r.act_max_global, None, None, r.f, labels, ids)

    def merge(self, branch, act_max, argmax, idx, f, labels, ids):
        """Low-level: fold one batch's pooled activations of `branch` into its lists.  act_max [B, P] fp32, argmax [B, P] int32 and
        idx [B, k] int32 (both None for 'global'), f [B, 1 + k, Dp] fp32 latent tokens (cls first), labels int64 [B], ids [B]."""
        if branch not in BRANCHES:
            raise ValueError(f"PrototypeBank.merge: branch must be one of {BRANCHES}")
        if (branch == "global") != (argmax is None):
            raise ValueError("PrototypeBank.merge: the local branch comes with argmax / idx, the global branch without")
        s, B = self.state[branch], act_max.shape[0]
        ids = self._ids(ids, B, act_max.device)
        labels = torch.as_tensor(labels).to(device=act_max.device, dtype=torch.int64).contiguous()
        ppc = self.ppc[branch] if self.class_specific else 0
        t0 = 1 if branch == "local" else 0
        f = f.contiguous()
        for b in range(0, B, MAX_BATCH):
            e = min(B, b + MAX_BATCH)
            ops.proto_topk_merge(act_max[b:e].contiguous(), None if argmax is None else argmax[b:e].contiguous(),
                                 None if idx is None else idx[b:e].contiguous(), f[b:e], t0, labels[b:e], ids[b:e], ppc,
                                 s["val"], s["img"], s["pos"], s["best_feat"])

    # ---------------------------------------------------------------------------------------------- reading
    def result(self):
        """One host read.  {'local' | 'global': dict(values [P, K] fp32, image_ids [P, K], grid_pos [P, K] (index in the side x side patch
        grid, -1 on the global branch), filled [P] = number of valid entries)} as numpy arrays; unfilled slots hold -inf / -1 / -1."""
        from .tooling import read_once
        host = read_once({(br, k): self.state[br][k] for br in BRANCHES for k in ("val", "img", "pos")})
        return {br: dict(values=host[br, "val"], image_ids=host[br, "img"], grid_pos=host[br, "pos"],
                         filled=(host[br, "img"] >= 0).sum(axis=1).astype(np.int32)) for br in BRANCHES}

    @torch.no_grad()
    def project_(self, ppnet=None, branches=BRANCHES):
        """Replace every prototype that has at least one entry by the latent token of its best one.  Goes through load_state_dict,
        the path a parameter load takes (the flat store's bf16 shadows are invalidated there).  Returns the number projected."""
        ppnet = self.ppnet if ppnet is None else ppnet
        n, new = 0, {}
        for br in branches:
            s = self.state[br]
            p = getattr(ppnet, PARAM_OF[br])
            filled = s["img"][:, 0] >= 0
            cur = p.detach().reshape(self.num[br], -1)
            new[PARAM_OF[br]] = torch.where(filled[:, None], s["best_feat"].to(cur.device), cur).reshape(p.shape)
            n += int(filled.sum())
        ppnet.load_state_dict(new, strict=False)             # in-place copies into the flat store's views + invalidation of its shadows
        return n

    def state_dict(self):
        sd = {"topk": self.topk, "class_specific": self.class_specific}
        for br in BRANCHES:
            for k, v in self.state[br].items():
                sd[f"{br}.{k}"] = v.detach().cpu()
        return sd

    def load_state_dict(self, sd):
        if int(sd["topk"]) != self.topk or bool(sd["class_specific"]) != self.class_specific:
            raise ValueError(f"PrototypeBank.load_state_dict: saved with topk={sd['topk']} class_specific={sd['class_specific']}, this bank has "
                             f"topk={self.topk} class_specific={self.class_specific}")
        for br in BRANCHES:
            for k, v in self.state[br].items():
                t = sd[f"{br}.{k}"]
                if t.shape != v.shape or t.dtype != v.dtype:
                    raise ValueError(f"PrototypeBank.load_state_dict: {br}.{k} is {tuple(t.shape)} {t.dtype}, expected {tuple(v.shape)} {v.dtype}")
                v.copy_(t)


# ------------------------------------------------------------------------------------------------ the report
def image_index(ds):
    """{image id: (file path, label)} of a data.Cub2011 (its own ids) or of StanfordCars / Dogs (position in the data set); a
    data.PartsWorld has no files: its entries read 'partsworld:<id>'."""
    if hasattr(ds, "original") and hasattr(ds, "spec"):
        return {int(i): (f"partsworld:{int(i)}", int(t)) for i, t in zip(ds.ids, ds.labels)}
    if hasattr(ds, "data") and hasattr(ds, "base_folder"):
        return {int(i): (os.path.join(ds.root, ds.base_folder, fp), int(t) - 1) for i, fp, t in ds.data}
    if hasattr(ds, "_samples"):
        return {i: (p, int(t)) for i, (p, t) in enumerate(ds._samples)}
    if hasattr(ds, "_flat_breed_images"):
        return {i: (os.path.join(ds.images_folder, n), int(t)) for i, (n, t) in enumerate(ds._flat_breed_images)}
    raise TypeError(f"image_index: do not know where {type(ds).__name__} keeps its file list")


def bank_report(result, index, ppc, side, patch_size):
    """The JSON document of the tool from a PrototypeBank.result() dict: {'topk', 'side', 'patch_size', 'prototypes': [{'branch',
    'prototype', 'class', 'entries': [{'rank', 'image_id', 'image', 'label', 'activation', 'grid_row', 'grid_col', 'box'}]}]}.
    index: {image id: (path, label)}; ppc: {'local' | 'global': prototypes per class}; box = [x0, y0, x1, y1] pixels in the
    view-transformed image, null on the global branch (as grid_row / grid_col)."""
    from .interpret import patch_box
    protos = []
    for br in BRANCHES:
        r = result[br]
        for p in range(r["values"].shape[0]):
            entries = []
            for k in range(int(r["filled"][p])):
                iid, gp = int(r["image_ids"][p, k]), int(r["grid_pos"][p, k])
                path, label = index.get(iid, (None, None))
                entries.append(dict(rank=k, image_id=iid, image=path, label=label, activation=float(r["values"][p, k]),
                                    grid_row=gp // side if gp >= 0 else None, grid_col=gp % side if gp >= 0 else None,
                                    box=list(patch_box(gp, side, patch_size)) if gp >= 0 else None))
            protos.append({"branch": br, "prototype": p, "class": p // ppc[br], "entries": entries})
    topk = int(result[BRANCHES[0]]["values"].shape[1])
    return dict(topk=topk, side=int(side), patch_size=int(patch_size), prototypes=protos)


def write_bank(out_dir, result, index, ppc, side, patch_size):
    """prototype_bank.npz (<branch>_<array> of result) + prototype_bank.json (bank_report) under out_dir; returns the two paths."""
    os.makedirs(out_dir, exist_ok=True)
    npz, js = os.path.join(out_dir, "prototype_bank.npz"), os.path.join(out_dir, "prototype_bank.json")
    np.savez(npz, **{f"{br}_{k}": v for br in BRANCHES for k, v in result[br].items()})
    with open(js, "w") as f:
        json.dump(bank_report(result, index, ppc, side, patch_size), f, indent=1)
    return npz, js


def write_gallery(out_dir, result, index, view_transform, side, patch_size, branch="local", original=None):
    """proto_<p>/rank<r>.jpg: the view-transformed image of every entry with its patch rectangle drawn.  original: image id -> uint8 HWC
    frame of a data set without files (data.PartsWorld.original); None: the file the index names.  Returns the written paths."""
    from PIL import Image

    from .data import default_loader
    from .interpret import draw_rect, patch_box
    r, written = result[branch], []
    for p in range(r["values"].shape[0]):
        for k in range(int(r["filled"][p])):
            iid = int(r["image_ids"][p, k])
            view = np.asarray(view_transform(Image.fromarray(original(iid)) if original is not None else default_loader(index[iid][0])))
            gp = int(r["grid_pos"][p, k])
            if gp >= 0:
                x0, y0, x1, y1 = patch_box(gp, side, patch_size)
                view = draw_rect(view, (x0, y0), (x1 - 1, y1 - 1), (255, 255, 0))
            d = os.path.join(out_dir, f"proto_{p}")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(view).save(os.path.join(d, f"rank{k}.jpg"))
            written.append(os.path.join(d, f"rank{k}.jpg"))
    return written


# ------------------------------------------------------------------------------------------------ the tool
def get_args_parser():
    from .train import get_args_parser as train_parser
    p = argparse.ArgumentParser("ProtoPFormer prototype bank: dataset-wide nearest patches per prototype", parents=[train_parser()])
    a = p.add_argument
    a("--split", type=str, default="train", choices=["train", "test"], help="which split is ranked (no augmentation either way)")
    a("--topk", type=int, default=10, help="entries kept per prototype (1..64)")
    a("--all-classes", action="store_true", default=False, help="offer every image to every prototype, not only to those of its class")
    a("--project", action="store_true", default=False, help="replace every prototype by the latent patch of its best entry and save the model")
    a("--save-projected", type=str, default="", metavar="PATH", help="where --project writes (default <output_dir>/checkpoints/projected.pth)")
    a("--gallery", action="store_true", default=False, help="also write proto_<p>/rank<r>.jpg with the patch rectangle drawn")
    return p


def main(args, model=None):
    from . import engine as E
    from .interpret import nearest_patches
    from .tooling import eval_loader, load_for_eval, model_from_args
    from .train import set_seed
    set_seed(args.seed)
    device = torch.device(args.device)
    ds, nb_classes, loader = eval_loader(args, device)
    model = load_for_eval(model_from_args(args, nb_classes) if model is None else model, args, device)
    bank = nearest_patches(model, loader, topk=args.topk, class_specific=not args.all_classes)
    result = bank.result()
    index = image_index(ds)
    patch = model.img_size // bank.side
    npz, js = write_bank(args.output_dir, result, index, bank.ppc, bank.side, patch)
    print(f"prototype bank over {len(ds)} {args.split} images: {npz} {js}", flush=True)
    if args.gallery:
        written = write_gallery(args.output_dir, result, index, ds.transform, bank.side, patch, original=getattr(ds, "original", None))
        print(f"gallery: {len(written)} images under {args.output_dir}", flush=True)
    if args.project:
        n = bank.project_(model)
        path = args.save_projected or os.path.join(args.output_dir, "checkpoints", "projected.pth")
        E.save_checkpoint(path, model, E.FlatAdamW(model), None, 0, args=args)
        print(f"projected {n} prototypes onto their nearest patches: {path}", flush=True)
    return bank


if __name__ == "__main__":
    cli_args = get_args_parser().parse_args()
    main(cli_args)
