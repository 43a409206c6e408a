"""Explain predictions: for every image of a split, the prototypes that carry the logit of its top classes (ProtoPNet's "local
analysis"; the reference has no such pass -- its main_visualize.py draws every prototype of a chosen class and never ranks evidence).

Per batch one eval forward and one `ppf_explain_topk` launch per branch (interpret.explain): the ranked prototypes, their share of the
logit, the grid cell each of them fired at and, with --render, their activation maps come back; nothing of size [B, P] is read.

    python -m protopformer_amd.explain --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split train|test] [--topk 10]
                                       [--top_classes 1] [--against] [--max_images N] [--bank OUT/prototype_bank.npz] [--stats OUT/prototype_stats.npz] [--render]
                                       + the model flags of train.py

writes OUT/explanations.jsonl, one line per image (Explanation.report's record plus image_id, image path and label); with
--bank every listed prototype carries its nearest training patches from the prototype bank (python -m protopformer_amd.bank); with
--stats its activation's percentile among all and among the own-class images of the prototype statistics (python -m
protopformer_amd.protostats); with
--render also img_<id>/class<c>_rank<r>.jpg: the activation overlay of the rank-r local prototype with its high-activation box."""
import json
import os

import numpy as np
import torch


def get_args_parser():
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer local analysis: the prototypes behind each image's top classes", "train", "explained")
    a = p.add_argument
    a("--topk", type=int, default=10, help="prototypes listed per (image, class) and branch (1..64)")
    a("--top_classes", type=int, default=1, help="classes explained per image, by logit (1..8)")
    a("--against", action="store_true", default=False, help="rank the strongest evidence against each class instead of for it")
    a("--bank", type=str, default="", metavar="PATH", help="prototype_bank.npz of the bank tool: attach each prototype's nearest training patches")
    a("--stats", type=str, default="", metavar="PATH", help="prototype_stats.npz of the protostats tool: attach each activation's percentiles")
    a("--render", action="store_true", default=False, help="also write img_<id>/class<c>_rank<r>.jpg activation overlays")
    return p


def view_images_bgr(x, mean, std):
    """The un-normalised uint8 images [B, H, W, 3] in B, G, R order of a normalised fp32 batch [B, 3, H, W] (host array)."""
    mean, std = (torch.as_tensor(np.asarray(v, dtype=np.float32), device=x.device).reshape(1, 3, 1, 1) for v in (mean, std))
    rgb = ((x.float() * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8)
    return rgb.permute(0, 2, 3, 1).flip(-1).cpu().numpy()


def render_overlays(out_dir, host, views_bgr, image_ids):
    """img_<id>/class<c>_rank<r>.jpg for every filled local slot of a host Explanation: interpret.activation_overlay of the returned
    map on the view image, with the high-activation box drawn.  Returns the written paths."""
    from PIL import Image

    from .interpret import activation_overlay, draw_rect
    f, written = host.local, []
    for b in range(f["classes"].shape[0]):
        d = os.path.join(out_dir, f"img_{int(image_ids[b])}")
        for m in range(f["classes"].shape[1]):
            c = int(f["classes"][b, m])
            rank = 0
            for k in range(f["prototypes"].shape[2]):
                if c < 0 or f["prototypes"][b, m, k] < 0:
                    continue
                over, (y0, y1, x0, x1), _ = activation_overlay(views_bgr[b], f["maps"][b, m, k], host.img_size)
                over = draw_rect(over, (x0, y0), (x1 - 1, y1 - 1), (0, 255, 255))
                os.makedirs(d, exist_ok=True)
                path = os.path.join(d, f"class{c}_rank{rank}.jpg")
                Image.fromarray(over[:, :, ::-1]).save(path)
                written.append(path)
                rank += 1
    return written


def main(args, model=None, loader=None, index=None):
    """model / loader / index: ready ones, the index {image id: (path, label)} (tests, notebooks); by default tooling.tool_setup builds them."""
    from . import data as D
    from .bank import image_index
    from .interpret import explain
    from .tooling import batches_with_ids, tool_setup
    model, loader, ds, device = tool_setup(args, "explain", model, loader)
    if ds is not None:
        index = image_index(ds)
    bank = dict(np.load(args.bank)) if args.bank else None
    stats = None
    if args.stats:
        from .protostats import load_stats
        stats = load_stats(args.stats)
    index = index or {}
    os.makedirs(args.output_dir, exist_ok=True)
    path, seen, rendered = os.path.join(args.output_dir, "explanations.jsonl"), 0, 0
    with open(path, "w") as out:
        for x, y, ids in batches_with_ids(loader, args.max_images):
            ids = ids.cpu().numpy()
            ex = explain(model, x if x.is_cuda else x.to(device), top_classes=args.top_classes, topk=args.topk, against=args.against, maps=args.render)
            host = ex.cpu()
            labels = np.asarray(torch.as_tensor(y).cpu())
            for rec in host.report(bank=bank, stats=stats):
                b = rec["image"]
                file, _ = index.get(int(ids[b]), (None, None))
                rec.update(image_id=int(ids[b]), image=file, label=int(labels[b]) if labels.ndim == 1 else None)
                out.write(json.dumps(rec) + "\n")
            if args.render:
                rendered += len(render_overlays(args.output_dir, host, view_images_bgr(x, D.IMAGENET_DEFAULT_MEAN, D.IMAGENET_DEFAULT_STD), ids))
            seen += x.shape[0]
    print(f"explained {seen} {args.split} images: {path}" + (f", {rendered} overlays under {args.output_dir}" if args.render else ""), flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
