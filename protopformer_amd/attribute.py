"""Which pixels carry the class?  Integrated gradients (Sundararajan et al., 2017) of the class logit over a split: per image the
attribution of every pixel, (x - baseline) times the gradient averaged along the straight path from the baseline (the data-set mean
colour) to the image, summed over the cells of the patch grid; and the completeness gap, how far the attributions of an image are from
adding up to logit(x) - logit(baseline).  The token reservation's top-k makes the model discontinuous along the path, so that gap is a
finding, not an error bound.  The reference has no such pass.

Per batch two eval forwards (the image and the baseline image), per path step one `ppf_ig_point`, one forward + backward and one
`ppf_ig_accumulate` per class column, and one `ppf_ig_finish` (interpret.integrated_gradients); per batch one host read.

    python -m protopformer_amd.attribute --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split test] [--steps 32]
                                         [--rule midpoint] [--top_classes 1] [--against_label] [--max_images N] [--save-maps]
                                         + the model flags of train.py

writes OUT/attributions.json: the settings, per image and class the logit at the image (`value`) and at the baseline (`value_base`),
the summed attribution (`total`), their gap (`delta`) and the ten cells with the largest attribution with their pixel boxes; overall
the mean of |delta| / |value - value_base|.  With --save-maps also OUT/attributions.npz: the cell scores [N, M, G] and the
channel-summed pixel maps [N, M, H, W] with the image ids and classes.  No rendering."""
import os

import numpy as np
import torch

TOP_CELLS = 10


def get_args_parser():
    from .interpret import IG_DEFAULTS, IG_RULES
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer attribution: integrated gradients of the class logit", "test", "attributed")
    a = p.add_argument
    a("--steps", type=int, default=IG_DEFAULTS["steps"], help="path steps (one forward and backward each, per class column)")
    a("--rule", type=str, default=IG_DEFAULTS["rule"], choices=list(IG_RULES), help="quadrature of the path integral")
    a("--top_classes", type=int, default=1, help="attribute the top M classes of every image")
    a("--against_label", action="store_true", default=False, help="attribute the logit of the image's label instead of its top classes")
    a("--save-maps", dest="save_maps", action="store_true", default=False, help="also write attributions.npz with the cell scores and pixel maps")
    p.set_defaults(seed=0)
    return p


def records(h, image_ids, side, patch, top_cells=TOP_CELLS):
    """The per-image records of a host IntegratedGradients h (IntegratedGradients.cpu()): per class column value, value_base, total,
    delta and the top_cells cells by score (descending, ties to the smaller cell) with their pixel boxes (interpret.patch_box)."""
    from .interpret import patch_box
    delta = h.delta()
    out = []
    for b, image_id in enumerate(image_ids):
        cols = []
        for m in range(h.targets.shape[1]):
            score = h.cell[b, m]
            nan = np.isnan(score)
            best = np.lexsort((np.arange(score.size), np.where(nan, np.float32(0), -score), nan))[:top_cells]
            cols.append(dict(target=int(h.targets[b, m]), value=float(h.value[b, m]), value_base=float(h.value_base[b, m]), total=float(h.total[b, m]),
                             delta=float(delta[b, m]),
                             cells=[dict(cell=int(g), score=float(score[g]), box=[int(v) for v in patch_box(int(g), side, patch)]) for g in best]))
        out.append(dict(image_id=int(image_id), classes=cols))
    return out


def relative_gaps(recs):
    """|delta| / |value - value_base| of every (image, class) of the records whose denominator is not zero, fp64."""
    rows = [(c["delta"], c["value"] - c["value_base"]) for r in recs for c in r["classes"]]
    return np.array([abs(d) / abs(v) for d, v in rows if v != 0 and d == d], dtype=np.float64)


def main(args, model=None, loader=None):
    """model / loader: a ready model and iterable of (x, labels[, ids]) CUDA batches (tests, notebooks); by default tooling.tool_setup builds both."""
    from .interpret import integrated_gradients
    from .tooling import batches_with_ids, tool_setup, write_json
    model, loader, _, _ = tool_setup(args, "attribute", model, loader)
    G = int(model.num_patches)
    side = int(round(G ** 0.5))
    patch = int(model.img_size) // side
    recs, kept = [], dict(cell=[], map=[], image_ids=[], classes=[])
    for x, y, ids in batches_with_ids(loader, args.max_images):
        x = (x if x.is_cuda else x.cuda()).float().contiguous()
        target = ("logit", torch.as_tensor(y).to(x.device)) if args.against_label else None
        found = integrated_gradients(model, x, target=target, top_classes=args.top_classes, steps=args.steps, rule=args.rule)
        pixel_map = found.attribution.sum(2) if args.save_maps else None                         # channel-summed, on the device
        found.attribution = found.attribution[:0]                                                # the pixel tensor itself is not read back
        h = found.cpu()
        ids = ids.cpu().numpy()
        recs += records(h, ids, side, patch)
        if args.save_maps:
            kept["cell"].append(h.cell); kept["map"].append(pixel_map.cpu().numpy()); kept["image_ids"].append(ids); kept["classes"].append(h.targets)
    if not recs:
        raise ValueError("attribute: the loader gave no image")
    gaps = relative_gaps(recs)
    doc = dict(images=len(recs), grid_cells=G, patch=patch,
               settings=dict(steps=args.steps, rule=args.rule, top_classes=args.top_classes, against_label=bool(args.against_label), split=args.split,
                             baseline=0.0),
               mean_relative_gap=float(gaps.mean()) if gaps.size else None, worst_relative_gap=float(gaps.max()) if gaps.size else None,
               per_image=recs)
    path = write_json(args, "attributions.json", doc)
    if args.save_maps:
        np.savez(os.path.join(args.output_dir, "attributions.npz"), **{k: np.concatenate(v) for k, v in kept.items()})
    print(f"integrated gradients of {len(recs)} {args.split} images: {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
