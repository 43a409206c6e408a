"""Are the explanations true?  Deletion / insertion curves (Petsiuk et al., RISE, 2018) over a split: the cells of the patch grid an
explanation names are removed most important first (deletion: the class probability should fall) or shown alone (insertion: it should
come back), under three orders of the cells -- the class evidence of the prototypes ('evidence'), the rollout attention the token
reservation looks at ('attention') and a random order, the control.  On request a fourth: 'rise', the cells ranked by the model-agnostic
saliency the metric was published with (interpret.rise_saliency: forwards of randomly masked images alone), the black-box baseline an
interpretable-by-design model is compared against; and 'ig', the cells ranked by the integrated gradients of the class logit
(interpret.integrated_gradients: one forward and backward per path step), the gradient baseline; and 'shap', the cells ranked by the
Shapley value of their block of cells (interpret.kernel_shap: KernelSHAP, forwards of sampled coalitions alone), at cell resolution only.
The reference has no such pass.

Per batch one eval forward, one `ppf_cell_order` launch per order, and per curve `ppf_patch_perturb`, the model's forwards and
`ppf_class_prob` (interpret.faithfulness); the curves stay on the device until the split is done.

    python -m protopformer_amd.faithfulness --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split test] [--steps 14]
                                            [--orders evidence attention random [rise] [ig] [shap]] [--modes deletion insertion] [--against_label]
                                            [--rise_masks 512] [--rise_cells 7] [--rise_p 0.5] [--ig_steps 32] [--ig_rule midpoint]
                                            [--shap_samples 512] [--shap_cells 7] [--shap_value prob|logit]
                                            [--resolution cell|pixel] [--baseline mean|blur] [--blur_sigma 5] [--blur_radius 5]
                                            [--max_images N] [--seed 0] [--per-image]
                                            + the model flags of train.py

writes OUT/faithfulness.json: the image count, the cell counts, per order and mode the mean curve and its area, and per order the
difference of both areas to the random order's (an explanation is informative when its deletion area lies below and its insertion area
above); with --per-image also OUT/faithfulness.npz (the curves, classes and ids of every image).

--resolution pixel is the metric as published: every order becomes a pixel map (the evidence and attention grids up-sampled as the
overlays are, the RISE saliency and the integrated gradients at their own resolution), the pixels are ranked by `ppf_pixel_order` and
removed by `ppf_pixel_perturb`; the counts are pixels.  --baseline blur replaces a removed pixel by the Gaussian-blurred image
(`ppf_gauss_blur`, --blur_sigma, --blur_radius) instead of the mean colour, at either resolution.  faithfulness.json carries the keys
`resolution`, `baseline` and `blur` only when one of these flags departs from its default."""
import os

import numpy as np


def get_args_parser():
    from .interpret import (BLUR_DEFAULTS, CURVE_MODES, EXTRA_ORDERS, GAME_ORDERS, GRADIENT_ORDERS, IG_DEFAULTS, IG_RULES, ORDER_MODES, RESOLUTIONS,
                            RISE_DEFAULTS, SHAP_DEFAULTS, SHAP_VALUES)
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer faithfulness: deletion / insertion curves of the explanations", "test", "evaluated")
    a = p.add_argument
    a("--steps", type=int, default=14, help="the curves have steps + 1 points: 0, G/steps, ... G cells removed / shown")
    a("--orders", type=str, nargs="+", default=list(ORDER_MODES), choices=list(ORDER_MODES + EXTRA_ORDERS + GRADIENT_ORDERS + GAME_ORDERS),
      help="cell orders to evaluate (random is the control; rise, the black-box baseline, ig, the gradient baseline, and shap, the Shapley "
           "values of blocks of cells, only on request)")
    a("--rise_masks", type=int, default=RISE_DEFAULTS["masks"], help="masks per image of the rise order (one forward each)")
    a("--rise_cells", type=int, default=RISE_DEFAULTS["cells"], help="low-resolution cells per side of a rise mask")
    a("--rise_p", type=float, default=RISE_DEFAULTS["p"], help="probability that a node of a rise mask is on")
    a("--ig_steps", type=int, default=IG_DEFAULTS["steps"], help="path steps of the ig order (one forward and backward each)")
    a("--ig_rule", type=str, default=IG_DEFAULTS["rule"], choices=list(IG_RULES), help="quadrature of the ig order's path integral")
    a("--shap_samples", type=int, default=SHAP_DEFAULTS["samples"], help="coalitions per image of the shap order (one forward each; even, >= 4 cells^2)")
    a("--shap_cells", type=int, default=SHAP_DEFAULTS["cells"], help="players per side of the shap order; must divide the grid side")
    a("--shap_value", type=str, default=SHAP_DEFAULTS["value"], choices=list(SHAP_VALUES), help="the game's value: class probability or class logit")
    a("--modes", type=str, nargs="+", default=list(CURVE_MODES), choices=list(CURVE_MODES))
    a("--resolution", type=str, default=RESOLUTIONS[0], choices=list(RESOLUTIONS), help="remove grid cells, or pixels as the published metric does")
    a("--baseline", type=str, default="mean", choices=["mean", "blur"], help="what a removed pixel becomes: the mean colour or the blurred image")
    a("--blur_sigma", type=float, default=BLUR_DEFAULTS["sigma"], help="standard deviation of the blur baseline, in pixels")
    a("--blur_radius", type=int, default=BLUR_DEFAULTS["radius"], help="radius of the blur baseline's kernel (2 r + 1 taps), at most 16")
    a("--against_label", action="store_true", default=False, help="follow the probability of the image's label instead of its top class")
    a("--per-image", dest="per_image", action="store_true", default=False, help="also write faithfulness.npz with every image's curves")
    p.set_defaults(seed=0)                                 # keys the random order (train.py's --seed, with this tool's default)
    return p


def summarize(result, extra=None):
    """The JSON record of interpret.faithfulness's result: images, counts, grid_cells, orders (mean curve and area per order and mode) and
    vs_random: per other order the two area differences to the random order and whether both have the informative sign.  extra: keys
    appended behind them (main: resolution, baseline, blur when a flag departs from its default)."""
    out = dict(images=int(result["images"]), counts=[int(c) for c in result["counts"]], grid_cells=int(result["grid_cells"]), orders=result["orders"],
               vs_random={})
    rnd = result["orders"].get("random")
    for order, modes in result["orders"].items():
        if rnd is None or order == "random":
            continue
        d = {f"{m}_auc_minus_random": modes[m]["auc"] - rnd[m]["auc"] for m in modes if m in rnd}
        if len(d) == 2:
            d["informative"] = bool(d["deletion_auc_minus_random"] < 0 < d["insertion_auc_minus_random"])
        out["vs_random"][order] = d
    out.update(extra or {})
    return out


def main(args, model=None, loader=None):
    """model / loader: a ready model and iterable of (x, labels[, ids]) CUDA batches (tests, notebooks); by default tooling.tool_setup builds both."""
    from .interpret import BLUR_DEFAULTS, default_counts, faithfulness
    from .tooling import tool_setup, write_json
    model, loader, _, _ = tool_setup(args, "faithfulness", model, loader)
    pixel, blur = args.resolution == "pixel", dict(sigma=args.blur_sigma, radius=args.blur_radius)
    res = faithfulness(model, loader, orders=tuple(args.orders), modes=tuple(args.modes),
                       counts=default_counts(int(model.img_size) ** 2 if pixel else model.num_patches, args.steps),
                       against_label=args.against_label, seed=args.seed, max_images=args.max_images,
                       rise=dict(masks=args.rise_masks, cells=args.rise_cells, p=args.rise_p), ig=dict(steps=args.ig_steps, rule=args.ig_rule),
                       resolution=args.resolution, baseline="blur" if args.baseline == "blur" else 0.0, blur=blur,
                       shap=dict(samples=args.shap_samples, cells=args.shap_cells, value=args.shap_value))
    extra = {}
    if pixel or args.baseline != "mean" or blur != BLUR_DEFAULTS:
        extra = dict(resolution=args.resolution, baseline=args.baseline, blur=blur)
    path = write_json(args, "faithfulness.json", summarize(res, extra))
    if args.per_image:
        arrays = {f"{order}_{mode}": c for order, modes in res["per_image"].items() for mode, c in modes.items()}
        np.savez(os.path.join(args.output_dir, "faithfulness.npz"), counts=np.asarray(res["counts"]), classes=res["classes"], image_ids=res["image_ids"],
                 **arrays)
    print(f"faithfulness of {res['images']} {args.split} images: {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
