"""What about this patch makes it look like that prototype: its colour, its texture or its shape?  The perturbation analysis of Nauta
et al., "This Looks Like That, Because ... Explaining Prototypes for Interpretable Image Recognition" (2021), over a split: one visual
characteristic of every image is suppressed -- hue, saturation, contrast (a colour transform), texture (an edge-preserving bilateral
filter) or shape (a smooth warp) --, the model runs again, and the fall of each prototype's similarity at the same grid cell is its local
importance; weighted over a prototype's own-class images it is the global one.  The reference has no such pass.

Per pass one eval forward and per characteristic one perturbation kernel, the model's forward and one `ppf_because_score` launch
(interpret.because, csrc/because.hip); the rows stay on the device until the split is done.  Passes have a fixed size, so the numbers do
not depend on --batch_size.

    python -m protopformer_amd.because --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split train]
                                       [--characteristics hue saturation contrast texture shape] [--protos own|top]
                                       [--protos_per_image 3] [--branch local|global] [--max_images N] [--per-image] [--save-images N]
                                       [--hue_turn 0.5] [--saturation_factor 0] [--contrast_factor 0.25]
                                       [--texture_radius 4] [--texture_sigma_space 3] [--texture_sigma_range 25]
                                       [--shape_cells 4] [--shape_amplitude 6] [--pass_images 16]
                                       + the model flags of train.py

The default strengths are choices, not tuned values: nobody has run this on a trained checkpoint.

writes OUT/because.json: the parameters, per prototype and overall the importance of every characteristic (the paper's weighted form, the
unweighted mean and the location-free variant), the share of lost cells, the dominant characteristic and the image counts; with
--per-image also OUT/because.npz (the rows); with --save-images N the perturbed views of the first N images as OUT/views/<id>_<name>.jpg."""
import os

import numpy as np
import torch


def get_args_parser():
    from .interpret import BECAUSE_DEFAULTS as D, CHARACTERISTICS, EXPLAIN_BRANCHES
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer: this looks like that, because ... (importance of hue, saturation, contrast, texture, shape)", "train", "analysed")
    a = p.add_argument
    a("--characteristics", type=str, nargs="+", default=list(CHARACTERISTICS), choices=list(CHARACTERISTICS))
    a("--protos", type=str, default="own", choices=["own", "top"],
      help="own: every prototype of the image's label class; top: the strongest prototypes of the predicted class")
    a("--protos_per_image", type=int, default=3, help="prototypes kept per image with --protos top")
    a("--branch", type=str, default="local", choices=list(EXPLAIN_BRANCHES), help="the global branch has no cells: pooled activations only")
    a("--pass_images", type=int, default=16, help="images per pass (fixed, so the result does not depend on --batch_size)")
    a("--per-image", dest="per_image", action="store_true", default=False, help="also write because.npz with every row")
    a("--save-images", dest="save_images", type=int, default=0, metavar="N", help="write the perturbed views of the first N images as JPEGs")
    untuned = " (a choice, not a tuned value)"
    a("--hue_turn", type=float, default=D["hue"], help="turn of the IQ plane as a fraction of a full turn" + untuned)
    a("--saturation_factor", type=float, default=D["saturation"], help="saturation that is left, 0 = grey" + untuned)
    a("--contrast_factor", type=float, default=D["contrast"], help="contrast that is left around the image's mean luma" + untuned)
    a("--texture_radius", type=int, default=D["radius"], help="window radius of the bilateral filter in pixels, 1 .. 8" + untuned)
    a("--texture_sigma_space", type=float, default=D["sigma_space"], help="spatial Gaussian width in pixels" + untuned)
    a("--texture_sigma_range", type=float, default=D["sigma_range"], help="range Gaussian width in 8-bit luma steps" + untuned)
    a("--shape_cells", type=int, default=D["cells"], help="warp grid cells per side, 1 .. 16" + untuned)
    a("--shape_amplitude", type=float, default=D["amplitude"], help="largest node displacement in pixels" + untuned)
    p.set_defaults(seed=0)                                 # keys the warp (train.py's --seed, with this tool's default)
    return p


def params_from_args(args):
    """The `params` of interpret.because from the strength flags."""
    return dict(hue=args.hue_turn, saturation=args.saturation_factor, contrast=args.contrast_factor, radius=args.texture_radius,
                sigma_space=args.texture_sigma_space, sigma_range=args.texture_sigma_range, cells=args.shape_cells, amplitude=args.shape_amplitude)


def summarize(result, args):
    """The JSON record of interpret.characteristic_importance's result (prototype ids as strings)."""
    return dict(images=int(result["images"]), rows=int(result["overall"]["rows"]), characteristics=list(result["characteristics"]), branch=result["branch"],
                settings=dict(split=args.split, protos=args.protos, protos_per_image=args.protos_per_image, pass_images=args.pass_images, seed=args.seed,
                              **params_from_args(args)),
                overall=result["overall"], per_prototype={str(p): v for p, v in sorted(result["per_prototype"].items())})


def save_views(x, ids, names, params, seed, out_dir):
    """The perturbed views of the batch x (and the clean one) as JPEGs: the device perturbs, the host writes."""
    from PIL import Image
    from .interpret import because_params, because_perturb
    p = because_params(params)
    mean, std = (torch.from_numpy(p[k]).to(x.device).reshape(1, 3, 1, 1) for k in ("mean", "std"))
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for name in ("clean",) + tuple(names):
        v = x if name == "clean" else because_perturb(x, name, params, seed, ids)
        u8 = ((v * std + mean).clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
        for j, i in enumerate(ids.tolist()):
            written.append(os.path.join(out_dir, f"{i}_{name}.jpg"))
            Image.fromarray(u8[j]).save(written[-1])
    return written


def main(args, model=None, loader=None):
    """model / loader: a ready model and iterable of (x, labels[, ids]) CUDA batches (tests, notebooks); by default tooling.tool_setup builds both."""
    from .interpret import characteristic_importance
    from .tooling import batches_with_ids, tool_setup, write_json
    model, loader, _, _ = tool_setup(args, "because", model, loader)
    params, names = params_from_args(args), tuple(args.characteristics)
    res = characteristic_importance(model, loader, protos=args.protos, branch=args.branch, characteristics=names, params=params, seed=args.seed,
                                    max_images=args.max_images, pass_images=args.pass_images, protos_per_image=args.protos_per_image,
                                    per_image=args.per_image)
    path = write_json(args, "because.json", summarize(res, args))
    if args.per_image:
        np.savez(os.path.join(args.output_dir, "because.npz"), characteristics=np.asarray(names), **{k: v for k, v in res["rows"].items() if v is not None})
    if args.save_images > 0:
        for x, _, ids in batches_with_ids(loader, args.save_images):
            save_views(x.float().contiguous(), ids, names, params, args.seed, os.path.join(args.output_dir, "views"))
    print(f"because: {res['images']} {args.split} images, {res['overall']['rows']} image-prototype rows: {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
