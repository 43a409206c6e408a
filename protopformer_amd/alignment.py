"""Do the prototypes look where they say they look?  The spatial-misalignment test (Sacha et al., AAAI 2024) over a split: for every
image the strongest local prototypes of its predicted class, each with a box around the peak of its up-sampled activation map; the
share of the pixel gradient of the prototype's activation that falls inside the box (against the box's share of the image area, what
a spatially blind gradient would reach), and an attack that may change only the pixels OUTSIDE the box: how far the activation falls
(PAC), how far the peak moves (PLC) and how often it leaves the box.  The reference has no such pass.

Per pass one eval forward, one forward + backward for the gradients (`ppf_col2im_patch_f32` ends the backward, `ppf_grad_box_mass`
sums the gradient) and per attack step one more forward + backward and one `ppf_pgd_step_box` (interpret.spatial_alignment); the rows
stay on the device until the split is done.

    python -m protopformer_amd.alignment --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split test]
                                         [--protos_per_image 3] [--half_size 36] [--attack_steps 10] [--eps 8] [--no-attack]
                                         [--max_images N] [--precise]
                                         + the model flags of train.py

writes OUT/alignment.json: the image and row counts, the settings, and overall and per prototype the mean share, the mean area
baseline, their ratio, the mean PAC, the mean PLC and the fraction of peaks that left the box."""


def get_args_parser():
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer spatial alignment: gradient locality and the misalignment attack", "test", "evaluated")
    a = p.add_argument
    a("--protos_per_image", type=int, default=3, help="the strongest local prototypes of the predicted class kept per image")
    a("--half_size", type=int, default=36, help="the box reaches this many pixels to each side of the activation peak")
    a("--attack_steps", type=int, default=10, help="signed-gradient steps of the attack (a forward and a backward each)")
    a("--eps", type=float, default=8.0, help="L-inf budget of the attack in 1/255 pixel units")
    a("--no-attack", dest="attack", action="store_false", default=True, help="gradient locality only")
    a("--precise", action="store_true", default=False, help="run the model in the fp32 verification mode")
    p.set_defaults(seed=0)
    return p


def summarize(result, args):
    """The JSON record: counts, settings, the overall means and the per-prototype table (keys as strings, NaN as null)."""
    from .tooling import json_clean
    return json_clean(dict(images=int(result["images"]), rows=int(result["rows"]),
                settings=dict(protos_per_image=args.protos_per_image, half_size=args.half_size, attack=bool(args.attack), attack_steps=args.attack_steps,
                              eps_255=args.eps, precise=bool(args.precise), split=args.split),
                overall=result["overall"], per_prototype=dict(sorted(result["per_prototype"].items()))))


def main(args, model=None, loader=None):
    """model / loader: a ready model and iterable of (x, ...) CUDA batches (tests, notebooks); by default tooling.tool_setup builds both."""
    from .interpret import spatial_alignment
    from .tooling import tool_setup, write_json
    model, loader, _, _ = tool_setup(args, "alignment", model, loader, with_ids=False)
    if args.precise:
        model.precise = True
    res = spatial_alignment(model, loader, protos_per_image=args.protos_per_image, half_size=args.half_size, attack=args.attack,
                            attack_steps=args.attack_steps, eps=args.eps / 255.0, max_images=args.max_images, pass_images=args.batch_size)
    path = write_json(args, "alignment.json", summarize(res, args))
    print(f"spatial alignment of {res['images']} {args.split} images ({res['rows']} image-prototype pairs): {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
