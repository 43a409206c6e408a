"""Explanations against the truth.  On PartsWorld the scene table is the render's input, so a part, the distractors or the background can
be taken out of an image exactly -- same geometry, same noise, no grey square -- and what each is worth to the model measured, not
estimated.  This tool measures it over a split and holds every explanation to it: does the map's mass on a part follow what removing
the part costs (single deletion), does the map find the most important part, where does its positive mass lie next to the area a blind
map would cover, and how fast does the class score fall when the parts are hidden in the map's order, between the best and the worst
order there is.  The protocol of FunnyBirds (Hesse et al., ICCV 2023) at this code base's size.  The reference has no such pass.

Per pass of --pass_images images: one eval forward, `ppf_synth_scene` + `ppf_synth_edit` + `ppf_synth_render` + the square view + the
model's forward for the standard edit list and for the cumulative deletions, one `ppf_part_mass` per order
(interpret.part_agreement); the rows stay on the device until the split is done.  PPF_DEVICE_DATA is honoured as in focus.

    python -m protopformer_amd.partcheck --resume CKPT --data_set PartsWorld --output_dir OUT [--split test]
                                         [--orders evidence attention random rise ig] [--value prob|logit] [--against_label]
                                         [--max_images N] [--per-image] [--pass_images 16]
                                         [--rise_masks 512 --rise_cells 7 --rise_p 0.5] [--ig_steps 32 --ig_rule midpoint]
                                         + the model and data flags of train.py

writes OUT/partcheck.json: counts, settings, the spec, `model` (what the parts, the distractors and the background are worth to the
model, once) and `per_order` (interpret.part_agreement_from_rows); with --per-image also OUT/partcheck.npz, the rows.  The default
orders are evidence, attention and random; rise and ig cost hundreds of forwards per image and are opt-in.  Any other --data_set is
refused by name: there is nothing to intervene on.  Nothing GPU-related is imported with the module: the parser works anywhere."""
import os

ORDERS = ("evidence", "attention", "random", "rise", "ig")


def get_args_parser():
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer part interventions on PartsWorld: explanations against the truth", "test", "evaluated")
    a = p.add_argument
    a("--orders", type=str, nargs="+", default=["evidence", "attention", "random"], choices=list(ORDERS), help="the explanations held to the interventions")
    a("--value", type=str, default="prob", choices=["prob", "logit"], help="what an intervention is measured in: the class probability or the class logit")
    a("--against_label", action="store_true", default=False, help="explain the image's label instead of the predicted class")
    a("--per-image", dest="per_image", action="store_true", default=False, help="also write the rows to partcheck.npz")
    a("--pass_images", type=int, default=16, help="images per pass; the result does not depend on --batch_size")
    a("--rise_masks", type=int, default=512)
    a("--rise_cells", type=int, default=7)
    a("--rise_p", type=float, default=0.5)
    a("--ig_steps", type=int, default=32)
    a("--ig_rule", type=str, default="midpoint")
    p.set_defaults(seed=0, data_set="PartsWorld")
    return p


def check_args(args):
    """Refuses by name what the tool cannot run on."""
    if args.data_set != "PartsWorld":
        raise ValueError(f"partcheck: --data_set {args.data_set!r} has nothing to intervene on: only PartsWorld renders its images from a scene table")
    if args.pass_images < 1:
        raise ValueError(f"partcheck: --pass_images {args.pass_images} must be >= 1")
    return args


def summarize(result, args):
    """The JSON record: counts, settings, the spec and the measures (keys as strings, NaN as null)."""
    from .data import partsworld_spec_from_args
    from .tooling import json_clean
    settings = dict(result.get("settings", {}), split=args.split, data_set=args.data_set)
    return json_clean(dict(images=int(result["images"]), parts=int(result["parts"]), settings=settings, spec=partsworld_spec_from_args(args).to_dict(),
                           model=result["model"], per_order=result["per_order"]))


def main(args, model=None):
    import numpy as np

    from .interpret import part_agreement
    from .tooling import tool_setup, write_json
    check_args(args)
    model, loader, ds, _ = tool_setup(args, "partcheck", model, square=True)   # the square view: the whole frame, so every part is in it
    model.eval()
    res = part_agreement(model, loader, ds.spec, orders=tuple(args.orders), value=args.value, against_label=args.against_label,
                         max_images=args.max_images, per_image=args.per_image, pass_images=args.pass_images,
                         rise=dict(masks=args.rise_masks, cells=args.rise_cells, p=args.rise_p), ig=dict(steps=args.ig_steps, rule=args.ig_rule),
                         seed=args.seed)
    path = write_json(args, "partcheck.json", summarize(res, args))
    if args.per_image:
        rows = res["per_image"]
        flat = {k: v for k, v in rows.items() if k != "orders" and v is not None}
        flat.update({f"{o}.{k}": v for o, f in rows["orders"].items() for k, v in f.items()})
        np.savez(os.path.join(args.output_dir, "partcheck.npz"), **flat)
    print(f"part interventions on {res['images']} {args.split} images, orders {' '.join(args.orders)}: {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
