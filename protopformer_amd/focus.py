"""Does the model look at the object?  Foreground focus of a trained checkpoint against annotated object boxes over a split: are the
reserved tokens on the object, do the prototype maps peak and carry their positive mass there (the pointing game and its energy-based
form, Wang et al., Score-CAM, 2020), and how much of the class evidence comes from cells on the object -- each next to the object's
share of the image area, what a spatially blind model would score.  The reference has no such pass.

Per batch one eval forward, one `ppf_act_focus` over the selected prototypes' maps, the order-statistics and box launches of
interpret.high_activation_boxes, `ppf_focus_box_terms`, `ppf_reserve_focus` and `ppf_evidence_focus` (interpret.foreground_focus); the
rows stay on the device until the split is done.  The images are seen in the square view (Resize((size, size))), as interp_eval sees
them, so the boxes map linearly (interpret.scaled_boxes); PPF_DEVICE_DATA is honoured as there.

    python -m protopformer_amd.focus --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split test]
                                     [--protos own|top] [--protos_per_image 3] [--percentile 95] [--max_images N]
                                     [--boxes FILE.json] [--per-image]
                                     + the model and data flags of train.py

writes OUT/focus.json: counts, settings, and overall, per class and (with --protos own) per prototype the measures of
interpret.focus_summary; with --per-image also OUT/focus.npz, the rows.  For CUB the boxes are bounding_boxes.txt's
(interpret.CubParts.id_to_bbox), for PartsWorld the rendered objects' own (data.PartsWorld.annotation()); for any other set --boxes names a JSON {image id: [x0, y0, x1, y1]} in pixels of the original files,
the image id being the image's index in the split's file order.  Nothing GPU-related is imported with the module: the parser works
anywhere."""
import json
import os


def get_args_parser():
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer foreground focus: reserved tokens, prototype maps and evidence against object boxes", "test", "evaluated")
    a = p.add_argument
    a("--protos", type=str, default="own", choices=["own", "top"],
      help="own: the prototypes of the image's label class; top: the strongest prototypes of the predicted class")
    a("--protos_per_image", type=int, default=3, help="with --protos top: the strongest local prototypes of the predicted class kept per image")
    a("--percentile", type=float, default=95, help="the high-activation box holds the map's entries at or above this percentile")
    a("--boxes", type=str, default="", metavar="FILE.json", help="{image id: [x0, y0, x1, y1]} in pixels of the original files (not needed for CUB)")
    a("--per-image", dest="per_image", action="store_true", default=False, help="also write the rows to focus.npz")
    p.set_defaults(seed=0)
    return p


def read_boxes(path):
    """{image id: (x0, y0, x1, y1)} of a --boxes file; refuses anything but four integers per image."""
    with open(path) as f:
        doc = json.load(f)
    out = {}
    for k, v in doc.items():
        if not isinstance(v, (list, tuple)) or len(v) != 4 or any(int(c) != c for c in v):
            raise ValueError(f"{path}: the box of image {k!r} must be four integers [x0, y0, x1, y1], got {v!r}")
        out[int(k)] = tuple(int(c) for c in v)
    return out


def image_files(ds):
    """{image id: path of the original file} of a data set of data.build_dataset: CUB's own image ids, else the index in file order
    (what tooling.batches_with_ids hands out for a loader without ids)."""
    if hasattr(ds, "data"):
        return {int(i): os.path.join(ds.root, ds.base_folder, fp) for i, fp, _ in ds.data}
    if hasattr(ds, "_samples"):
        return {i: path for i, (path, _) in enumerate(ds._samples)}
    return {i: os.path.join(ds.images_folder, name) for i, (name, _) in enumerate(ds._flat_breed_images)}


def cub_boxes(data_path):
    """bounding_boxes.txt of the CUB tree under --data_path (which may name the directory that holds CUB_200_2011/ or that directory)."""
    from .interp_eval import cub_dirs
    from .interpret import CubParts
    return dict(CubParts(cub_dirs(data_path)[1]).id_to_bbox)


def summarize(result, args):
    """The JSON record: counts, settings and the measures (keys as strings, NaN as null)."""
    from .tooling import json_clean
    settings = dict(result.get("settings", {}), split=args.split, data_set=args.data_set,
                    boxes=args.boxes or ("annotation" if args.data_set == "PartsWorld" else "bounding_boxes.txt"))
    return json_clean(dict(images=int(result["images"]), rows=int(result["rows"]), settings=settings, overall=result["overall"],
                           per_class=dict(sorted(result["per_class"].items())),
                           per_prototype=None if result.get("per_prototype") is None else dict(sorted(result["per_prototype"].items()))))


def main(args, model=None):
    import numpy as np
    from PIL import Image

    from .interpret import foreground_focus
    from .tooling import tool_setup, write_json
    model, loader, ds, _ = tool_setup(args, "focus", model, square=True)       # the square view, resident on the device where PPF_DEVICE_DATA says so
    rendered = args.data_set == "PartsWorld"                    # no files: boxes and sizes are the data set's own annotation
    if args.boxes:
        boxes = read_boxes(args.boxes)
    elif args.data_set == "CUB2011U":
        boxes = cub_boxes(args.data_path)
    elif rendered:
        boxes = dict(ds.annotation().id_to_bbox)
    else:
        raise ValueError(f"focus: --boxes FILE.json is needed for data_set {args.data_set!r} (only CUB's annotation is read here)")
    sizes = dict(ds.annotation().image_sizes) if rendered else {}
    for i, path in ({} if rendered else image_files(ds)).items():
        with Image.open(path) as im:
            sizes[i] = im.size                                  # (width, height) of the original file
    model.eval()
    res = foreground_focus(model, loader, boxes, sizes, protos=args.protos, protos_per_image=args.protos_per_image, percentile=args.percentile,
                           max_images=args.max_images, per_image=args.per_image)
    path = write_json(args, "focus.json", summarize(res, args))
    if args.per_image:
        np.savez(os.path.join(args.output_dir, "focus.npz"), **{k: v for k, v in res["per_image"].items() if v is not None})
    print(f"foreground focus of {res['images']} {args.split} images ({res['rows']} image-prototype pairs): {path}", flush=True)
    return path


if __name__ == "__main__":
    main(get_args_parser().parse_args())
