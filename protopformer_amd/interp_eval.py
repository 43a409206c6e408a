"""Interpretability of a trained checkpoint on the CUB-200-2011 test set: the part-consistency score of the reference's
eval_interpretability.py and the stability score reported next to it (Huang et al., ICCV 2023), in one pass over the data.

    python -m protopformer_amd.interp_eval --data_path .../CUB_200_2011 --resume CKPT --out_dir OUT --batch_size 256
                                           --base_architecture deit_small_patch16_224 --prototype_shape 2000 192 1 1
                                           --reserve_layers 11 --reserve_token_nums 81 --use_global True --use_ppc_loss True
                                           [--no-stability] [--noise_std 0.2] [--noise_seed 0] [--host]

The flags of eval_interpretability.py keep their names, types and defaults.  Prints 'Consistency Score: xx.xx%' in the reference's
format and 'Stability Score: xx.xx%', and writes OUT/interpretability.json (scores, per-prototype lists, noise settings, image
count).  Nothing GPU-related is imported with the module: the parser works anywhere."""
import argparse
import json
import os


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("true", "yes", "t", "y"):
        return True
    if v.lower() in ("false", "no", "f", "n"):
        return False
    raise argparse.ArgumentTypeError("Unsupported value encountered.")


def get_args_parser():
    p = argparse.ArgumentParser("ProtoPFormer interpretability: part-consistency and stability score on CUB-200-2011")
    a = p.add_argument
    a("--gpuid", type=str, default="0")
    a("--data_path", type=str)
    a("--imgclass", type=int, default=[15, ], nargs=1)
    a("--out_dir", type=str)
    a("--batch_size", type=int)
    a("--check_test", type=str2bool, default=False)
    # model
    a("--data_set", default="CUB2011U", type=str, help="CUB2011U (200 classes, 15 parts, read under --data_path), or PartsWorld: the classes, "
      "parts and annotations of the rendered set (data.PartsWorld); --data_path may then name a settings .json")
    a("--base_architecture", type=str, default="vgg16")
    a("--input_size", default=224, type=int, help="images input size")
    a("--prototype_shape", nargs="+", type=int, default=[2000, 64, 1, 1])
    a("--prototype_activation_function", type=str, default="log")
    a("--add_on_layers_type", type=str, default="regular")
    a("--reserve_layers", nargs="+", type=int, default=[])
    a("--reserve_token_nums", nargs="+", type=int, default=[])
    a("--use_global", type=str2bool, default=False)
    a("--use_ppc_loss", type=str2bool, default=False)
    a("--ppc_cov_thresh", type=float, default=1.)
    a("--ppc_mean_thresh", type=float, default=2.)
    a("--global_coe", type=float, default=0.5)
    a("--global_proto_per_class", type=int, default=5)
    a("--resume", type=str)
    # the stability score
    a("--no-stability", dest="no_stability", action="store_true", default=False, help="consistency score only: no noisy second pass")
    a("--noise_std", type=float, default=0.2, help="sigma of the Gaussian noise added to the normalised input")
    a("--noise_seed", type=int, default=0, help="seed of the noise; an image's noise depends on (seed, image id, element) only")
    a("--host", action="store_true", default=False, help="score on the host (numpy referee path) instead of on the device")
    return p


def cub_dirs(data_path):
    """(root that holds CUB_200_2011/, the CUB_200_2011 directory itself): --data_path may name either (the reference's script takes the
    inner directory, data.Cub2011 the outer one)."""
    data_path = os.path.abspath(os.path.expanduser(data_path))
    if os.path.isdir(os.path.join(data_path, "CUB_200_2011")):
        return data_path, os.path.join(data_path, "CUB_200_2011")
    return os.path.dirname(data_path), data_path


def report(scores, n_images, args):
    """The JSON document of the tool."""
    return dict(consistency=scores["consistency"], stability=scores["stability"], effects=scores["effects"], max_parts=scores["max_parts"],
                stable_fraction=scores["stable_fraction"], noise_std=args.noise_std, noise_seed=args.noise_seed, stability_computed=not args.no_stability,
                path="host" if args.host else "device", images=int(n_images))


def main(args, model=None):
    os.environ.setdefault("CUDA_VISIBLE_DEVICES", args.gpuid[0])
    import torch
    from PIL import Image

    from . import data as D
    from . import engine as E
    from .interpret import CubParts, interpretability_scores
    from .tooling import load_for_eval, model_from_args
    device = torch.device("cuda")
    nb_classes, n_parts, half_size, part_thresh = 200, 15, 36, 0.8
    rendered = args.data_set == "PartsWorld"                  # classes, parts and sizes are the spec's; nothing is read from disk
    view = D.build_view_transform(args, square=True)          # the reference's Resize((size, size)); GpuFinisher normalises
    if rendered:
        ds = D.PartsWorld(D.partsworld_spec_from_args(args), train=False, transform=view, return_id=True)
        nb_classes, n_parts = ds.spec.classes, ds.spec.parts
    if model is None:
        model = model_from_args(args, nb_classes, img_size=args.input_size, pretrained=not rendered)
    load_for_eval(model, args, device)
    model.eval()
    if not rendered:
        root, meta = cub_dirs(args.data_path)
        ds = D.Cub2011(root, train=False, transform=view, return_id=True)
    if D.device_data_enabled(args):                     # the same square bilinear view produced on the device from resident originals
        loader = D.DeviceAugLoader(D.DeviceDataset(ds, device, num_workers=10), args.batch_size, D.GpuFinisher(re_prob=0.0), False, args, square=True)
    else:
        loader = D.DeviceLoader(ds, args.batch_size, device, D.GpuFinisher(re_prob=0.0), shuffle=False, num_workers=10)
    if args.check_test:
        acc = E.evaluate_epoch(loader, model, device)
        print(f"test accuracy: {acc['acc1']:.2f}%", flush=True)
    parts = ds.annotation() if rendered else CubParts(meta)
    sizes = dict(parts.image_sizes) if rendered else {}
    for img_id, fp, _ in ([] if rendered else ds.data):
        with Image.open(os.path.join(ds.root, ds.base_folder, fp)) as im:
            sizes[int(img_id)] = im.size                       # (width, height) of the original file
    scores = interpretability_scores(model, loader, parts, sizes, num_classes=nb_classes, part_thresh=part_thresh, half_size=half_size,
                                     n_parts=n_parts, noise_std=args.noise_std, seed=args.noise_seed, stability=not args.no_stability,
                                     device=not args.host)
    print("Consistency Score: {:.2%} ".format(scores["consistency"]), flush=True)
    if scores["stability"] is not None:
        print("Stability Score: {:.2%} ".format(scores["stability"]), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, "interpretability.json")
    with open(path, "w") as f:
        json.dump(report(scores, len(ds), args), f, indent=1)
    print(f"interpretability of {len(ds)} test images: {path}", flush=True)
    return scores


if __name__ == "__main__":
    main(get_args_parser().parse_args())
