"""What the command-line tools (train, bank, explain, faithfulness, alignment, because, attribute, focus, interp_eval) set up alike: the PPNet
of the training flags, a checkpoint loaded for evaluation, the eval-view loader over a split, the --split / --max_images flags, the "stop
after N images" iteration, passes of a fixed size, the one host read and the JSON they write; tool_setup is their common prologue.  Plain
functions over `args`; nothing GPU-related is imported with the module."""


def model_from_args(args, num_classes, *, img_size=None, pretrained=None):
    """construct_PPNet from the model flags of train.py.  img_size / pretrained override args.img_size / not args.no_pretrained
    (interp_eval keeps the reference's --input_size and always starts from the pretrained backbone)."""
    from .protopformer import construct_PPNet
    return construct_PPNet(base_architecture=args.base_architecture, pretrained=not args.no_pretrained if pretrained is None else pretrained,
                           img_size=args.img_size if img_size is None else img_size, prototype_shape=args.prototype_shape,
                           num_classes=num_classes, reserve_layers=args.reserve_layers, reserve_token_nums=args.reserve_token_nums,
                           use_global=args.use_global, use_ppc_loss=args.use_ppc_loss, ppc_cov_thresh=args.ppc_cov_thresh,
                           ppc_mean_thresh=args.ppc_mean_thresh, global_coe=args.global_coe, global_proto_per_class=args.global_proto_per_class,
                           prototype_activation_function=args.prototype_activation_function, add_on_layers_type=args.add_on_layers_type)


def load_for_eval(model, args, device):
    """The model on `device`, with the parameters of --resume (strict, no optimizer state) when one is given."""
    from .engine import load_checkpoint
    model.to(device)
    if args.resume:
        load_checkpoint(args.resume, model, strict=True, eval_only=True)
    return model


def eval_loader(args, device, *, with_ids=True, square=False):
    """(data set, class count, loader) of --split in the eval geometry (Resize(256/224 * size) + CenterCrop, or with square the
    Resize((size, size)) view interp_eval and focus see; no augmentation, in file order); with_ids: the batches carry the image ids
    where the data set has them (Cub2011.return_id)."""
    from . import data as D
    ds, num_classes = D.build_dataset(args.split == "train", args, transform=D.build_view_transform(args, square=square))
    if with_ids and hasattr(ds, "return_id"):
        ds.return_id = True
    if D.device_data_enabled(args):                     # the same geometry produced on the device from resident originals
        return ds, num_classes, D.DeviceAugLoader(D.DeviceDataset(ds, device, num_workers=args.num_workers), args.batch_size,
                                                  D.GpuFinisher(re_prob=0.0), False, args, square=square)
    return ds, num_classes, D.DeviceLoader(ds, args.batch_size, device, D.GpuFinisher(re_prob=0.0), shuffle=False, num_workers=args.num_workers)


def tool_setup(args, who, model=None, loader=None, *, with_ids=True, square=False):
    """What every tool's main starts with: the seed, the device, the model of the flags on it with --resume loaded, and the eval loader
    over --split.  model / loader: ready ones (tests, notebooks); a ready loader needs its model, since the class count is the data
    set's.  Returns (model, loader, data set or None for a ready loader, device)."""
    import torch
    from .train import set_seed
    set_seed(args.seed)
    device = torch.device(args.device)
    if loader is not None and model is None:
        raise ValueError(f"{who}.main: a ready loader comes with a ready model (the class count is the data set's)")
    ds = None
    if loader is None:
        ds, nb_classes, loader = eval_loader(args, device, with_ids=with_ids, square=square)
    return load_for_eval(model_from_args(args, nb_classes) if model is None else model, args, device), loader, ds, device


def json_clean(v):
    """v as strict JSON takes it: dictionary keys as strings and NaN as null, at every depth (tuples become lists)."""
    if isinstance(v, dict):
        return {str(k): json_clean(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [json_clean(x) for x in v]
    return None if isinstance(v, float) and v != v else v


def write_json(args, name, doc):
    """json_clean(doc) as --output_dir/name (the directory is made if missing), indent 1.  Returns the path."""
    import json
    import os
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, name)
    with open(path, "w") as f:
        json.dump(json_clean(doc), f, indent=1)
    return path


def add_split_flags(parser, split, what):
    """--split (default `split`; the help says the split is `what`) and --max_images."""
    parser.add_argument("--split", type=str, default=split, choices=["train", "test"], help=f"which split is {what} (no augmentation either way)")
    parser.add_argument("--max_images", type=int, default=0, metavar="N", help="stop after N images (0: the whole split)")


def tool_parser(title, split, what):
    """The parser of a tool that runs over a split: every flag of train.py (the model and data flags among them) and add_split_flags."""
    import argparse
    from .train import get_args_parser as train_parser
    p = argparse.ArgumentParser(title, parents=[train_parser()])
    add_split_flags(p, split, what)
    return p


def take_images(loader, max_images):
    """The loader's batch tuples up to max_images images (0 / None: all of them): the batch that reaches the count is cut to it in
    every element, and nothing is pulled from the loader after it."""
    left = int(max_images or 0)
    for batch in loader:
        n = len(batch[0])
        if max_images and n >= left:
            yield tuple(b[:left] for b in batch)
            return
        yield batch
        left -= n


def batches_with_ids(loader, max_images=0):
    """take_images as (x, y, ids): the int64 image ids the loader supplies as a third element, else the running index in loader order
    (so such a loader must not shuffle)."""
    import torch
    seen = 0
    for x, y, *rest in take_images(loader, max_images):
        n = len(x)
        yield x, y, torch.as_tensor(rest[0]).to(torch.int64) if rest else torch.arange(seen, seen + n, dtype=torch.int64)
        seen += n


def regroup(batches, n):
    """Batch tuples of tensors (of any width) regrouped into consecutive passes of exactly n rows (the last may be shorter), whatever
    the batch sizes they arrive in: what a pass computes then depends on the row sequence alone.  Yields tuples of contiguous tensors;
    dtype and device are the caller's to convert before or after."""
    import torch
    held, have = [], 0
    for batch in batches:
        held.append(tuple(batch)); have += len(batch[0])
        while have >= n:
            full = tuple(torch.cat(f) if len(held) > 1 else f[0] for f in zip(*held))
            yield tuple(f[:n].contiguous() for f in full)
            held, have = ([tuple(f[n:] for f in full)] if have > n else []), have - n
    if have:
        yield tuple(torch.cat(f).contiguous() for f in zip(*held))


def read_once(named):
    """{name: device tensor or None} -> {name: numpy array of the same dtype and shape, or None} in ONE device-to-host transfer.  The
    fields are packed as bytes, larger element sizes first, so that each starts at a multiple of its own; nothing is converted, and the
    arrays are independent copies."""
    import numpy as np
    import torch
    live = sorted(((k, v) for k, v in named.items() if v is not None), key=lambda kv: -kv[1].element_size())
    out = dict.fromkeys(named)
    if live:
        host, o = torch.cat([v.detach().contiguous().reshape(-1).view(torch.uint8) for _, v in live]).cpu().numpy(), 0
        for k, v in live:
            n = v.numel() * v.element_size()
            out[k] = host[o:o + n].view(str(v.dtype).split(".")[1]).reshape(tuple(v.shape)).copy()
            o += n
    return out


def read_rows(kept, who, dims=None):
    """The rows of a data set from the per-batch dicts of device tensors a driver kept: every field concatenated over the batches (along
    dims[field], default 0; a field that is None stays None) and all of them read in one read_once.  No batch: the loader was empty."""
    import torch
    if not kept:
        raise ValueError(f"{who}: the loader gave no image")
    dims = dims or {}
    return read_once({k: (None if kept[0][k] is None else torch.cat([d[k] for d in kept], dim=dims.get(k, 0))) for k in kept[0]})
