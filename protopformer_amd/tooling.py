"""What the command-line tools (train, bank, explain, faithfulness, alignment, because, interp_eval) set up alike: the PPNet of the training
flags, a checkpoint loaded for evaluation, the eval-view loader over a split, the --split / --max_images flags and the "stop after N
images" iteration.  Plain functions over `args`; nothing GPU-related is imported with the module."""


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


def eval_loader(args, device, *, with_ids=True):
    """(data set, class count, loader) of --split in the eval geometry (Resize(256/224 * size) + CenterCrop, no augmentation, in file
    order); with_ids: the batches carry the image ids where the data set has them (Cub2011.return_id)."""
    from . import data as D
    ds, num_classes = D.build_dataset(args.split == "train", args, transform=D.build_view_transform(args))
    if with_ids and hasattr(ds, "return_id"):
        ds.return_id = True
    if D.device_data_enabled(args):                     # the same geometry produced on the device from resident originals
        return ds, num_classes, D.DeviceAugLoader(D.DeviceDataset(ds, device, num_workers=args.num_workers), args.batch_size,
                                                  D.GpuFinisher(re_prob=0.0), False, args)
    return ds, num_classes, D.DeviceLoader(ds, args.batch_size, device, D.GpuFinisher(re_prob=0.0), shuffle=False, num_workers=args.num_workers)


def add_split_flags(parser, split, what):
    """--split (default `split`; the help says the split is `what`) and --max_images."""
    parser.add_argument("--split", type=str, default=split, choices=["train", "test"], help=f"which split is {what} (no augmentation either way)")
    parser.add_argument("--max_images", type=int, default=0, metavar="N", help="stop after N images (0: the whole split)")


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
