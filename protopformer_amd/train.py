"""The training driver (main.py of the reference): argument parser, distributed initialisation, data, model, optimizer, schedule, --resume,
--eval and the epoch loop (train, step the schedule, checkpoint every save_ep_freq epochs, validate, keep epoch-best.pth).

    python -m protopformer_amd.train --base_architecture deit_small_patch16_224 --data_set CUB2011U --data_path datasets ...
    torchrun --nproc_per_node=N -m protopformer_amd.train ...

Every flag of main.py:get_args_parser is accepted with its name, type and default (tests/golden/train_args.json pins that), so the
argument lists of scripts/train_*.sh carry over; two flags are ours: --no-pretrained (seeded random init instead of the ImageNet weights
under $PPF_PRETRAINED_DIR) and --step (recorded or eager train step).  tensorboard's scalars go to <output_dir>/train-logs/scalars.jsonl,
one JSON object per epoch, under the same names."""
import argparse
import copy
import datetime
import json
import logging
import os
import random
import time

import numpy as np
import torch
import torch.distributed as dist

from . import data as D
from . import engine as E
from .mixup import create_criterion, create_mixup
from .tooling import model_from_args

LOGGER_NAME = "protopformer_amd.train"
SCALARS = ("epoch/train_loss", "epoch/val_acc1", "epoch/val_loss", "epoch/val_acc5", "epoch/global_acc1", "epoch/local_acc1")
PPC_START_EPOCH = 20                      # engine_proto.py:61-64: the PPC terms join the loss from this epoch on


def str2bool(v):
    if v.lower() in ("true", "yes", "t", "y"):
        return True
    if v.lower() in ("false", "no", "f", "n"):
        return False
    raise argparse.ArgumentTypeError(f"expected one of true/yes/t/y/false/no/f/n, got {v!r}")


def get_args_parser():
    p = argparse.ArgumentParser("ProtoPFormer training and evaluation on the HIP kernels", add_help=False)
    a = p.add_argument
    # the recipe switches.  type=bool as in the reference: any non-empty value, "False" included, switches the flag ON
    a("--batch_size", type=int, default=256)
    a("--distillw", type=float, default=0.5, help="unused (kept for the reference's command lines)")
    a("--enable_smoothing", type=bool, default=False, help="label smoothing 0.1")
    a("--enable_mixup", type=bool, default=False, help="Mixup / CutMix with the --mixup* / --cutmix* settings")
    a("--w_dis_token", type=bool, default=False, help="unused")
    # the ProtoPFormer head
    a("--base_architecture", type=str, default="deit_tiny_patch16_224")
    a("--img_size", type=int, default=224)
    a("--prototype_shape", type=int, nargs="+", default=[2000, 192, 1, 1])
    a("--prototype_activation_function", type=str, default="log")
    a("--add_on_layers_type", type=str, default="regular")
    a("--baseline_path", type=str, default=None, help="unused")
    a("--reserve_layers", type=int, nargs="+", default=[])
    a("--reserve_token_nums", type=int, nargs="+", default=[])
    a("--use_global", type=str2bool, default=False)
    a("--use_ppc_loss", type=str2bool, default=False)
    a("--ppc_cov_thresh", type=float, default=1.)
    a("--ppc_mean_thresh", type=float, default=2.)
    a("--global_coe", type=float, default=0.5)
    a("--global_proto_per_class", type=int, default=5)
    a("--ppc_cov_coe", type=float, default=0.1)
    a("--ppc_mean_coe", type=float, default=0.5)
    a("--data_path", type=str, default="./datasets/cub200_cropped/")
    # the three learning rates of the joint optimizer
    a("--features_lr", type=float, default=1e-4)
    a("--add_on_layers_lr", type=float, default=3e-3)
    a("--prototype_vectors_lr", type=float, default=3e-3)
    a("--joint_lr_step_size", type=int, default=5, help="unused")
    a("--coefs_crs_ent", type=float, default=1, help="unused")
    a("--coefs_clst", type=float, default=0.8, help="unused")
    a("--coefs_sep", type=float, default=-0.08, help="unused")
    a("--coefs_l1", type=float, default=1e-4, help="unused")
    a("--epochs", type=int, default=40)
    # model
    a("--model", type=str, default="deit_tiny_patch16_224", metavar="MODEL", help="names the log file")
    a("--input_size", type=int, default=224)
    a("--save_ep_freq", type=int, default=400, help="write checkpoint-<epoch>.pth every this many epochs")
    a("--drop", type=float, default=0.0, metavar="PCT", help="unused")
    a("--drop_path", type=float, default=0.1, metavar="PCT", help="unused (construct_PPNet builds the backbone with 0.1)")
    a("--model_ema", action="store_true")
    a("--no-model-ema", action="store_false", dest="model_ema")
    p.set_defaults(model_ema=True)
    a("--model-ema-decay", type=float, default=0.99996)
    a("--model-ema-force-cpu", action="store_true", default=False, help="ignored: the average lives in the flat device buffers")
    # optimizer
    a("--opt", type=str, default="adamw", metavar="OPTIMIZER", help="only adamw (the fused kernel); anything else is ignored")
    a("--opt-eps", type=float, default=1e-8, metavar="EPSILON")
    a("--opt-betas", type=float, nargs="+", default=None, metavar="BETA")
    a("--clip_grad", type=float, default=None, metavar="NORM")
    a("--momentum", type=float, default=0.9, metavar="M", help="unused (SGD)")
    a("--weight_decay", type=float, default=0.05)
    # schedule
    a("--sched", type=str, default="cosine", metavar="SCHEDULER", help="only cosine")
    a("--lr", type=float, default=5e-4, metavar="LR", help="unused (the three *_lr flags set the rates)")
    a("--lr-noise", type=float, nargs="+", default=None, metavar="pct, pct", help="ignored")
    a("--lr-noise-pct", type=float, default=0.67, metavar="PERCENT", help="ignored")
    a("--lr-noise-std", type=float, default=1.0, metavar="STDDEV", help="ignored")
    a("--warmup-lr", type=float, default=1e-6, metavar="LR")
    a("--min-lr", type=float, default=1e-5, metavar="LR")
    a("--decay-epochs", type=float, default=30, metavar="N", help="unused by the cosine schedule")
    a("--warmup-epochs", type=int, default=5, metavar="N")
    a("--cooldown-epochs", type=int, default=10, metavar="N")
    a("--patience-epochs", type=int, default=10, metavar="N", help="unused by the cosine schedule")
    a("--decay-rate", "--dr", type=float, default=0.1, metavar="RATE", help="unused by the cosine schedule")
    # augmentation
    a("--color-jitter", type=float, default=0.4, metavar="PCT")
    a("--aa", type=str, default="rand-m9-mstd0.5-inc1", metavar="NAME")
    a("--smoothing", type=float, default=0.0)
    a("--train-interpolation", type=str, default="bicubic")
    a("--reprob", type=float, default=0.25, metavar="PCT")
    a("--remode", type=str, default="pixel")
    a("--recount", type=int, default=1)
    a("--resplit", action="store_true", default=False)
    a("--mixup", type=float, default=0.0)
    a("--cutmix", type=float, default=1.0)
    a("--cutmix-minmax", type=float, nargs="+", default=None)
    a("--mixup-prob", type=float, default=1.0)
    a("--mixup-switch-prob", type=float, default=0.5)
    a("--mixup-mode", type=str, default="batch")
    a("--finetune", default="", help="names the run in the reference's scripts; nothing is loaded from it")
    # data, run
    a("--data_set", type=str, default="CIFAR100", choices=["CUB2011U", "Car", "Dogs", "PartsWorld"])
    a("--inat-category", type=str, default="name",
      choices=["kingdom", "phylum", "class", "order", "supercategory", "family", "genus", "name"], help="unused")
    a("--output_dir", default="output_kd/test/", help="where logs and checkpoints go; empty: nothing is saved")
    a("--device", default="cuda")
    a("--seed", type=int, default=1028)
    a("--resume", default="", help="checkpoint to continue from (with --eval: to evaluate)")
    a("--start_epoch", type=int, default=0, metavar="N")
    a("--eval", action="store_true", help="evaluate only")
    a("--dist-eval", action="store_true", default=False, help="shard the validation set over the ranks")
    a("--num_workers", type=int, default=10)
    a("--pin-mem", action="store_true")
    a("--no-pin-mem", action="store_false", dest="pin_mem")
    p.set_defaults(pin_mem=True)
    a("--world_size", type=int, default=1)
    a("--dist_url", default="env://")
    # ours
    a("--no-pretrained", action="store_true", default=False,
      help="seeded random init of the backbone instead of <base_architecture>.pth under $PPF_PRETRAINED_DIR")
    a("--step", type=str, default=None, choices=["replayed", "eager"],
      help="train step: a recorded command list replayed per batch, or the eager step (default: replayed unless Mixup is on)")
    return p


def set_seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def env_rank():
    return int(os.environ.get("RANK", 0)) if "WORLD_SIZE" in os.environ else 0


def init_distributed_mode(args):
    """tools/utils.py:247-269 for a torchrun / torch.distributed.launch --use_env start: RANK, WORLD_SIZE and LOCAL_RANK."""
    if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        args.distributed, args.rank, args.gpu = False, 0, 0
        return
    args.rank, args.world_size, args.gpu = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", 0))
    args.distributed = True
    torch.cuda.set_device(args.gpu)
    args.dist_backend = "nccl"
    if not dist.is_initialized():
        dist.init_process_group(backend=args.dist_backend, init_method=args.dist_url, world_size=args.world_size, rank=args.rank)
    dist.barrier()


def get_logger(args, master=True):
    """Console + <output_dir>/{train,eval}-logs/<model>_<data_set>.log (rank 0 only); creates the output directories."""
    logger = logging.getLogger(LOGGER_NAME)
    for h in list(logger.handlers):               # main() may run more than once in a process
        logger.removeHandler(h)
        h.close()
    logger.setLevel(logging.INFO if master else logging.WARNING)
    logger.propagate = False
    fmt = logging.Formatter("%(asctime)s - %(funcName)s - %(levelname)s - %(message)s")
    console = logging.StreamHandler()
    console.setFormatter(fmt)
    logger.addHandler(console)
    if master and args.output_dir:
        log_dir = os.path.join(args.output_dir, "eval-logs" if args.eval else "train-logs")
        os.makedirs(log_dir, exist_ok=True)
        os.makedirs(os.path.join(args.output_dir, "checkpoints"), exist_ok=True)
        fh = logging.FileHandler(os.path.join(log_dir, f"{args.model}_{args.data_set}.log"), "w")
        fh.setFormatter(fmt)
        logger.addHandler(fh)
    return logger


def log_ignored(args, logger):
    """Flags of the reference that have no meaning on this path: said once, then ignored."""
    if args.opt.lower() != "adamw":
        logger.warning(f"--opt {args.opt} ignored: the optimizer is the fused AdamW kernel")
    if args.model_ema_force_cpu:
        logger.warning("--model-ema-force-cpu ignored: the average is a flat device buffer updated by the optimizer kernel")
    if not args.pin_mem:
        logger.warning("--no-pin-mem ignored: the loader always stages uint8 frames through pinned memory")
    if args.lr_noise is not None:
        logger.warning("--lr-noise / --lr-noise-pct / --lr-noise-std ignored: the schedule runs without noise")


def resume(args, model, optimizer, lr_scheduler, logger):
    """main.py:393-407.  Training: model, optimizer, schedule, EMA, and args.start_epoch = checkpoint epoch + 1.  --eval: the model only."""
    if args.resume.startswith("https"):
        raise ValueError("--resume from a URL: there is no download on this path, pass a local checkpoint file")
    start = E.load_checkpoint(args.resume, model, optimizer, lr_scheduler, strict=True, eval_only=args.eval)
    if not args.eval and start > 0:
        args.start_epoch = start
    logger.info(f"resumed from {args.resume}" + ("" if args.eval else f", start epoch {args.start_epoch}"))
    return args.start_epoch


def run_epochs(args, start_epoch, train_epoch, eval_epoch, step_scheduler, save, logger, n_parameters=0, n_val=0, master=True):
    """The epoch loop of main.py:418-471 over callables, so that its bookkeeping can be tested without a GPU:
    train_epoch(epoch) -> {'loss', ...}, step_scheduler(epoch), save(file name, epoch), eval_epoch(epoch) -> {'acc1', 'acc5', 'loss', ...}.
    Returns the per-epoch log_stats."""
    records, max_accuracy = [], 0.0
    for epoch in range(start_epoch, args.epochs):
        train_stats = train_epoch(epoch)
        logger.info(f"Averaged stats: {train_stats}")
        step_scheduler(epoch)
        if args.output_dir and (epoch + 1) % args.save_ep_freq == 0:
            save(f"checkpoint-{epoch}.pth", epoch)
        test_stats = eval_epoch(epoch)
        logger.info(test_stats)
        logger.info(f"Accuracy of the network on the {n_val} test images: {test_stats['acc1']:.1f}%")
        if max_accuracy < test_stats["acc1"]:                      # strictly better than the best so far (which starts at 0.0)
            if args.output_dir:
                save("epoch-best.pth", epoch)
        max_accuracy = max(max_accuracy, test_stats["acc1"])
        logger.info(f"Max accuracy: {max_accuracy:.2f}%")
        if master and args.output_dir:
            scalars = {"epoch": epoch, "epoch/train_loss": train_stats["loss"], "epoch/val_acc1": test_stats["acc1"],
                       "epoch/val_loss": test_stats["loss"], "epoch/val_acc5": test_stats.get("acc5"),
                       "epoch/global_acc1": test_stats.get("global_acc1"), "epoch/local_acc1": test_stats.get("local_acc1")}
            os.makedirs(os.path.join(args.output_dir, "train-logs"), exist_ok=True)
            with open(os.path.join(args.output_dir, "train-logs", "scalars.jsonl"), "a") as f:
                f.write(json.dumps(scalars) + "\n")
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, **{f"test_{k}": v for k, v in test_stats.items()},
                     "epoch": epoch, "n_parameters": n_parameters}
        logger.info(log_stats)
        records.append(log_stats)
    return records


class StepPhases:
    """One recorded step per phase of the loss: a ReplayedTrainStep bakes in whether the PPC terms are part of the loss (epoch >= 20 with
    --use_ppc_loss, GraphedTrainStep.check_matches), so the step of the first phase is never replayed in the second -- a new one is
    recorded when the epoch reaches 20."""

    def __init__(self, args, model, criterion, optimizer, grad_sync):
        self.args, self.model, self.criterion, self.optimizer, self.grad_sync = args, model, criterion, optimizer, grad_sync
        self.steps = {}

    def get(self, epoch):
        a = self.args
        phase = bool(a.use_ppc_loss) and epoch >= PPC_START_EPOCH
        if phase not in self.steps:
            self.steps[phase] = E.ReplayedTrainStep(self.model, self.criterion, self.optimizer, epoch=epoch, ppc_cov_coe=a.ppc_cov_coe,
                                                    ppc_mean_coe=a.ppc_mean_coe, use_ppc_loss=bool(a.use_ppc_loss),
                                                    grad_sync=self.grad_sync, max_norm=a.clip_grad)
        return self.steps[phase]


def main(args, model=None):
    """main.py:251-475.  model: an already built PPNet used instead of construct_PPNet (tests).  Returns the per-epoch log_stats, or the
    validation stats under --eval."""
    set_seed(args.seed + env_rank())
    if args.enable_smoothing:
        args.smoothing = 0.1
    init_distributed_mode(args)
    master = args.rank == 0
    logger = get_logger(args, master)
    logger.info(f"Start running with args: \n{args}")
    logger.info(f"Distributed: {args.distributed}")
    log_ignored(args, logger)
    device = torch.device(args.device)

    loader_train, loader_val, args.nb_classes = D.build_loaders(args, device)
    if args.distributed and args.dist_eval:
        ds_val = loader_val.dataset
        if len(ds_val) % args.world_size != 0:
            logger.warning("Warning: Enabling distributed evaluation with an eval dataset not divisible by process number. This will slightly "
                           "alter validation results as extra duplicate entries are added to achieve equal num of samples per-process.")
        sampler_val = torch.utils.data.DistributedSampler(ds_val, num_replicas=args.world_size, rank=args.rank, shuffle=False)
        if isinstance(loader_val, D.DeviceAugLoader):                # the resident path (PPF_DEVICE_DATA): every rank holds the whole set
            loader_val = D.DeviceAugLoader(loader_val.dd, int(1.5 * args.batch_size), D.GpuFinisher(re_prob=0.0), False, args, sampler=sampler_val,
                                           seed=args.seed)
        else:
            loader_val = D.DeviceLoader(ds_val, int(1.5 * args.batch_size), device, D.GpuFinisher(re_prob=0.0), sampler=sampler_val,
                                        num_workers=args.num_workers)
    n_train, n_val = len(loader_train.dataset), len(loader_val.dataset)
    logger.info(f"Dataset num_classes: {args.nb_classes}")
    logger.info(f"train {n_train} test: {n_val}")

    mixup_fn = create_mixup(args)
    criterion = create_criterion(args)
    logger.info(f"Label smoothing rate: {args.smoothing}; " + ("Mixup is not enabled" if mixup_fn is None else
                                                                f"mixup_fn smoothing rate: {mixup_fn.label_smoothing}"))

    if model is None:
        model = model_from_args(args, args.nb_classes)
    model.to(device)
    n_parameters = sum(p.numel() for p in model.parameters() if p.requires_grad)
    logger.info(f"number of params: {n_parameters}")

    lrs = {"features": args.features_lr, "add_on_layers": args.add_on_layers_lr, "prototype_vectors": args.prototype_vectors_lr}
    betas = tuple(args.opt_betas) if args.opt_betas is not None else (0.9, 0.999)
    optimizer = E.FlatAdamW(model, joint_optimizer_lrs=lrs, weight_decay=args.weight_decay, betas=betas, eps=args.opt_eps,
                            ema_decay=args.model_ema_decay if args.model_ema else None)
    sched_args = args
    if args.lr_noise is not None:                                  # logged as ignored above
        sched_args = copy.copy(args)
        sched_args.lr_noise = None
    lr_scheduler, _ = E.create_scheduler(sched_args, optimizer)

    if args.resume:
        resume(args, model, optimizer, lr_scheduler, logger)
    # after --resume, so that every rank continues from rank 0's restored state (parameters, moments, EMA)
    grad_sync = E.make_grad_sync(model, optimizer) if args.distributed and args.world_size > 1 else None

    dist_eval = bool(args.distributed and args.dist_eval)
    if args.eval:
        test_stats = E.evaluate_epoch(loader_val, model, device, distributed=dist_eval)
        logger.info(test_stats)
        logger.info(f"Accuracy of the network on the {n_val} test images: {test_stats['acc1']:.1f}%")
        return test_stats

    step_kind = args.step or ("replayed" if mixup_fn is None else "eager")
    phases = StepPhases(args, model, criterion, optimizer, grad_sync) if step_kind == "replayed" else None
    logger.info(f"Start training for {args.epochs} epochs ({step_kind} step)")

    def train_epoch(epoch):
        if hasattr(loader_train, "set_epoch"):
            loader_train.set_epoch(epoch)                            # the resident loader: its draws and its sampler follow the epoch
        elif loader_train.sampler is not None:
            loader_train.sampler.set_epoch(epoch)
        return E.train_one_epoch(model, criterion, loader_train, optimizer, device, epoch, args=args, grad_sync=grad_sync, logger=logger.info,
                                 max_norm=args.clip_grad, step_fn=phases.get(epoch) if phases is not None else None, mixup_fn=mixup_fn)

    def save(name, epoch):
        E.save_checkpoint(os.path.join(args.output_dir, "checkpoints", name), model, optimizer, lr_scheduler, epoch, args=args)

    start_time = time.time()
    records = run_epochs(args, args.start_epoch, train_epoch, lambda epoch: E.evaluate_epoch(loader_val, model, device, distributed=dist_eval),
                         lr_scheduler.step, save, logger, n_parameters=n_parameters, n_val=n_val, master=master)
    logger.info(f"Training time {datetime.timedelta(seconds=int(time.time() - start_time))}")
    return records


if __name__ == "__main__":
    parser = argparse.ArgumentParser("ProtoPFormer training and evaluation script", parents=[get_args_parser()])
    cli_args = parser.parse_args()
    if cli_args.output_dir:
        os.makedirs(cli_args.output_dir, exist_ok=True)
    try:
        main(cli_args)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
