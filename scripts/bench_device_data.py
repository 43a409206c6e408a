"""Cost of the device-resident data path (data.DeviceDataset / DeviceAugLoader, csrc/device_data.hip) on one MI355X --
profiles/device_data_cost.txt.

    python scripts/bench_device_data.py [--images 2048 --batch 256 --workers 16 --reps 10] [--no-step] [--out profiles/device_data_cost.txt]

Over a tree of --images synthetic 500 x 375 JPEGs (made here with Pillow, CUB-200-2011's on-disk format) it measures
  * the yardstick: data.DeviceLoader with --workers CPU workers, train and eval transform, in images/s (the first batches, which pay
    for the start of the workers and arrive together, are reported apart from the steady rate of the rest);
  * the resident loader on the same tree: the one-time decode pass, then train and eval epochs in images/s (events around whole
    epochs, host enqueue time inside: this is what a train loop sees), and the host time per batch for the draws;
  * every kernel at --batch 224 x 224 frames: HIP events around the single call, queued behind a running matrix product
    (bench_common.timed), against a device copy of the bytes it moves;
  * for scale, unless --no-step: the line of `bench.py --gpus 1` in a child process on the same box.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import subprocess
import sys
import tempfile
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402
from PIL import Image   # noqa: E402

from bench_common import row, timed      # noqa: E402

S = 224


def build_tree(root, n):
    """n smooth 500 x 375 JPEGs (a bicubic blow-up of a 20 x 15 random image plus mild noise: tens of KB each, as photographs are)."""
    meta = os.path.join(root, "CUB_200_2011")
    os.makedirs(os.path.join(meta, "images", "001.B"))
    rng = np.random.default_rng(0)
    size = 0
    for i in range(1, n + 1):
        small = Image.fromarray(rng.integers(0, 256, (15, 20, 3), dtype=np.uint8)).resize((500, 375), Image.BICUBIC)
        a = np.clip(np.asarray(small).astype(np.int16) + rng.integers(-12, 13, (375, 500, 3)), 0, 255).astype(np.uint8)
        path = os.path.join(meta, "images", "001.B", f"{i:05d}.jpg")
        Image.fromarray(a).save(path, quality=90)
        size += os.path.getsize(path)
    for name, fmt in (("images.txt", "{i} 001.B/{i:05d}.jpg\n"), ("image_class_labels.txt", "{i} 1\n"), ("train_test_split.txt", "{i} 1\n")):
        with open(os.path.join(meta, name), "w") as f:
            f.write("".join(fmt.format(i=i) for i in range(1, n + 1)))
    return size / n


def epoch_rate(loader, what, skip):
    """One pass over `loader`: seconds until `skip` batches are out (the start of the workers and what they prefetched while the first
    batch was awaited), then images/s of the rest, which the workers produce in steady state (synchronised at both ends)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    head, seen, t1 = 0, 0, None
    for k, batch in enumerate(loader):
        if k == skip:
            torch.cuda.synchronize()
            t1, head = time.perf_counter(), seen
        seen += len(batch[1])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return dict(what=what, images=seen, batches_skipped=skip, skipped_s=round(t1 - t0, 3), rest_s=round(t2 - t1, 3),
                images_per_s_steady=round((seen - head) / (t2 - t1), 1), images_per_s_whole_pass=round(seen / (t2 - t0), 1))


def loaders(root, B, workers, epochs):
    from protopformer_amd import data as D
    dev = torch.device("cuda")
    args = types.SimpleNamespace(input_size=S, aa="rand-m9-mstd0.5-inc1", train_interpolation="bicubic", data_set="CUB2011U", data_path=root, batch_size=B,
                                 num_workers=workers, reprob=0.25, seed=1028)
    rows = []
    # the yardstick walks the tree four times in one pass, at batch 64: every worker produces several batches after the ones it had
    # prefetched when the first batch arrived (at batch 256 the 8 batches of the tree are one batch per worker, all of it start-up)
    four = lambda ds: torch.utils.data.ConcatDataset([ds] * 4)
    cpu_train = D.DeviceLoader(four(D.build_dataset(True, args)[0]), 64, dev, D.GpuFinisher(re_prob=0.25), shuffle=True, num_workers=workers, drop_last=True)
    cpu_eval = D.DeviceLoader(four(D.build_dataset(True, args, transform=D.build_transform(False, args))[0]), 64, dev, D.GpuFinisher(re_prob=0.0),
                              num_workers=workers)
    rows.append(epoch_rate(cpu_train, f"yardstick: DeviceLoader, {workers} CPU workers, train transform, batch 64, the tree four times", 3 * workers))
    rows.append(epoch_rate(cpu_eval, f"yardstick: DeviceLoader, {workers} CPU workers, eval transform, batch 64, the tree four times", 3 * workers))
    dd = D.DeviceDataset(D.build_dataset(True, args)[0], dev, num_workers=workers)
    rows.append(dict(what=f"DeviceDataset: one-time decode pass, {workers} CPU workers, and upload", images=len(dd), seconds=round(dd.decode_seconds, 2),
                     images_per_s=round(len(dd) / dd.decode_seconds, 1), resident_bytes=int(dd.flat.numel())))
    for train, fin in ((True, D.GpuFinisher(re_prob=0.25)), (False, D.GpuFinisher(re_prob=0.0))):
        ld = D.DeviceAugLoader(dd, B, fin, train, args, shuffle=train, drop_last=train, seed=1028)
        for x in ld:                                                               # warm-up epoch: allocations
            pass
        torch.cuda.synchronize()
        ld.host_seconds.clear()
        t0, seen = time.perf_counter(), 0
        for e in range(epochs):
            ld.set_epoch(e + 1)
            for batch in ld:
                seen += len(batch[1])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        hs = np.asarray(ld.host_seconds) * 1e3
        rows.append(dict(what=f"resident loader (DeviceAugLoader), {'train' if train else 'eval'}, batch {B}, {epochs} epochs", images=seen, seconds=round(dt, 3),
                         images_per_s=round(seen / dt, 1), ms_per_batch=round(dt / len(hs) * 1e3, 2), host_draw_ms_per_batch_median=round(float(np.median(hs)), 2),
                         host_draw_ms_per_batch_max=round(float(hs.max()), 2)))
    return rows, dd, args


def kernels(dd, args, B, reps):
    import random
    from protopformer_amd import _lib, data as D
    dev = torch.device("cuda")
    rows = []
    ld = D.DeviceAugLoader(dd, B, D.GpuFinisher(re_prob=0.25), True, args, shuffle=True, seed=1)
    rng = random.Random(3)
    plan = ld._plan(list(range(B)), D.RandomResizedCrop(S, rng=rng), D.RandAugment(args.aa, rng=rng), rng)
    ws = torch.empty(D.resize_workspace_bytes(plan["resize"], S, S, Image.BICUBIC, dd.flat.numel()), dtype=torch.uint8, device=dev)
    frames = D.resize_crop(dd.flat, plan["resize"], S, S, device=True, workspace=ws)
    out = torch.empty_like(frames)
    nbytes = frames.numel()
    src_bytes = int(sum((p[5] - p[3]) * (p[6] - p[4]) * 3 for p in plan["resize"]))
    copy_t = timed(lambda: out.copy_(frames), reps)
    rows.append(row(f"yardstick: device copy of the batch, uint8 [{B}][{S}][{S}][3]", copy_t, 2 * nbytes))

    def add(what, fn, moved):
        t = timed(fn, reps)
        rows.append(row(what, t, moved, time_over_copy_of_the_batch=round(t["us_median"] / copy_t["us_median"], 2)))
    add(f"ppf_resize_crop_u8 (taps + horizontal + vertical pass), RandomResizedCrop boxes of 500 x 375 frames, B={B}; bytes: the boxes read, the batch written",
        lambda: D.resize_crop(dd.flat, plan["resize"], S, S, device=True, workspace=ws), src_bytes + nbytes)
    eplan = D.resize_plan(dd.offsets_host[:B], dd.sizes_host[:B], [(0, 0, 500, 375)] * B, [D.eval_geometry(375, 500, 256, S)[:2]] * B,
                          [D.eval_geometry(375, 500, 256, S)[2:]] * B, [0] * B)
    ews = torch.empty(D.resize_workspace_bytes(eplan, S, S, Image.BICUBIC, dd.flat.numel()), dtype=torch.uint8, device=dev)
    add(f"ppf_resize_crop_u8, eval geometry (Resize 256 + CenterCrop 224, only the window), B={B}; bytes: the frames' share under the window, the batch",
        lambda: D.resize_crop(dd.flat, eplan, S, S, device=True, workspace=ews), int(B * 375 * 500 * 3 * (224 / 256) * (224 / 341)) + nbytes)
    hist = torch.empty((B, 3, 256), dtype=torch.int32, device=dev)
    lut = torch.empty((B, 3, 256), dtype=torch.uint8, device=dev)

    def one(name, param, resample=Image.BILINEAR):
        return torch.from_numpy(D.aug_plan([[(name, param, resample)]] * B, S, S)).to(dev)
    eq, color, sharp = one("Equalize", 0.0), one("ColorIncreasing", 1.81), one("SharpnessIncreasing", 1.81)
    rot2, rot3 = one("Rotate", 27.0, Image.BILINEAR), one("Rotate", 27.0, Image.BICUBIC)
    add("ppf_aug_hist (memset + launch), every sample Equalize", lambda: _lib.call("ppf_aug_hist", frames, eq, 0, B, S, S, hist), nbytes)
    add("ppf_aug_lut_build, every sample Equalize", lambda: _lib.call("ppf_aug_lut_build", hist, eq, 0, B, S, S, lut), B * 768 * 5)
    add("ppf_aug_apply, every sample a table op", lambda: _lib.call("ppf_aug_apply", frames, eq, 0, lut, B, S, S, out), 2 * nbytes)
    add("ppf_aug_apply, every sample ColorIncreasing", lambda: _lib.call("ppf_aug_apply", frames, color, 0, lut, B, S, S, out), 2 * nbytes)
    add("ppf_aug_sharpness, every sample", lambda: _lib.call("ppf_aug_sharpness", frames, sharp, 0, B, S, S, out), 2 * nbytes)
    add("ppf_aug_affine, every sample Rotate 27, BILINEAR (fp64)", lambda: _lib.call("ppf_aug_affine", frames, rot2, 0, B, S, S, 124, 116, 104, out), 2 * nbytes)
    add("ppf_aug_affine, every sample Rotate 27, BICUBIC (fp64)", lambda: _lib.call("ppf_aug_affine", frames, rot3, 0, B, S, S, 124, 116, 104, out), 2 * nbytes)
    add("randaugment_apply of a drawn batch (both slots, ops as rand-m9-mstd0.5-inc1 draws them; host plan upload inside)",
        lambda: D.randaugment_apply(frames, plan["aug"], (124, 116, 104), device=True), 2 * nbytes)
    fin = D.GpuFinisher(re_prob=0.25)
    add("ppf_image_finish_u8 with RandomErasing (unchanged kernel, for scale)", lambda: fin(frames, rects=plan["rects"]), 5 * nbytes)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "device_data_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_data.py measures on the GPU; none found")
    with tempfile.TemporaryDirectory() as root:
        kb = build_tree(root, a.images) / 1e3
        rows = [dict(what=f"tree: {a.images} synthetic 500 x 375 JPEGs, quality 90", mean_kilobytes_per_file=round(kb, 1))]
        lrows, dd, args = loaders(root, a.batch, a.workers, a.epochs)
        rows += lrows + kernels(dd, args, a.batch, a.reps)
    del dd
    torch.cuda.empty_cache()
    if not a.no_step:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "30", "--warmup", "10"], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        rows.append(dict(what="for scale: bench.py --gpus 1 --steps 30 --warmup 10 in a child process on the same box", returncode=r.returncode,
                         line=json.loads(line[-1]) if line else None))
    head = [f"# device-resident data path cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}, Pillow {Image.__version__}",
            f"# produced by: python scripts/bench_device_data.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# loaders: wall clock between device synchronisations; kernels: HIP events around single calls queued behind a running kernel"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
