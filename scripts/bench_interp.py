"""Cost of the part-consistency post-processing on one MI355X, host path against device path -- profiles/interp_device_cost.txt.

    python scripts/bench_interp.py [--images 5794 --ppc 10 --sweep-images 256 --sweep-protos 2000 --reps 20] [--out profiles/interp_device_cost.txt]

At CUB's test-set shape (5 794 images x 10 own prototypes, 81 of 196 tokens reserved, 14 x 14 -> 224 x 224, 15 parts, random
activations passed through log((d + 1) / (d + 1e-4)), random part locations) it measures
  * interpret.consistency_from_outputs with device=False (the host path: numpy resize_cubic and a peak scan per map) and with
    device=True (expand_to_grid on the GPU, one ppf_act_peak launch with the fused part table, uint8 tables read back), wall clock
    around the whole call ending in a synchronise, inputs on the host in both cases; the two results are compared;
  * PPNet.push_forward of deit_small over the same number of images in batches of 256, for the split between forward and post-processing;
  * the all-prototype sweep (--sweep-images x --sweep-protos maps, one launch), device only: HIP events, --reps repeats after warm-up;
  * ppf_act_upsample alone on 2 560 maps: HIP event pairs, --reps repeats after warm-up, bytes/s against M * (g*g + S*S) * 4 bytes.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import push_forward_ms, timed_back_to_back      # noqa: E402

G, S, KTOK, NPARTS, CLASSES = 14, 224, 81, 15, 200


def activation_like(shape, seed):
    d = np.random.default_rng(seed).random(shape, dtype=np.float32) * 4.0
    return np.log((d + 1) / (d + np.float32(1e-4))).astype(np.float32)


def make_eval(B, ppc):
    rng = np.random.default_rng(1028)
    s = int(round(KTOK ** 0.5))
    attn = rng.random((B, G * G), dtype=np.float32)
    acts = activation_like((B, ppc, s, s), 7)
    targets = np.arange(B) % CLASSES
    ids = np.arange(1, B + 1)
    sizes = {int(i): (int(rng.integers(300, 500)), int(rng.integers(250, 400))) for i in ids}
    locs = {}
    for i in ids:
        w, h = sizes[int(i)]
        locs[int(i)] = [[p, float(rng.random() * (w - 1)), float(rng.random() * (h - 1))] for p in range(1, NPARTS + 1) if rng.random() < 0.75]
    return attn, acts, targets, ids, types.SimpleNamespace(id_to_part_loc=locs), sizes


def consistency(B, ppc):
    from protopformer_amd import interpret as I
    attn, acts, targets, ids, parts, sizes = make_eval(B, ppc)
    args = (attn, acts, targets, ids, parts, sizes, KTOK, S, CLASSES)
    I.consistency_from_outputs(*(a[:64] if isinstance(a, np.ndarray) else a for a in args), device=True)       # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = I.consistency_from_outputs(*args, device=True)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = I.consistency_from_outputs(*args)
    t_host = time.perf_counter() - t0
    same = dev[0] == host[0] and dev[1] == host[1] and dev[2] == host[2]
    return dict(what=f"interpret.consistency_from_outputs, {B} images x {ppc} prototypes = {B * ppc} maps {G}x{G} -> {S}, {KTOK} of {G * G} tokens reserved, "
                     f"{NPARTS} parts; wall clock of the whole call from host inputs",
                host_path_s=round(t_host, 3), device_path_s=round(t_dev, 4), host_over_device=round(t_host / t_dev, 1),
                host_us_per_map=round(t_host / (B * ppc) * 1e6, 1), device_us_per_map=round(t_dev / (B * ppc) * 1e6, 3),
                same_score_effects_and_fractions=bool(same), score=host[0], cpu_threads=torch.get_num_threads())


def push_forward(images, reps):
    ms = push_forward_ms(256, reps)
    med = float(np.median(ms))
    nb = -(-images // 256)
    return dict(what="PPNet.push_forward, deit_small 2000x384, batch 256 (the forward's share of a consistency run)", runs=reps,
                ms_per_batch_median=round(med, 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), batches_for_the_test_set=nb,
                forward_s_for_the_test_set=round(med * nb / 1e3, 3))


def sweep(images, protos, reps):
    from protopformer_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5)
    d = torch.rand((images * protos, G, G), device=dev, generator=g) * 4.0
    maps = torch.log((d + 1) / (d + 1e-4))
    del d
    parts = torch.randint(0, S, (images, NPARTS, 3), device=dev, generator=g, dtype=torch.int32)
    parts[:, :, 0] = 1
    ms = timed_back_to_back({"peak": lambda: ops.act_peak(maps, S, parts, 36)}, reps)["peak"]
    med = float(np.median(ms))
    _, _, table = ops.act_peak(maps, S, parts, 36)
    return dict(what=f"all-prototype sweep: ppf_act_peak with the fused part table, {images} images x {protos} prototypes = {images * protos} maps "
                     f"{G}x{G} -> {S}, one launch, device only (HIP events)", runs=reps, ms_median=round(med, 3), ms_min=round(min(ms), 3),
                ms_max=round(max(ms), 3), us_per_map=round(med * 1e3 / (images * protos), 4),
                upsampled_values_per_s=round(images * protos * S * S / (med * 1e-3), 0), table_bytes_read_back=int(table.numel()),
                table_ones=int(table.sum()))


def upsample(reps, M=2560):
    from protopformer_amd import ops
    maps = torch.from_numpy(activation_like((M, G, G), 9)).cuda()
    ms = timed_back_to_back({"up": lambda: ops.act_upsample(maps, S)}, reps)["up"]
    med = float(np.median(ms))
    nbytes = M * (G * G + S * S) * 4
    return dict(what=f"ppf_act_upsample alone, {M} maps {G}x{G} -> {S}x{S} (HIP event pairs; the output buffer is allocated inside the pair)", runs=reps,
                us_median=round(med * 1e3, 1), us_min=round(min(ms) * 1e3, 1), us_max=round(max(ms) * 1e3, 1), algorithmic_bytes=nbytes,
                gb_per_s_at_median=round(nbytes / (med * 1e-3) / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5794, help="CUB's test set")
    ap.add_argument("--ppc", type=int, default=10)
    ap.add_argument("--sweep-images", type=int, default=256)
    ap.add_argument("--sweep-protos", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "interp_device_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_interp.py measures on the GPU; none found")
    head = [f"# interpretability post-processing cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}, numpy {np.__version__}",
            f"# produced by: python scripts/bench_interp.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# device times are HIP events around single launches on an otherwise idle stream; path times are perf_counter around a call that ends in a synchronise"]
    print("\n".join(head), flush=True)
    rows = []
    for fn in (lambda: upsample(a.reps), lambda: sweep(a.sweep_images, a.sweep_protos, a.reps), lambda: push_forward(a.images, 5),
               lambda: consistency(a.images, a.ppc)):
        rows.append(json.dumps(fn()))
        print(rows[-1], flush=True)
    text = "\n".join(head + rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
