"""Cost of the stability score on one MI355X -- profiles/stability_cost.txt.

    python scripts/bench_stability.py [--images 5794 --batch 256 --ppc 10 --reps 20 --knockouts] [--out profiles/stability_cost.txt]

  1. ppf_add_gauss_noise at --batch x 3 x 224 x 224 (one read and one write of the batch) next to a plain device-to-device copy of the
     same bytes and next to `x + std * torch.randn_like(x)`: HIP event pairs around single launches, the three alternating inside every
     repetition, --reps repetitions after warm-up.  --knockouts repeats the kernel's timing in child processes on measurement builds of
     the library (python -m protopformer_amd.build --variant noiseko<N> PPF_NOISE_KO=<N>; N = 1: a counter hash instead of Philox,
     2: the fast logarithm, 3: the fast sine / cosine), which shows what the kernel waits for if it is not the memory.
  2. What the device path of interpret.interpretability_scores adds to a batch beyond its two push_forwards: the noise, expand_to_grid and
     ppf_act_peak for the clean and the noisy pass, one ppf_part_meter_update; event pairs around each and around the whole sequence.
  3. Wall clock of interpret.interpretability_scores over --images synthetic images (deit_small, 200 classes x --ppc prototypes, 81 of 196
     tokens reserved, random weights, random part locations) with device=True and device=False; the two results are compared.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import deit_small_ppnet, timed_back_to_back      # noqa: E402

G, S, KTOK, NPARTS, CLASSES = 14, 224, 81, 15, 200


def spread(us):
    return dict(us_median=round(float(np.median(us)), 1), us_min=round(min(us), 1), us_max=round(max(us), 1))


def alternate(fns, reps):
    """{name: [us per repetition]} of bench_common.timed_back_to_back."""
    return {k: [ms * 1e3 for ms in v] for k, v in timed_back_to_back(fns, reps).items()}


def noise(batch, reps, kernel_only=False):
    from protopformer_amd import ops
    x = torch.randn((batch, 3, S, S), device="cuda")
    out = torch.empty_like(x)
    ids = torch.arange(1, batch + 1, device="cuda")
    fns = {"kernel": lambda: ops.add_gauss_noise(x, ids, 0.2, 0, out=out)}
    if not kernel_only:
        fns["copy"] = lambda: out.copy_(x)
        fns["torch"] = lambda: x + 0.2 * torch.randn_like(x)
    us = alternate(fns, reps)
    nbytes = 2 * x.numel() * 4
    row = dict(what=f"ppf_add_gauss_noise, {batch} x 3 x {S} x {S} fp32, out of place into an existing buffer; one read + one write = {nbytes} bytes "
                    "(HIP event pairs around single launches, the candidates alternating)", runs=reps, library=os.path.basename(os.environ.get("PPF_LIB_PATH", "libppf_hip.so")),
               kernel=dict(spread(us["kernel"]), gb_per_s_at_median=round(nbytes / np.median(us["kernel"]) / 1e3, 1)))
    if not kernel_only:
        row["device_to_device_copy"] = dict(spread(us["copy"]), gb_per_s_at_median=round(nbytes / np.median(us["copy"]) / 1e3, 1))
        row["x_plus_std_times_randn_like"] = spread(us["torch"])
        row["kernel_over_copy"] = round(float(np.median(us["kernel"]) / np.median(us["copy"])), 3)
    return row


def knockouts(batch, reps):
    """The kernel's time on the measurement builds, each in a process of its own (PPF_LIB_PATH selects the library)."""
    rows = []
    for n, what in ((1, "a counter hash instead of Philox4x32-10"), (2, "__logf instead of logf"), (3, "__sinf / __cosf instead of sincospif")):
        lib = os.path.join(ROOT, "protopformer_amd", "lib", f"libppf_hip_noiseko{n}.so")
        if not os.path.exists(lib):
            rows.append(dict(what=f"knock-out {n} ({what})", skipped=f"{os.path.basename(lib)} not built"))
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-noise", "--batch", str(batch), "--reps", str(reps)],
                           env=dict(os.environ, PPF_LIB_PATH=lib), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"knock-out {n} failed:\n{r.stdout}\n{r.stderr}")
        row = json.loads(r.stdout.strip().splitlines()[-1])
        rows.append(dict(what=f"knock-out {n}: {what}; the noise is wrong on purpose, only the time counts", library=row["library"], kernel=row["kernel"]))
    return rows


def attribution(full, kos):
    """What the knock-outs say: the median each one saves against the full kernel of the same run, next to the copy."""
    names = ("philox", "logf", "sincospif")
    saved = {n: round(full["kernel"]["us_median"] - k["kernel"]["us_median"], 1) for n, k in zip(names, kos) if "kernel" in k}
    return dict(what="ppf_add_gauss_noise against the copy: microseconds of the median each knock-out saves (child processes: compare with the spread "
                     "between min and max of the rows above)", kernel_us=full["kernel"]["us_median"], copy_us=full["device_to_device_copy"]["us_median"],
                us_saved_without=saved, largest=max(saved, key=saved.get) if saved else None)


def make_parts(ids, rng):
    sizes = {int(i): (int(rng.integers(300, 500)), int(rng.integers(250, 400))) for i in ids}
    locs = {}
    for i in ids:
        w, h = sizes[int(i)]
        locs[int(i)] = [[p, float(rng.random() * (w - 1)), float(rng.random() * (h - 1))] for p in range(1, NPARTS + 1) if rng.random() < 0.75]
    return types.SimpleNamespace(id_to_part_loc=locs), sizes


def per_batch(batch, ppc, reps):
    from protopformer_amd import interpret as I
    rng = np.random.default_rng(1028)
    s = int(round(KTOK ** 0.5))
    ids = np.arange(1, batch + 1)
    parts, sizes = make_parts(ids, rng)
    x = torch.randn((batch, 3, S, S), device="cuda")
    ids_dev = torch.from_numpy(ids).cuda()
    attn = [torch.rand((batch, G * G), device="cuda") for _ in range(2)]
    d = [torch.rand((batch, ppc, s, s), device="cuda") * 4.0 for _ in range(2)]
    acts = [torch.log((v + 1) / (v + 1e-4)) for v in d]
    labels = (torch.arange(batch, device="cuda") % CLASSES).long()
    plist = torch.from_numpy(I._part_list(ids, parts, sizes, S, NPARTS)[0]).cuda()
    grids = [I._grid_on_device(attn[j], acts[j], KTOK) for j in range(2)]
    tables = [I._tables_for_parts(grids[j], plist, S, 36) for j in range(2)]
    meter = I.PartMeter(CLASSES, ppc, NPARTS, "cuda")

    def whole():
        I.add_input_noise(x, ids_dev, 0.2, 0)
        t = [I._tables_for_parts(I._grid_on_device(attn[j], acts[j], KTOK), plist, S, 36) for j in range(2)]
        meter.update(t[0], plist, labels, t[1])

    us = alternate({"noise": lambda: I.add_input_noise(x, ids_dev, 0.2, 0),
                    "expand_to_grid_x2": lambda: [I._grid_on_device(attn[j], acts[j], KTOK) for j in range(2)],
                    "act_peak_x2": lambda: [I._tables_for_parts(grids[j], plist, S, 36) for j in range(2)],
                    "meter_update": lambda: meter.update(tables[0], plist, labels, tables[1]),
                    "whole_sequence": whole}, reps)
    return dict(what=f"device path of interpretability_scores per batch beyond the two push_forwards: batch {batch}, {ppc} prototypes per class, "
                     f"{batch * ppc} maps {G}x{G} -> {S} per pass, {NPARTS} parts, {CLASSES} classes (HIP event pairs; the noise allocates its output inside the pair; "
                     "the part list's host construction and upload are not in these figures)", runs=reps, **{k: spread(v) for k, v in us.items()})


class SyntheticSet:
    """--images random images in batches, the same ones on every pass (seeded device generator); ids 1.., labels id % classes."""

    def __init__(self, images, batch):
        self.images, self.batch = images, batch

    def __iter__(self):
        g = torch.Generator(device="cuda").manual_seed(1028)
        for b in range(0, self.images, self.batch):
            n = min(self.batch, self.images - b)
            ids = torch.arange(b + 1, b + 1 + n)
            yield torch.randn((n, 3, S, S), device="cuda", generator=g), (ids - 1) % CLASSES, ids


def end_to_end(images, batch, ppc):
    from protopformer_amd import interpret as I
    m = deit_small_ppnet(prototypes=CLASSES * ppc)
    parts, sizes = make_parts(np.arange(1, images + 1), np.random.default_rng(7))
    I.interpretability_scores(m, SyntheticSet(min(images, 2 * batch), batch), parts, sizes, num_classes=CLASSES, device=True)      # warm-up
    torch.cuda.synchronize()
    t = {}
    res = {}
    for name, dev in (("device", True), ("host", False)):
        t0 = time.perf_counter()
        res[name] = I.interpretability_scores(m, SyntheticSet(images, batch), parts, sizes, num_classes=CLASSES, device=dev)
        torch.cuda.synchronize()
        t[name] = time.perf_counter() - t0
    return dict(what=f"interpret.interpretability_scores, {images} synthetic images in batches of {batch}, deit_small, {CLASSES} x {ppc} prototypes, {KTOK} of {G * G} "
                     "tokens reserved, noise_std 0.2: wall clock of the whole call (two push_forwards per batch included) ending in a synchronise",
                device_true_s=round(t["device"], 3), device_false_s=round(t["host"], 3), host_over_device=round(t["host"] / t["device"], 1),
                same_result=bool(res["device"] == res["host"]), consistency=res["device"]["consistency"], stability=res["device"]["stability"],
                cpu_threads=torch.get_num_threads())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5794, help="CUB's test set")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ppc", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--knockouts", action="store_true", help="also time the kernel on the noiseko1..3 measurement builds")
    ap.add_argument("--child-noise", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "stability_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stability.py measures on the GPU; none found")
    if a.child_noise:
        print(json.dumps(noise(a.batch, a.reps, kernel_only=True)), flush=True)
        return
    head = [f"# stability score cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}, numpy {np.__version__}",
            f"# produced by: python scripts/bench_stability.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# device times are HIP events around single launches on an otherwise idle stream; path times are perf_counter around a call that ends in a synchronise"]
    print("\n".join(head), flush=True)
    rows = []
    def noise_rows():
        full = noise(a.batch, a.reps)
        if not a.knockouts:
            return [full]
        kos = knockouts(a.batch, a.reps)
        return [full] + kos + [attribution(full, kos)]

    for fn in (noise_rows, lambda: [per_batch(a.batch, a.ppc, a.reps)], lambda: [end_to_end(a.images, a.batch, a.ppc)]):
        for row in fn():
            rows.append(json.dumps(row))
            print(rows[-1], flush=True)
    text = "\n".join(head + rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
