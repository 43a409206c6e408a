"""Cost of the integrated-gradients pass (interpret.integrated_gradients) on one MI355X -- profiles/ig_cost.txt.

    python scripts/bench_ig.py [--batch 256 --steps 32 --reps 10 --rounds 3] [--out profiles/ig_cost.txt]

At the deit_small shape (3 x 224 x 224 images, batch 256, a 196-cell grid, one class per image) it measures
  * ppf_ig_point, ppf_ig_accumulate and ppf_ig_finish (constant and tensor baseline, first and later steps): HIP events around every
    single launch, queued behind a running matrix product so that the host's enqueue time is not in the figure; the bytes each moves
    are computed from the shapes;
  * next to each kernel, alternating with it round by round in the same run, its yardstick: a device copy that moves the same number
    of bytes (half read, half written); the ratio of the two times is reported;
  * the whole pass at --steps midpoint steps next to the --steps forward + backward pairs (interpret.input_gradient on the same batch)
    it serves, and the share of the three kernels in the pass;
  * the completeness gap |delta| / |value - value_base| on the two micro fixtures (64 x 64 images, random weights of the reference's
    fixtures, top 2 classes), in the fp32 mode and on the bf16 product path, at 8, 32 and 128 midpoint steps: mean and worst.  The token
    reservation's top-k makes the model discontinuous along the path, so the gap need not fall with the steps; nothing is gated.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import deit_small_ppnet, row, timed      # noqa: E402

GRID, IMG, PATCH = 196, 224, 16


def kernels(B, reps, rounds):
    """The rows of the three kernels with their copy yardsticks, and {kernel: median of the rounds' medians in us}."""
    from protopformer_amd import ops
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1028)
    x = torch.randn((B, 3, IMG, IMG), device=dev, generator=gen)
    base = torch.randn(x.shape, device=dev, generator=gen)
    g = torch.randn(x.shape, device=dev, generator=gen)
    acc = torch.randn((B, 1, 3, IMG, IMG), device=dev, generator=gen)
    out = torch.empty_like(x)
    N = x.numel() * 4                                                           # bytes of one image-sized tensor
    shape = f"B={B} 3x{IMG}x{IMG}"
    cands = {
        "ppf_ig_point, constant baseline": (lambda: ops.ig_point(x, 0.3, 0.0, out=out), 2 * N),
        "ppf_ig_point, tensor baseline": (lambda: ops.ig_point(x, 0.3, base, out=out), 3 * N),
        "ppf_ig_accumulate, first step (acc written, not read)": (lambda: ops.ig_accumulate(g, 0.03125, acc[:, 0], first=True), 2 * N),
        "ppf_ig_accumulate, later step": (lambda: ops.ig_accumulate(g, 0.03125, acc[:, 0]), 3 * N),
        "ppf_ig_finish, constant baseline, M=1": (lambda: ops.ig_finish(acc, x, 0.0, PATCH), 3 * N + B * GRID * 8),
        "ppf_ig_finish, tensor baseline, M=1": (lambda: ops.ig_finish(acc, x, base, PATCH), 4 * N + B * GRID * 8),
    }
    src = torch.randn((2 * N // 4,), device=dev, generator=gen)
    dst = torch.empty_like(src)
    copies = {nbytes: (lambda n=nbytes // 8: dst[:n].copy_(src[:n])) for nbytes in sorted({2 * N, 3 * N, 4 * N})}     # half read, half written
    rows, med = [], {k: [] for k in list(cands) + list(copies)}
    for r in range(rounds):                                                     # alternating: every round times each candidate and each copy once
        for k, (fn, nbytes) in cands.items():
            t = timed(fn, reps)
            med[k].append(t["us_median"])
            rows.append(row(f"round {r}: {k}, {shape}", t, nbytes))
        for nbytes, fn in copies.items():
            t = timed(fn, reps)
            med[nbytes].append(t["us_median"])
            rows.append(row(f"round {r}: yardstick: device copy moving {nbytes // N} image-sized tensors' bytes (half read, half written), {shape}", t, nbytes))
    best = {k: float(np.median(v)) for k, v in med.items()}
    for k, (_, nbytes) in cands.items():
        copy_us = best[nbytes - nbytes % N]
        rows.append(dict(what=f"{k} against the device copy of the same bytes, medians of the rounds' medians", kernel_us=best[k], copy_us=copy_us,
                         kernel_tb_per_s=round(nbytes / best[k] / 1e6, 3), copy_tb_per_s=round((nbytes - nbytes % N) / copy_us / 1e6, 3),
                         rate_ratio_to_copy=round(copy_us / best[k], 3)))
    return rows, best


def whole_pass(B, steps, best, runs=3):
    """integrated_gradients at `steps` midpoint steps against the forward + backward pairs it serves, and the kernels' share."""
    from protopformer_amd.interpret import input_gradient, integrated_gradients
    m = deit_small_ppnet()
    x = torch.randn((B, 3, IMG, IMG), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    cls = torch.zeros(B, dtype=torch.int64, device="cuda")

    def ms_of(fn):
        fn()                                                                    # warm-up
        out = []
        for _ in range(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def pairs():
        for _ in range(steps):
            input_gradient(m, x, ("logit", cls))
    t_pass, t_pairs = ms_of(lambda: integrated_gradients(m, x, target=("logit", cls), steps=steps)), ms_of(pairs)
    own_us = steps * (best["ppf_ig_point, constant baseline"] + best["ppf_ig_accumulate, later step"]) + best["ppf_ig_finish, constant baseline, M=1"]
    p, q = float(np.median(t_pass)), float(np.median(t_pairs))
    return [dict(what=f"the whole pass: integrated_gradients, deit_small 2000x384, batch {B}, {steps} midpoint steps, one class, constant baseline "
                      "(two eval forwards, the steps, ppf_ig_finish; host enqueue inside)", runs=runs, ms_median=round(p, 3), ms_min=round(min(t_pass), 3),
                 ms_max=round(max(t_pass), 3)),
            dict(what=f"for scale: the {steps} forward + backward pairs it serves (interpret.input_gradient on the same batch)", runs=runs,
                 ms_median=round(q, 3), ms_min=round(min(t_pairs), 3), ms_max=round(max(t_pairs), 3)),
            dict(what=f"share: {steps} x (ppf_ig_point + ppf_ig_accumulate) + ppf_ig_finish, from the single-launch medians above, over the pass",
                 kernels_ms=round(own_us / 1e3, 3), pass_ms=round(p, 3), share_percent=round(100 * own_us / 1e3 / p, 3),
                 pass_over_pairs=round(p / q, 4))]


def completeness(step_counts=(8, 32, 128)):
    """|delta| / |value - value_base| of the top 2 classes on the micro fixtures, fp32 mode and product path: mean and worst per step count."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import build_micro, micro
    from protopformer_amd.interpret import integrated_gradients
    rows = []
    for fixture in ("micro_deit.npz", "micro_cait.npz"):
        sd, cfg, z = micro(fixture)
        x = torch.from_numpy(z["img"]).cuda()
        for precise in (True, False):
            m = build_micro(cfg, sd).eval()
            m.precise = precise
            for steps in step_counts:
                h = integrated_gradients(m, x, top_classes=2, steps=steps).cpu()
                gap, span = np.abs(h.delta()), np.abs(h.value.astype(np.float64) - h.value_base.astype(np.float64))
                rows.append(dict(what=f"completeness gap: {fixture}, {'fp32 mode' if precise else 'bf16 product path'}, {steps} midpoint steps, "
                                      f"{x.shape[0]} images x top 2 classes", mean_rel_gap=round(float((gap / span).mean()), 5),
                                 worst_rel_gap=round(float((gap / span).max()), 5), mean_abs_gap=round(float(gap.mean()), 5),
                                 mean_abs_span=round(float(span.mean()), 5)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ig_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ig.py measures on the GPU; none found")
    rows, best = kernels(a.batch, a.reps, a.rounds)
    torch.cuda.empty_cache()
    rows += whole_pass(a.batch, a.steps, best)
    torch.cuda.empty_cache()
    rows += completeness()
    head = [f"# integrated-gradients cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_ig.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
