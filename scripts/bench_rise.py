"""Cost of the RISE saliency pass (interpret.rise_saliency) on one MI355X -- profiles/rise_cost.txt.

    python scripts/bench_rise.py [--batch 256 --masks 512 --cells 7 --reps 10 --rounds 3] [--out profiles/rise_cost.txt] [--variant TEXT]

At the deit_small shape (3 x 224 x 224 images, batch 256, a 196-cell grid, one class per image, s = 7, N = 512 masks, a 1 GiB chunk of
masked images) it measures
  * ppf_rise_nodes (all N masks), ppf_rise_apply (one chunk; constant and tensor baseline) and ppf_rise_accumulate (all N masks): HIP
    events around every single launch, queued behind a running matrix product so that the host's enqueue time is not in the figure;
  * the yardstick of ppf_rise_apply in the same run, alternating with it round by round: ppf_patch_perturb writing the same number of
    bytes, and a write-only fill of those bytes; the ratio of the write rates is reported;
  * for scale: PPNet.push_forward of the batch (the pass forwards N such batches), and the torch alternative on the device for one chunk:
    F.interpolate of the [Nc * B, 1, s + 1, s + 1] grids, crops at random offsets, and a broadcast multiply-add.
With PPF_LIB_PATH naming a measurement build of the library (python -m protopformer_amd.build --variant TAG DEFINE: PPF_RISE_KNOCKOUT=1 a
constant mask, =2 no LDS staging either, PPF_RISE_CH=1 one channel per thread) and --variant TEXT, only the ppf_rise_apply rows are
measured, labelled TEXT and appended to --out: what each knocked-out part costs next to the writes.
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

from bench_common import push_forward_row, row, timed      # noqa: E402

GRID, IMG = 196, 224


def kernels(B, N, s, reps, rounds, variant):
    from protopformer_amd import ops
    from protopformer_amd.interpret import rise_threshold
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1028)
    x = torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    thr, L = rise_threshold(0.5), s + 2
    img = x[0].numel() * 4
    Nc = max(1, min(N, (1 << 30) // (B * img)))
    written = Nc * B * img
    shape = f"B={B} s={s} 3x{IMG}x{IMG}"
    rows = []
    nodes, shift = ops.rise_nodes(ids, IMG, N, s, thr, 7)
    out = torch.empty((Nc, B, 3, IMG, IMG), device=dev)
    tag = f" [measurement build: {variant}]" if variant else ""
    cands = {"ppf_rise_apply, constant baseline": lambda: ops.rise_apply(x, nodes, shift, s, 0, Nc, 0.0, out=out)}
    if not variant:
        rank = torch.rand((B, 1, GRID), device=dev, generator=g).argsort(-1).to(torch.int32).contiguous()
        counts = torch.linspace(0, GRID, Nc, device=dev).to(torch.int32).contiguous()
        pout = out.view(Nc, B, 1, 3, IMG, IMG)
        cands["yardstick: ppf_patch_perturb, deletion, constant baseline, same bytes written"] = lambda: ops.patch_perturb(x, rank, counts, False, 0.0, out=pout)
        cands["yardstick: fill of the same bytes (write only)"] = lambda: out.fill_(1.0)
    med = {k: [] for k in cands}
    for r in range(rounds):                                                     # alternating: every round times each candidate once
        for k, fn in cands.items():
            t = timed(fn, reps)
            med[k].append(t["us_median"])
            nbytes = written + (0 if "fill" in k else B * img) + (Nc * B * (L * L + 8) if "rise" in k else 0)
            rows.append(row(f"round {r}: {k}{tag}, Nc={Nc} {shape}", t, nbytes, bytes_written=written, tb_per_s_written=round(written / t["us_median"] / 1e6, 3)))
    if variant:
        return rows
    a, p = (float(np.median(med[k])) for k in list(cands)[:2])
    rows.append(dict(what="ppf_rise_apply against ppf_patch_perturb, medians of the rounds' medians", rise_apply_us=a, patch_perturb_us=p,
                     rise_apply_tb_per_s=round(written / a / 1e6, 3), patch_perturb_tb_per_s=round(written / p / 1e6, 3),
                     write_rate_ratio=round(p / a, 3)))
    base = torch.zeros_like(x)
    t = timed(lambda: ops.rise_apply(x, nodes, shift, s, 0, Nc, base, out=out), reps)
    rows.append(row(f"ppf_rise_apply, tensor baseline, Nc={Nc} {shape}", t, written + 2 * B * img, bytes_written=written))
    t_nodes = timed(lambda: ops.rise_nodes(ids, IMG, N, s, thr, 7), reps)
    rows.append(row(f"ppf_rise_nodes, N={N} {shape}", t_nodes, B * N * (L * L + 8) + B * 8))
    prob = torch.rand((N, B, 1), device=dev, generator=g)
    t_acc = timed(lambda: ops.rise_accumulate(nodes, shift, prob, IMG, s, GRID, thr), max(3, reps // 3))
    rows.append(row(f"ppf_rise_accumulate (pixels and cells), N={N} M=1 G={GRID} {shape}", t_acc, B * N * (L * L + 8 + 4) + B * (IMG * IMG + GRID) * 4))
    # the torch alternative for one chunk, on the device
    import torch.nn.functional as F
    c = -(-IMG // s)

    def alternative():
        grid = (torch.rand((Nc * B, 1, s + 1, s + 1), device=dev) < 0.5).float()
        up = F.interpolate(grid, size=((s + 1) * c, (s + 1) * c), mode="bilinear", align_corners=False)
        dy, dx = torch.randint(0, c, (2,)).tolist()                             # one offset per chunk: per-mask offsets would need a gather on top
        m = up[:, :, dy:dy + IMG, dx:dx + IMG].reshape(Nc, B, 1, IMG, IMG)
        torch.mul(m, x[None], out=out)
    t = timed(alternative, min(reps, 5), warm=1)
    rows.append(dict(what=f"torch alternative on the device for one chunk: rand, F.interpolate of [{Nc * B}, 1, {s + 1}, {s + 1}] grids, one crop, broadcast "
                          "multiply (baseline 0, masks tied to the generator's state)", **t, bytes_written=written))
    del out, base
    torch.cuda.empty_cache()
    fwd = push_forward_row(B, 5, f"for scale: PPNet.push_forward, deit_small 2000x384, batch {B}")
    rows.append(fwd)
    chunks = -(-N // Nc)
    own_ms = (t_nodes["us_median"] + chunks * a + t_acc["us_median"]) / 1e3
    rows.append(dict(what=f"share: the three kernels over a pass of N={N} masks ({chunks} chunks) against the {N} forwards of batch {B} they serve (push_forward as the forward)",
                     kernels_ms=round(own_ms, 3), forwards_ms=round(N * fwd["ms_median"], 1), share_percent=round(100 * own_ms / (N * fwd["ms_median"]), 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--masks", type=int, default=512)
    ap.add_argument("--cells", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", type=str, default="", help="the loaded library (PPF_LIB_PATH) is this measurement build: time ppf_rise_apply only and append")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "rise_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rise.py measures on the GPU; none found")
    rows = kernels(a.batch, a.masks, a.cells, a.reps, a.rounds, a.variant)
    head = [] if a.variant else [
        f"# RISE saliency cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
        f"# produced by: python scripts/bench_rise.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
        "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.variant else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
