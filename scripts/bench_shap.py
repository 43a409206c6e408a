"""Cost of the KernelSHAP pass (interpret.kernel_shap) on one MI355X -- profiles/shap_cost.txt.

    python scripts/bench_shap.py [--batch 256 --samples 512 --cells 7 --reps 10 --rounds 3] [--out profiles/shap_cost.txt] [--variant TEXT]

At the deit_small shape (3 x 224 x 224 images, batch 256, a 196-cell grid, one class per image, s = 7 so d = 49 players, N = 512
samples, a 1 GiB chunk of masked images) it measures
  * ppf_shap_apply (one chunk; constant and tensor baseline): HIP events around every single launch, queued behind a running matrix
    product so that the host's enqueue time is not in the figure;
  * its yardstick in the same run, alternating with it round by round: ppf_patch_perturb writing the same number of bytes, and a
    write-only fill of those bytes; the ratio of the write rates is reported;
  * the three small launches: ppf_shap_coalitions (all N samples), ppf_shap_gram and ppf_shap_solve, also at s = 14 (d = 196, N = 2048
    for the coalitions and the Gram sums), the largest system the solve accepts;
  * for scale: PPNet.push_forward of the batch (the pass forwards N + 2 such batches), the whole pass as a share of them, and the torch
    alternative on the device for one chunk: the membership bits unpacked, a repeat_interleave to pixel resolution and torch.where.
With PPF_LIB_PATH naming a measurement build of the library (python -m protopformer_amd.build --variant TAG DEFINE: PPF_SHAP_KNOCKOUT=1 no
LDS staging and no barrier, PPF_SHAP_CH=3 three channels per thread) and --variant TEXT, only the ppf_shap_apply rows and its yardsticks are
measured, labelled TEXT and appended to --out: what each part costs next to the writes.
Nobody has run the pass on a trained checkpoint: the figures are costs, not attributions.
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


def small_launches(B, N, s, M, reps, g):
    """Rows of the coalition draw, the Gram sums and the solve at s players per side."""
    from protopformer_amd import ops
    from protopformer_amd.interpret import shap_size_table
    dev = torch.device("cuda")
    d, Wd = s * s, (s * s + 31) // 32
    ids, table = torch.arange(B, device=dev, dtype=torch.int64), shap_size_table(d)
    shape = f"B={B} s={s} d={d} N={N} M={M}"
    coal = ops.shap_coalitions(ids, s, N, table, 7)
    t_coal = timed(lambda: ops.shap_coalitions(ids, s, N, table, 7), reps)
    val, v0 = torch.rand((N, B, M), device=dev, generator=g), torch.rand((B, M), device=dev, generator=g)
    v1 = torch.rand((B, M), device=dev, generator=g)
    A, bvec = ops.shap_gram(coal, val, v0, s)
    t_gram = timed(lambda: ops.shap_gram(coal, val, v0, s), max(3, reps // 3))
    t_solve = timed(lambda: ops.shap_solve(A, bvec, v0, v1, s, GRID), max(3, reps // 3))
    bad = int(ops.shap_solve(A, bvec, v0, v1, s, GRID)[2].sum())
    rows = [row(f"ppf_shap_coalitions (includes the upload of the {d - 1}-entry size table), {shape}", t_coal, B * N * Wd * 4 + B * 8),
            row(f"ppf_shap_gram, {shape}", t_gram, B * N * (Wd + M) * 4 + B * d * d * 4 + B * M * d * 8),
            row(f"ppf_shap_solve (fp64 Cholesky, factor in global scratch), G={GRID} {shape}, singular images: {bad}", t_solve,
                B * d * d * (4 + 2 * 8) + B * M * (d * 16 + GRID * 4))]
    return rows, t_coal, t_gram, t_solve


def kernels(B, N, s, reps, rounds, variant=""):
    from protopformer_amd import ops
    from protopformer_amd.interpret import shap_size_table
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1028)
    x = torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    d, Wd = s * s, (s * s + 31) // 32
    img = x[0].numel() * 4
    Nc = max(1, min(N, (1 << 30) // (B * img)))
    written = Nc * B * img
    shape = f"B={B} s={s} 3x{IMG}x{IMG}"
    rows = []
    coal = ops.shap_coalitions(ids, s, N, shap_size_table(d), 7)
    out = torch.empty((Nc, B, 3, IMG, IMG), device=dev)
    rank = torch.rand((B, 1, GRID), device=dev, generator=g).argsort(-1).to(torch.int32).contiguous()
    counts = torch.linspace(0, GRID, Nc, device=dev).to(torch.int32).contiguous()
    pout = out.view(Nc, B, 1, 3, IMG, IMG)
    tag = f" [measurement build: {variant}]" if variant else ""
    cands = {"ppf_shap_apply, constant baseline" + tag: lambda: ops.shap_apply(x, coal, s, 0, Nc, 0.0, out=out),
             "yardstick: ppf_patch_perturb, deletion, constant baseline, same bytes written": lambda: ops.patch_perturb(x, rank, counts, False, 0.0, out=pout),
             "yardstick: fill of the same bytes (write only)": lambda: out.fill_(1.0)}
    med = {k: [] for k in cands}
    for r in range(rounds):                                                     # alternating: every round times each candidate once
        for k, fn in cands.items():
            t = timed(fn, reps)
            med[k].append(t["us_median"])
            nbytes = written + (0 if "fill" in k else B * img) + (Nc * B * Wd * 4 if "shap" in k else 0)
            rows.append(row(f"round {r}: {k}, Nc={Nc} {shape}", t, nbytes, bytes_written=written, tb_per_s_written=round(written / t["us_median"] / 1e6, 3)))
    a, p, f = (float(np.median(med[k])) for k in cands)
    rows.append(dict(what="ppf_shap_apply against its yardsticks, medians of the rounds' medians" + tag, shap_apply_us=a, patch_perturb_us=p, fill_us=f,
                     shap_apply_tb_per_s=round(written / a / 1e6, 3), patch_perturb_tb_per_s=round(written / p / 1e6, 3),
                     write_rate_ratio_to_patch_perturb=round(p / a, 3), write_rate_ratio_to_fill=round(f / a, 3)))
    if variant:
        return rows
    base = torch.zeros_like(x)
    t = timed(lambda: ops.shap_apply(x, coal, s, 0, Nc, base, out=out), reps)
    rows.append(row(f"ppf_shap_apply, tensor baseline, Nc={Nc} {shape}", t, written + 2 * B * img, bytes_written=written))
    small, t_coal, t_gram, t_solve = small_launches(B, N, s, 1, reps, g)
    rows += small
    if s != 14:
        rows += small_launches(B, 2048, 14, 1, reps, g)[0]
    # the torch alternative for one chunk, on the device: unpack the bits, blow the s x s grid up to pixels, select
    shifts = torch.arange(32, device=dev, dtype=torch.int32)
    w = IMG // s

    def alternative():
        z = ((coal[:, :Nc, :, None] >> shifts) & 1).reshape(B, Nc, Wd * 32)[:, :, :d].bool().reshape(B, Nc, s, s)
        keep = z.repeat_interleave(w, dim=2).repeat_interleave(w, dim=3).permute(1, 0, 2, 3)[:, :, None]
        torch.where(keep, x[None], torch.zeros((), device=dev), out=out)
    t = timed(alternative, min(reps, 5), warm=1)
    rows.append(dict(what=f"torch alternative on the device for one chunk: unpack {Nc} x {B} coalitions, repeat_interleave to {IMG} x {IMG}, torch.where "
                          "(baseline 0)", **t, bytes_written=written))
    del out, base
    torch.cuda.empty_cache()
    fwd = push_forward_row(B, 5, f"for scale: PPNet.push_forward, deit_small 2000x384, batch {B}")
    rows.append(fwd)
    chunks = -(-N // Nc)
    own_ms = (t_coal["us_median"] + chunks * a + t_gram["us_median"] + t_solve["us_median"]) / 1e3
    rows.append(dict(what=f"share: the four kernels over a pass of N={N} samples ({chunks} chunks) against the {N + 2} forwards of batch {B} they serve "
                          "(push_forward as the forward)",
                     kernels_ms=round(own_ms, 3), forwards_ms=round((N + 2) * fwd["ms_median"], 1), share_percent=round(100 * own_ms / ((N + 2) * fwd["ms_median"]), 3)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--cells", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--variant", type=str, default="", help="the loaded library (PPF_LIB_PATH) is this measurement build: time ppf_shap_apply only and append")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "shap_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shap.py measures on the GPU; none found")
    rows = kernels(a.batch, a.samples, a.cells, a.reps, a.rounds, a.variant)
    head = [] if a.variant else [f"# KernelSHAP cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_shap.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)",
            "# costs only: nobody has run the pass on a trained checkpoint"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.variant else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
