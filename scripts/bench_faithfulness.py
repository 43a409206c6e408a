"""Cost of the faithfulness pass (interpret.faithfulness_curves) on one MI355X -- profiles/faithfulness_cost.txt.

    python scripts/bench_faithfulness.py [--batch 256 --steps 15 --reps 20] [--out profiles/faithfulness_cost.txt]

At the deit_small shape (2000 prototypes, 200 classes, 81 reserved tokens on a 196-cell grid, 3 x 224 x 224 images, batch 256, one
class per image, `steps` points per curve) it measures
  * ppf_cell_order (evidence, attention and random order), ppf_patch_perturb (all steps of one curve in one launch; constant and tensor
    baseline) and ppf_class_prob (the steps * batch logits rows of one curve): HIP events around every single launch, queued behind a
    running matrix product so that the host's enqueue time is not in the figure, `reps` launches after 3 warm-up launches;
  * the bytes each launch moves (computed from the shapes, below) and the GB/s of the median launch;
  * for scale: PPNet.push_forward of the same batch; a plain device-to-device copy and a fill of as many bytes as ppf_patch_perturb
    writes; and the host alternative -- interpret.expand_to_grid of all P maps, torch.einsum with the class's weight row, argsort, and
    the perturbed images by torch indexing, one step at a time.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

from bench_common import push_forward_row, row, timed      # noqa: E402

P, KTOK, GRID, CLASSES, COE, IMG = 2000, 81, 196, 200, 0.3, 224


def make_batch(B, dev):
    g = torch.Generator(device=dev).manual_seed(1028)
    ppc = P // CLASSES
    own = (torch.arange(P, device=dev) // ppc)[None, :] == torch.arange(CLASSES, device=dev)[:, None]
    return dict(act_full=torch.rand((B, P, KTOK), device=dev, generator=g), attn=torch.rand((B, GRID), device=dev, generator=g),
                idx=torch.rand((B, GRID), device=dev, generator=g).argsort(1)[:, :KTOK].sort(1).values.to(torch.int32).contiguous(),
                weight=torch.where(own, 1.0, -0.5).contiguous(), classes=torch.randint(0, CLASSES, (B, 1), device=dev, generator=g).to(torch.int32),
                ids=torch.arange(B, device=dev, dtype=torch.int64), x=torch.randn((B, 3, IMG, IMG), device=dev, generator=g))


def kernels(b, S, reps):
    from protopformer_amd import _lib, ops
    from protopformer_amd.interpret import default_counts
    B, M = b["classes"].shape
    rows, shape = [], f"B={B} M={M} P={P} C={CLASSES} T={KTOK} G={GRID}"
    order, rank, score = ops.cell_order(b["classes"], GRID, "evidence", act_full=b["act_full"], idx=b["idx"], token_attn=b["attn"], weight=b["weight"],
                                        scale=1.0 - COE)
    out_bytes = B * M * GRID * 12
    for mode, args, nbytes in (
            ("evidence", (b["act_full"], b["idx"], b["attn"], b["weight"], 1.0 - COE, b["classes"], None, 0, 0),
             B * M * (P * KTOK * 4 + P * 4 + 4) + B * (KTOK + GRID) * 4 + out_bytes),
            ("attention", (None, None, b["attn"], None, 1.0, b["classes"], None, 0, 1), B * M * 4 + B * GRID * 4 + out_bytes),
            ("random", (None, None, None, None, 1.0, b["classes"], b["ids"], 7, 2), B * M * 4 + B * 8 + out_bytes)):
        o2, r2, s2 = torch.empty_like(order), torch.empty_like(rank), torch.empty_like(score)
        t = timed(lambda: _lib.call("ppf_cell_order", *args, B, P, CLASSES, KTOK, GRID, M, o2, r2, s2), reps)
        rows.append(row(f"ppf_cell_order, {mode} order, {shape}", t, nbytes, workgroups=B * M, threads_per_workgroup=1024))
    counts = torch.from_numpy(default_counts(GRID, S - 1)).to(b["x"].device)
    S = counts.shape[0]
    img = b["x"][0].numel() * 4
    out = torch.empty((S, B, M, 3, IMG, IMG), device=b["x"].device)
    written = S * B * M * img
    for name, base in (("constant baseline", 0.0), ("tensor baseline", torch.zeros_like(b["x"]))):
        t = timed(lambda: ops.patch_perturb(b["x"], rank, counts, False, base, out=out), reps)
        nbytes = written + B * img * (2 if isinstance(base, torch.Tensor) else 1) + B * M * GRID * 4
        rows.append(row(f"ppf_patch_perturb, deletion, {name}, S={S} {shape} 3x{IMG}x{IMG}", t, nbytes, bytes_written=written,
                        workgroups=B * 3 * IMG * IMG // 4 // 128))
    src = torch.empty_like(out)
    t = timed(lambda: out.copy_(src), reps)
    rows.append(row(f"for scale: device-to-device copy of the {written} bytes ppf_patch_perturb writes (reads as many)", t, 2 * written, bytes_written=written))
    t = timed(lambda: out.fill_(1.0), reps)
    rows.append(row(f"for scale: fill of the {written} bytes ppf_patch_perturb writes (write only)", t, written, bytes_written=written))
    del src
    R = S * B * M
    logits = torch.randn((R, CLASSES), device=b["x"].device) * 4
    cls = b["classes"].reshape(1, -1).expand(S, -1).reshape(-1).contiguous()
    prob = torch.empty(R, device=b["x"].device)
    t = timed(lambda: _lib.call("ppf_class_prob", logits, cls, R, CLASSES, prob), reps)
    rows.append(row(f"ppf_class_prob, R={R} rows (S={S} x B={B} x M={M}) C={CLASSES}", t, R * CLASSES * 4 + R * 8, workgroups=(R + 3) // 4))
    # the host alternative, on the device with torch: all P maps on the grid, the evidence per cell, the order, the images step by step
    from protopformer_amd.interpret import expand_to_grid
    w = (b["weight"] * (1.0 - COE))[b["classes"][:, 0].long()]                        # [B, P]
    side, patch = int(GRID ** 0.5), IMG // int(GRID ** 0.5)

    def alternative():
        grid = expand_to_grid(b["act_full"].reshape(B, P, 9, 9), b["attn"], KTOK).reshape(B, P, GRID)
        ev = torch.einsum("bp,bpg->bg", w, grid)
        rk = ev.argsort(1, descending=True).argsort(1)
        pix = rk.reshape(B, side, side).repeat_interleave(patch, 1).repeat_interleave(patch, 2)[:, None]
        for s in range(S):
            out[s, :, 0] = torch.where(pix < counts[s], 0.0, b["x"])
    t = timed(alternative, min(reps, 5), warm=1)
    rows.append(dict(what=f"torch alternative on the device: expand_to_grid of all {P} maps ({B * P * GRID * 4} bytes), einsum, two argsorts, {S} torch.where "
                          "steps (no tier, no tie order, fp32 sums)", **t, bytes_written=written))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15, help="points per curve")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "faithfulness_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_faithfulness.py measures on the GPU; none found")
    b = make_batch(a.batch, torch.device("cuda"))
    rows = kernels(b, a.steps, a.reps)
    del b
    torch.cuda.empty_cache()
    rows.append(push_forward_row(a.batch, 5, f"for scale: PPNet.push_forward, deit_small 2000x384, batch {a.batch}"))
    head = [f"# faithfulness (deletion / insertion curves) cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_faithfulness.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
