"""Cost of the per-pixel faithfulness pass (interpret.faithfulness_curves with resolution="pixel", baseline="blur") on one MI355X --
profiles/pixel_faithfulness_cost.txt.

    python scripts/bench_pixel_faithfulness.py [--batch 256 --steps 15 --reps 20] [--out profiles/pixel_faithfulness_cost.txt]

At the deit_small shape (3 x 224 x 224 images, n = 50 176 pixels, batch 256, one class per image, `steps` points per curve) it measures,
with HIP events around every single launch, queued behind a running matrix product so that the host's enqueue time is not in the figure,
`reps` launches after 3 warm-up launches, all in this one run:
  * ppf_pixel_order on three kinds of scores -- normal values (all four radix passes), a 14 x 14 grid with 81 occupied cells up-sampled
    by ppf_act_upsample (what the evidence order ranks) and seven distinct values (passes skipped) -- against the torch alternative on the
    device, torch.argsort(descending=True, stable=True) plus the scatter of an arange (no NaN rule, no -0 rule);
  * ppf_pixel_random;
  * ppf_pixel_perturb (all steps of one curve in one launch; constant and tensor baseline) against ppf_patch_perturb writing the same
    bytes, and a write-only fill of as many bytes;
  * ppf_gauss_blur (radius 5) of the batch against a device copy of the same bytes and against depthwise F.conv2d (one 11 x 11 kernel
    with zero padding, and the separable pair 1 x 11, 11 x 1);
  * for scale: PPNet.push_forward of the same batch, and the share of the per-pixel launches in the `steps` forwards of a curve.
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

GRID, KTOK, IMG = 196, 81, 224


def order_rows(B, reps, dev):
    from protopformer_amd import _lib, ops
    from protopformer_amd.interpret import upsample_cubic_device
    g = torch.Generator(device=dev).manual_seed(1028)
    n = IMG * IMG
    grid = torch.rand((B, GRID), device=dev, generator=g)
    grid = torch.where(torch.rand((B, GRID), device=dev, generator=g).argsort(1) < KTOK, grid, torch.zeros_like(grid))
    kinds = (("normal scores", torch.randn((B, n), device=dev, generator=g)),
             ("an up-sampled 14 x 14 grid with 81 occupied cells", upsample_cubic_device(grid.reshape(B, 14, 14).contiguous(), IMG).reshape(B, n).contiguous()),
             ("seven distinct values", (torch.randint(0, 7, (B, n), device=dev, generator=g).float() / 4 - 1).contiguous()))
    cls = torch.zeros(B, dtype=torch.int32, device=dev)
    rank = torch.empty((B, n), dtype=torch.int32, device=dev)
    nbytes = _lib.lib().ppf_pixel_order_scratch_bytes(B, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    arange = torch.arange(n, device=dev, dtype=torch.int32).expand(B, n).contiguous()
    rows = []
    for name, score in kinds:
        t = timed(lambda: _lib.call("ppf_pixel_order", score, cls, B, n, rank, ws, nbytes), reps)
        rows.append(row(f"ppf_pixel_order, {name}, R={B} n={n}", t, B * n * 8, workgroups=min(B, 256), threads_per_workgroup=1024, scratch_bytes=nbytes))
        out = torch.empty((B, n), dtype=torch.int32, device=dev)

        def alternative():
            out.scatter_(1, torch.argsort(score, dim=1, descending=True, stable=True), arange)
        t2 = timed(alternative, min(reps, 10), warm=2)
        same = bool(torch.equal(out, ops.pixel_order(score, cls)))
        rows.append(dict(what=f"torch alternative on the device: argsort(descending, stable) + scatter of an arange, {name} (no NaN or -0 rule)", **t2,
                         equals_the_kernel=same, kernel_over_torch=round(t["us_median"] / t2["us_median"], 3)))
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    sc = torch.empty((B, n), device=dev)
    t = timed(lambda: _lib.call("ppf_pixel_random", ids, 7, B, n, sc), reps)
    rows.append(row(f"ppf_pixel_random, B={B} n={n}", t, B * n * 4 + B * 8))
    return rows


def perturb_rows(B, S, reps, dev):
    from protopformer_amd import ops
    from protopformer_amd.interpret import default_counts
    g = torch.Generator(device=dev).manual_seed(7)
    n, M = IMG * IMG, 1
    x = torch.randn((B, 3, IMG, IMG), device=dev, generator=g)
    prank = torch.rand((B, M, n), device=dev, generator=g).argsort(-1).to(torch.int32).contiguous()
    crank = torch.rand((B, M, GRID), device=dev, generator=g).argsort(-1).to(torch.int32).contiguous()
    pcounts = torch.from_numpy(default_counts(n, S - 1)).to(dev)
    ccounts = torch.from_numpy(default_counts(GRID, S - 1)).to(dev)
    S = pcounts.shape[0]
    img = x[0].numel() * 4
    out = torch.empty((S, B, M, 3, IMG, IMG), device=dev)
    written = S * B * M * img
    rows, med = [], {}
    for name, base in (("constant baseline", 0.0), ("tensor baseline", torch.zeros_like(x))):
        reads = B * img * (2 if isinstance(base, torch.Tensor) else 1)
        t = timed(lambda: ops.pixel_perturb(x, prank, pcounts, False, base, out=out), reps)
        rows.append(row(f"ppf_pixel_perturb, deletion, {name}, S={S} B={B} M={M} 3x{IMG}x{IMG}", t, written + reads + B * M * n * 4, bytes_written=written,
                        workgroups=B * n // 4 // 128))
        med["pixel", name] = t["us_median"]
        t = timed(lambda: ops.patch_perturb(x, crank, ccounts, False, base, out=out), reps)
        rows.append(row(f"ppf_patch_perturb writing the same bytes, deletion, {name}, S={S} B={B} M={M} G={GRID}", t, written + reads + B * M * GRID * 4,
                        bytes_written=written, workgroups=B * 3 * n // 4 // 128))
        med["patch", name] = t["us_median"]
        rows.append(dict(what=f"ratio ppf_pixel_perturb / ppf_patch_perturb, {name}", time_ratio=round(med["pixel", name] / med["patch", name], 4),
                         byte_ratio=round((written + reads + B * M * n * 4) / (written + reads + B * M * GRID * 4), 4)))
    t = timed(lambda: out.fill_(1.0), reps)
    rows.append(row(f"for scale: fill of the {written} bytes both write (write only)", t, written, bytes_written=written))
    del out
    # the blur of the same batch
    from protopformer_amd.interpret import gauss_taps
    taps = torch.from_numpy(gauss_taps()).to(dev)
    t = timed(lambda: ops.gauss_blur(x, taps), reps)
    rows.append(row(f"ppf_gauss_blur, radius 5, {B * 3} planes of {IMG}x{IMG}", t, 2 * B * img, workgroups=B * 3 * 4 * 14))
    dst = torch.empty_like(x)
    t = timed(lambda: dst.copy_(x), reps)
    rows.append(row("for scale: device-to-device copy of the same batch", t, 2 * B * img))
    import torch.nn.functional as F
    k2 = (taps[:, None] * taps[None, :])[None, None].expand(3, 1, 11, 11).contiguous()
    kh, kv = taps.reshape(1, 1, 1, 11).expand(3, 1, 1, 11).contiguous(), taps.reshape(1, 1, 11, 1).expand(3, 1, 11, 1).contiguous()
    t = timed(lambda: F.conv2d(x, k2, padding=5, groups=3), min(reps, 10), warm=2)
    rows.append(dict(what="torch alternative: depthwise F.conv2d, one 11 x 11 kernel, zero padding", **t))
    t = timed(lambda: F.conv2d(F.conv2d(x, kh, padding=(0, 5), groups=3), kv, padding=(5, 0), groups=3), min(reps, 10), warm=2)
    rows.append(dict(what="torch alternative: depthwise F.conv2d, separable pair 1 x 11 and 11 x 1, zero padding", **t))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=15, help="points per curve")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pixel_faithfulness_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_faithfulness.py measures on the GPU; none found")
    dev = torch.device("cuda")
    rows = order_rows(a.batch, a.reps, dev)
    torch.cuda.empty_cache()
    rows += perturb_rows(a.batch, a.steps, a.reps, dev)
    torch.cuda.empty_cache()
    rows.append(push_forward_row(a.batch, 5, f"for scale: PPNet.push_forward, deit_small 2000x384, batch {a.batch}"))
    head = [f"# per-pixel faithfulness (pixel order, perturbation, blur) cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_pixel_faithfulness.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# kernels: HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
