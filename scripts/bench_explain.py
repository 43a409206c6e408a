"""Cost of the local analysis (interpret.explain) on one MI355X -- profiles/explain_cost.txt.

    python scripts/bench_explain.py [--batch 256 --topk 10 --reps 50] [--out profiles/explain_cost.txt]

At the deit_small shape (2000 local and 2000 global prototypes, 200 classes, 81 reserved tokens on a 196-cell grid, batch 256) and for
M = 1 and M = 5 explained classes per image it measures
  * ppf_explain_topk: the local launch with and without maps and the global launch, HIP events around every single launch (queued behind a
    running matrix product, so the host's enqueue time is not in the figure), `reps` launches after 5 warm-up launches, on random activations quantised to 1/64 and last-layer weights of 1 / -0.5;
  * achieved GB/s of the median launch against its algorithmic bytes (per list the act_max and weight rows, the K argmax / idx reads and
    the outputs; with maps also K * (G * 4 written + T * 4 read));
  * PPNet.push_forward of one such batch, for scale;
  * the host alternative: read act_max and argmax back, torch.topk on act * W[cls] on the CPU, and interpret.expand_to_grid of all P
    maps on the device (what a caller without the kernel materialises to draw ten of them).
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import push_forward_row, timed      # noqa: E402

P, KTOK, GRID, CLASSES, COE = 2000, 81, 196, 200, 0.3


def make_batch(B, dev):
    g = torch.Generator(device=dev).manual_seed(1028)
    ppc = P // CLASSES
    own = (torch.arange(P, device=dev) // ppc)[None, :] == torch.arange(CLASSES, device=dev)[:, None]
    return dict(act=torch.randint(0, 640, (B, P), device=dev, generator=g).float() / 64.0,
                argmax=torch.randint(0, KTOK, (B, P), device=dev, generator=g).to(torch.int32),
                idx=torch.rand((B, GRID), device=dev, generator=g).argsort(1)[:, :KTOK].sort(1).values.to(torch.int32),
                act_full=torch.rand((B, P, KTOK), device=dev, generator=g), logits=torch.randn((B, CLASSES), device=dev, generator=g),
                weight=torch.where(own, 1.0, -0.5).contiguous(), attn=torch.rand((B, GRID), device=dev, generator=g), ppc=ppc)


def explain_launches(b, K, M, reps, local, maps):
    from protopformer_amd import _lib, ops
    B = b["act"].shape[0]
    kw = dict(argmax=b["argmax"], idx=b["idx"], act_full=b["act_full"], grid_cells=GRID, want_maps=maps) if local else {}
    scale = (1.0 - COE) if local else COE
    out = ops.explain_topk(b["act"], b["weight"], scale, b["ppc"], b["logits"], K, top_classes=M, **kw)      # allocates the outputs once
    args = (b["act"], kw.get("argmax"), kw.get("idx"), KTOK if local else 0, kw.get("act_full"), b["weight"], scale, b["ppc"], b["logits"], None, 1, B, P,
            CLASSES, M, K, GRID if local else 0, out["classes"], out["class_logits"], out["prototypes"], out["contributions"], out["activations"],
            out["cells"], out["evidence"], out["maps"])
    t = timed(lambda: _lib.call("ppf_explain_topk", *args), reps, warm=5)
    lists = B * M
    nbytes = lists * (P * 8 + CLASSES * 4 + K * 16 + 16) + (lists * K * 8 if local else 0) + (lists * K * (GRID + KTOK) * 4 + lists * KTOK * 4 if maps else 0)
    form = ("local, with maps" if maps else "local, no maps") if local else "global"
    return dict(what=f"ppf_explain_topk, {form}, B={B} P={P} C={CLASSES} M={M} K={K} T={KTOK} G={GRID}", launches_timed=t["launches_timed"],
                workgroups=lists, us_median=t["us_median"], us_min=t["us_min"], us_max=t["us_max"], algorithmic_bytes=nbytes,
                gb_per_s_at_median=round(nbytes / t["us_median"] / 1e3, 1), filled_entries=int((out["prototypes"] >= 0).sum()))


def host_alternative(b, K, M, reps):
    from protopformer_amd.interpret import expand_to_grid
    B = b["act"].shape[0]
    w = b["weight"].cpu() * (1.0 - COE)
    read, top = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        act, _ = b["act"].cpu(), b["argmax"].cpu()
        logits = b["logits"].cpu()
        read.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        cls = torch.topk(logits, M, dim=1).indices                                   # [B, M]
        best = torch.topk(act[:, None, :] * w[cls], K, dim=2)
        top.append((time.perf_counter() - t0) * 1e3)
    grid_ms = []
    for rep in range(3 + min(reps, 10)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        grid = expand_to_grid(b["act_full"], b["attn"], KTOK)
        e1.record()
        torch.cuda.synchronize()
        if rep >= 3:
            grid_ms.append(e0.elapsed_time(e1))
    return dict(what=f"host alternative, M={M}: act_max + argmax + logits read back, torch.topk({K}) of act * W[cls] on the CPU (no tie order, no "
                     f"evidence sums), expand_to_grid of all P maps on the device, {torch.get_num_threads()} CPU threads",
                readback_ms_median=round(float(np.median(read)), 3), readback_bytes=B * P * 8 + B * CLASSES * 4,
                cpu_topk_ms_median=round(float(np.median(top)), 3), expand_to_grid_ms_median=round(float(np.median(grid_ms)), 3),
                expand_to_grid_bytes_written=int(grid.numel()) * 4, checksum=float(best.values.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "explain_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_explain.py measures on the GPU; none found")
    dev = torch.device("cuda")
    b = make_batch(a.batch, dev)
    rows = []
    for M in (1, 5):
        rows += [explain_launches(b, a.topk, M, a.reps, True, True), explain_launches(b, a.topk, M, a.reps, True, False),
                 explain_launches(b, a.topk, M, a.reps, False, False)]
    rows += [host_alternative(b, a.topk, M, min(a.reps, 10)) for M in (1, 5)]
    del b
    torch.cuda.empty_cache()
    rows.append(push_forward_row(a.batch, 5, f"PPNet.push_forward, deit_small 2000x384, batch {a.batch} (for scale)"))
    head = [f"# local analysis (explain) cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_explain.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# ppf_explain_topk: HIP events around single launches queued behind a running kernel (no host enqueue time inside); host times are perf_counter"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
