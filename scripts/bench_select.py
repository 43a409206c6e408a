"""Launch times of the selection kernels that no other driver times alone, on one MI355X -- profiles/select_cost.txt.

    python scripts/bench_select.py [--reps 20] [--out profiles/select_cost.txt]

At the deit_small shapes (batch 256, N = 197 tokens in rows of NP = 200, L = 11 rollout layers, k = 81; 2560 activation maps 14 x 14
up-sampled to 224 x 224, the two ranks around the 95th percentile) it measures ppf_rollout_threshold (one layer), ppf_rollout with the
thresholds given and with the select inside the chain kernel, ppf_topk_sorted (256 x 196) and ppf_act_order_stats on random maps and on
maps of one value with one peak: HIP events around every single launch, queued behind a running matrix product, `reps` launches after
3 warm-up launches.  For a comparison of two builds run it once per library (PPF_LIB_PATH), alternating.
Prints one JSON line per measurement and writes them, with the device and the command line, to --out."""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

from bench_common import timed      # noqa: E402

B, N, NP, L, K, MAPS, GRID, SIZE = 256, 197, 200, 11, 81, 2560, 14, 224


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "select_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py measures on the GPU; none found")
    from protopformer_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1028)
    hm = torch.zeros((L, B, N, NP), device=dev)
    hm[..., :N] = torch.softmax(2.0 * torch.randn((L, B, N, N), device=dev, generator=g), dim=-1)
    thr = torch.empty((L, B), dtype=torch.int32, device=dev)
    for layer in range(L):
        ops.rollout_threshold(hm[layer], thr[layer], N)
    out = ops.rollout_outputs(B, N, K, 1, dev)
    scores = torch.rand((B, N - 1), device=dev, generator=g)
    random_maps = torch.rand((MAPS, GRID, GRID), device=dev, generator=g)
    peak_maps = torch.full((MAPS, GRID, GRID), 0.125, device=dev)
    peak_maps[:, 5, 9] = 1.0
    rank = int(0.95 * (SIZE * SIZE - 1))
    rows = []
    for what, fn in ((f"ppf_rollout_threshold, one layer, B={B} N={N} NP={NP}", lambda: ops.rollout_threshold(hm[0], thr[0], N)),
                     (f"ppf_rollout, thresholds given, L={L} B={B} N={N} k={K}", lambda: ops.rollout(hm, L, B, N, K, thr=thr, out=out)),
                     (f"ppf_rollout, select inside, L={L} B={B} N={N} k={K}", lambda: ops.rollout(hm, L, B, N, K, out=out)),
                     (f"ppf_topk_sorted, {B} x {N - 1}, k={K}", lambda: ops.topk_sorted(scores, K)),
                     (f"ppf_act_order_stats, random maps, M={MAPS} {GRID}x{GRID} -> {SIZE}", lambda: ops.act_order_stats(random_maps, SIZE, rank, rank + 1)),
                     (f"ppf_act_order_stats, one value and one peak, M={MAPS} {GRID}x{GRID} -> {SIZE}",
                      lambda: ops.act_order_stats(peak_maps, SIZE, rank, rank + 1))):
        rows.append(dict(what=what, **timed(fn, a.reps)))
    head = [f"# selection kernels: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_select.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# HIP events around single launches queued behind a running kernel (no host enqueue time inside)"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
