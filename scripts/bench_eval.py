"""Cost of a validation epoch on one MI355X: engine.evaluate (four host read-backs per batch) against engine.evaluate_epoch (metrics
accumulated on the device by ppf_eval_metrics, one read-back per epoch) -- profiles/eval_cost.txt.

    python scripts/bench_eval.py [--warmup 5 --epochs 20 --batches 16 --batch 384] [--iters 200]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/bench_eval.py --kernel-only --iters 50      (kernel times:
                                                                                 python scripts/rocpd_stats.py DIR/p_results.db 10)

deit_small with 2000 x 384 prototypes in eval mode over `batches` batches of `batch` random images that already live on the device
(16 x 384 = 6144 images ~ CUB's 5794 test images), so that the loop measured is forward + metrics, not JPEG decoding.  Both loops run
in one process, warmed up, in alternating epochs; the time of an epoch is a host clock around a loop that ends in a synchronise
(both loops end in a read-back).  The metrics entry point alone: HIP events around `iters` back-to-back calls at batch x 200.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np      # noqa: E402
import torch            # noqa: E402

from bench_common import deit_small_ppnet      # noqa: E402


def epochs(warmup, timed, nbatch, B):
    from protopformer_amd.engine import evaluate, evaluate_epoch
    dev, C = torch.device("cuda"), 200
    m = deit_small_ppnet()
    g = torch.Generator(device=dev).manual_seed(1028)
    data = [(torch.randn(B, 3, 224, 224, device=dev, generator=g), torch.randint(0, C, (B,), device=dev, generator=g)) for _ in range(nbatch)]
    loops = {"evaluate": lambda: evaluate(data, m, dev), "evaluate_epoch": lambda: evaluate_epoch(data, m, dev)}
    stats = {}
    for _ in range(warmup):
        for k, fn in loops.items():
            stats[k] = fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in loops}
    for _ in range(timed):
        for k, fn in loops.items():
            t0 = time.perf_counter()
            stats[k] = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    old, new = stats["evaluate"], stats["evaluate_epoch"]
    assert new["n"] == nbatch * B and all(new[k] == old[k] for k in ("acc1", "global_acc1", "local_acc1")), (old, new)
    out = {k: dict(median_ms=round(float(np.median(v)), 3), mean_ms=round(float(np.mean(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
           for k, v in ms.items()}
    out["delta_pct_median"] = round((out["evaluate_epoch"]["median_ms"] / out["evaluate"]["median_ms"] - 1.0) * 100.0, 2)
    out["loss_rel_gap"] = abs(new["loss"] - old["loss"]) / abs(old["loss"])
    print(json.dumps(dict(what=f"validation epoch, deit_small 2000x384 eval, {nbatch} x {B} images resident on the device", warmup_epochs=warmup,
                          timed_epochs=timed, **out, stats_evaluate=old, stats_evaluate_epoch=new)), flush=True)


def kernel(iters, B):
    from protopformer_amd import ops
    dev, C = torch.device("cuda"), 200
    g = torch.Generator(device=dev).manual_seed(0)
    x, xg, xl = (torch.randn(B, C, device=dev, generator=g) for _ in range(3))
    y = torch.randint(0, C, (B,), device=dev, generator=g)
    acc = torch.zeros(ops.EVAL_SLOTS, dtype=torch.float64, device=dev)
    for _ in range(10):
        ops.eval_metrics(acc, x, y, xg, xl)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.eval_metrics(acc, x, y, xg, xl)
    e1.record()
    torch.cuda.synchronize()
    host_us = (time.perf_counter() - t0) / iters * 1e6
    print(json.dumps(dict(what="ppf_eval_metrics (eval_metrics_kernel + eval_metrics_finish_kernel), three logit tensors", shape=[B, C], calls=iters,
                          us_per_call_device_events=round(e0.elapsed_time(e1) * 1e3 / iters, 2), us_per_call_host_clock=round(host_us, 2))),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch", type=int, default=384)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernel-only", action="store_true", help="only the back-to-back ppf_eval_metrics calls (for a profiler run)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none found")
    kernel(a.iters, a.batch)
    if not a.kernel_only:
        epochs(a.warmup, a.epochs, a.batches, a.batch)


if __name__ == "__main__":
    main()
