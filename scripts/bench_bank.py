"""Cost of the prototype bank on one MI355X -- profiles/proto_bank_cost.txt.

    python scripts/bench_bank.py [--batch 256 --batches 24 --topk 10 --reps 5] [--out profiles/proto_bank_cost.txt]

At the deit_small shape (2000 x 384 local prototypes, 2000 global, 81 reserved tokens, batch 256) it measures
  * ppf_proto_topk_merge, local (argmax + idx) and global (no argmax) branch, class-specific: HIP events around every launch of a
    simulated epoch (`batches` batches of random activations quantised to 1/64, unique image ids, 200 classes) into lists that start
    empty, `reps` epochs; the first launch of an epoch (empty lists: every offered candidate is inserted) is reported apart from the rest;
  * achieved GB/s of the median launch against its algorithmic bytes B*P*8 + B*k*4 + 2*P*K*12;
  * PPNet.push_forward of one such batch, for scale;
  * the host alternative: read act_max and argmax back every batch, concatenate and torch.topk on the CPU at the end.
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

from bench_common import push_forward_row      # noqa: E402

P, DP, KTOK, CLASSES = 2000, 384, 81, 200


def make_epoch(nbatch, B, dev):
    g = torch.Generator(device=dev).manual_seed(1028)
    out = []
    for i in range(nbatch):
        act = torch.randint(0, 640, (B, P), device=dev, generator=g).float() / 64.0
        argmax = torch.randint(0, KTOK, (B, P), device=dev, generator=g).to(torch.int32)
        idx = torch.rand((B, 196), device=dev, generator=g).argsort(1)[:, :KTOK].sort(1).values.to(torch.int32)
        tok = torch.rand((B, 1 + KTOK, DP), device=dev, generator=g)
        label = torch.randint(0, CLASSES, (B,), device=dev, generator=g)
        ids = torch.arange(i * B, (i + 1) * B, device=dev, dtype=torch.int32)
        out.append(dict(act=act, argmax=argmax, idx=idx, tok=tok, label=label, ids=ids))
    return out


def merge_launches(epoch, K, reps, local):
    from protopformer_amd import ops
    dev = epoch[0]["act"].device
    B = epoch[0]["act"].shape[0]
    val = torch.empty((P, K), dtype=torch.float32, device=dev)
    img, pos = (torch.empty((P, K), dtype=torch.int32, device=dev) for _ in range(2))
    feat = torch.zeros((P, DP), device=dev)
    first, rest, whole = [], [], []
    for rep in range(reps + 1):                                  # rep 0 warms up
        ops.proto_topk_init(val, img, pos)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in epoch]
        torch.cuda.synchronize()
        for (e0, e1), b in zip(ev, epoch):
            e0.record()
            ops.proto_topk_merge(b["act"], b["argmax"] if local else None, b["idx"] if local else None, b["tok"], 1 if local else 0, b["label"],
                                 b["ids"], P // CLASSES, val, img, pos, feat)
            e1.record()
        torch.cuda.synchronize()
        if rep:
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
            first.append(us[0]); rest += us[1:]; whole.append(ev[0][0].elapsed_time(ev[-1][1]) * 1e3 / len(epoch))
    nbytes = B * P * (8 if local else 4) + (B * KTOK * 4 if local else 0) + 2 * P * K * 12
    med = float(np.median(rest))
    return dict(what=f"ppf_proto_topk_merge, {'local (argmax + idx)' if local else 'global (no argmax)'}, class-specific, B={B} P={P} K={K} Dp={DP}",
                launches_timed=len(rest), us_median=round(med, 2), us_min=round(min(rest), 2), us_max=round(max(rest), 2),
                us_first_launch_median=round(float(np.median(first)), 2), us_per_launch_over_epoch=round(float(np.median(whole)), 2),
                algorithmic_bytes=nbytes, gb_per_s_at_median=round(nbytes / med / 1e3, 1), filled_entries=int((img >= 0).sum()))


def host_alternative(epoch, K):
    torch.cuda.synchronize()
    per_batch, acts, args = [], [], []
    for b in epoch:
        t0 = time.perf_counter()
        acts.append(b["act"].cpu()); args.append(b["argmax"].cpu())
        per_batch.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    a = torch.cat(acts)
    torch.cat(args)
    top = torch.topk(a, K, dim=0)
    end_ms = (time.perf_counter() - t0) * 1e3
    return dict(what=f"host alternative: act_max + argmax read back per batch, concatenate + torch.topk({K}) on the CPU at the end "
                     f"(all classes, no tie order, no feature capture), {torch.get_num_threads()} CPU threads",
                batches=len(epoch), readback_ms_per_batch_median=round(float(np.median(per_batch)), 3),
                readback_ms_per_batch_max=round(max(per_batch), 3), final_cat_topk_ms=round(end_ms, 2), checksum=float(top.values.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--batches", type=int, default=24, help="batches per simulated epoch (24 x 256 ~ CUB's 5994 training images)")
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "proto_bank_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bank.py measures on the GPU; none found")
    dev = torch.device("cuda")
    epoch = make_epoch(a.batches, a.batch, dev)
    rows = [merge_launches(epoch, a.topk, a.reps, True), merge_launches(epoch, a.topk, a.reps, False),
            push_forward_row(a.batch, a.reps, f"PPNet.push_forward, deit_small 2000x384, batch {a.batch} (for scale)"),
            host_alternative(epoch, a.topk)]
    head = [f"# prototype bank cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}",
            f"# produced by: python scripts/bench_bank.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# device times are HIP events around single launches on an otherwise idle stream; host times are perf_counter"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
