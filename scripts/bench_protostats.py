"""Cost of the prototype statistics (protostats.PrototypeStats) on one MI355X -- profiles/proto_stats_cost.txt.

    python scripts/bench_protostats.py [--batch 256 --bins 64 --reps 50] [--out profiles/proto_stats_cost.txt]

At the deit_small shape (2000 local and 2000 global prototypes, 200 classes, 81 reserved tokens on a 196-cell grid, batch 256) it measures
  * ppf_proto_stats_update: the local call (histogram + co-location launches) and the global call (histogram launch only), HIP events
    around every single call (queued behind a running matrix product, so the host's enqueue time is not in the figure), `reps` calls after
    5 warm-up calls, on two kinds of activations: log((d + 1) / (d + eps)) of uniform distances (what a model produces: a few bins per
    prototype fill, so few counters are flushed) and uniform over the whole range (every bin fills: the most flushes a batch can cause);
  * achieved GB/s of the median call against the bytes it must read (act_max, the labels, the own-class argmax entries and idx rows);
  * (a) PPNet.push_forward of one such batch, for scale;
  * (b) the torch alternative on the device, timed the same way: torch.bucketize + scatter_add_ for the histograms and a [B, ppc, ppc]
    compare + index_add_ for the co-location (no NaN count, no check of the labels);
  * (c) the host alternative: act_max / argmax / idx read back, then np.add.at into the same tables (perf_counter).
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

P, KTOK, GRID, CLASSES, EPS = 2000, 81, 196, 200, 1e-4
PPC = P // CLASSES
LO, HI = 0.0, float(np.float32(np.log(1.0 / EPS)))


def make_batch(B, dev, kind):
    g = torch.Generator(device=dev).manual_seed(1028)
    if kind == "model-like":
        d = torch.rand((B, P), device=dev, generator=g) * 4.0
        act = torch.log((d + 1.0) / (d + EPS))
    else:
        act = torch.rand((B, P), device=dev, generator=g) * HI
    return dict(kind=kind, act=act.contiguous(), argmax=torch.randint(0, KTOK, (B, P), device=dev, generator=g).to(torch.int32),
                idx=torch.rand((B, GRID), device=dev, generator=g).argsort(1)[:, :KTOK].sort(1).values.to(torch.int32).contiguous(),
                labels=torch.randint(0, CLASSES, (B,), device=dev, generator=g))


def new_tables(NB, dev):
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    return dict(hist=z(P, 2, NB), nan_count=z(P, 2), coloc=z(P, PPC), images=z(CLASSES), bad=z(1))


def kernel_rows(b, NB, reps):
    from protopformer_amd import _lib
    from protopformer_amd.protostats import inv_width_of
    B, dev = b["act"].shape[0], b["act"].device
    w = float(inv_width_of(NB, LO, HI))
    rows = []
    for local in (True, False):
        t = new_tables(NB, dev)
        args = (b["act"], b["argmax"] if local else None, b["idx"] if local else None, KTOK if local else 0, b["labels"], PPC, B, P, NB, LO, w, t["hist"],
                t["nan_count"], t["coloc"] if local else None, t["images"], t["bad"])
        r = timed(lambda: _lib.call("ppf_proto_stats_update", *args), reps, warm=5)
        read = B * P * 4 + B * 8 + (B * PPC * 4 + B * KTOK * 4 if local else 0)
        calls = reps + 5
        filled = int((t["hist"] != 0).sum())
        assert int(t["hist"].sum()) == calls * B * P and int(t["images"].sum()) == calls * B
        rows.append(dict(what=f"ppf_proto_stats_update, {'local (histogram + co-location launches)' if local else 'global (histogram launch)'}, "
                              f"{b['kind']} activations, B={B} P={P} ppc={PPC} NB={NB}" + (f" T={KTOK}" if local else ""), **r, bytes_read=read,
                         gb_per_s_at_median=round(read / r["us_median"] / 1e3, 1), table_bytes=P * 2 * NB * 4, counters_nonzero=filled,
                         counters_total=P * 2 * NB))
    return rows


def torch_alternative(b, NB, reps):
    B, dev = b["act"].shape[0], b["act"].device
    t = new_tables(NB, dev)
    edges = (LO + torch.arange(1, NB, device=dev, dtype=torch.float32) * ((HI - LO) / NB)).contiguous()
    proto, cls = torch.arange(P, device=dev)[None, :], (torch.arange(P, device=dev) // PPC)[None, :]
    ones = torch.ones(B * P, dtype=torch.int32, device=dev)
    rows_b = torch.arange(B, device=dev)

    def hist():
        bins = torch.bucketize(b["act"], edges, right=True)
        slot = (cls != b["labels"][:, None]).long()
        t["hist"].view(-1).scatter_add_(0, ((proto * 2 + slot) * NB + bins).view(-1), ones)

    def coloc():
        am = b["argmax"].view(B, CLASSES, PPC)[rows_b, b["labels"]]
        cell = torch.gather(b["idx"], 1, am.long())
        t["coloc"].view(CLASSES, PPC, PPC).index_add_(0, b["labels"], (cell[:, :, None] == cell[:, None, :]).to(torch.int32))

    h, c = timed(hist, reps, warm=5), timed(coloc, reps, warm=5)
    both = timed(lambda: (hist(), coloc()), reps, warm=5)
    return dict(what=f"torch alternative on the device, {b['kind']} activations: bucketize + scatter_add_ for one branch's histograms, [B, ppc, ppc] compare + "
                     "index_add_ for the co-location (no NaN count, no label check), same event pairs", histogram=h, colocation=c, local_branch_both=both)


def host_alternative(b, NB, reps):
    from protopformer_amd.protostats import bin_index, inv_width_of
    B = b["act"].shape[0]
    w = inv_width_of(NB, LO, HI)
    hist, coloc = np.zeros((P, 2, NB), dtype=np.int32), np.zeros((P, PPC), dtype=np.int32)
    read, add = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        act, am, idx, lab = b["act"].cpu().numpy(), b["argmax"].cpu().numpy(), b["idx"].cpu().numpy(), b["labels"].cpu().numpy()
        read.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        bins, _ = bin_index(act, NB, LO, w)
        slot = ((np.arange(P) // PPC)[None, :] != lab[:, None]).astype(np.int64)
        np.add.at(hist, (np.broadcast_to(np.arange(P)[None, :], (B, P)), slot, bins), 1)
        own = am.reshape(B, CLASSES, PPC)[np.arange(B), lab]
        cell = np.take_along_axis(idx, own.astype(np.int64), axis=1)
        np.add.at(coloc.reshape(CLASSES, PPC, PPC), lab, (cell[:, :, None] == cell[:, None, :]).astype(np.int32))
        add.append((time.perf_counter() - t0) * 1e3)
    return dict(what=f"host alternative, {b['kind']} activations, local branch: act_max + argmax + idx + labels read back, np.add.at into the tables",
                readback_ms_median=round(float(np.median(read)), 3), readback_bytes=B * P * 8 + B * KTOK * 4 + B * 8,
                numpy_ms_median=round(float(np.median(add)), 3), runs=reps, checksum=int(hist.sum()) + int(coloc.sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "proto_stats_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_protostats.py measures on the GPU; none found")
    dev = torch.device("cuda")
    rows = []
    for kind in ("model-like", "uniform"):
        b = make_batch(a.batch, dev, kind)
        rows += kernel_rows(b, a.bins, a.reps)
        rows.append(torch_alternative(b, a.bins, a.reps))
        rows.append(host_alternative(b, a.bins, min(a.reps, 10)))
        del b
    torch.cuda.empty_cache()
    rows.append(push_forward_row(a.batch, 5, f"PPNet.push_forward, deit_small 2000x384, batch {a.batch} (for scale)"))
    head = [f"# prototype statistics cost: {torch.cuda.get_device_name(0)}, one GPU, one process; torch {torch.__version__}, numpy {np.__version__}",
            f"# produced by: python scripts/bench_protostats.py {' '.join(sys.argv[1:])}".rstrip() + f"   ({datetime.date.today().isoformat()})",
            "# device times are HIP events around single calls queued behind a running kernel (no host enqueue time inside); host times are perf_counter"]
    text = "\n".join(head + [json.dumps(r) for r in rows]) + "\n"
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
