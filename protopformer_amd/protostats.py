"""Prototype statistics over a data set: which prototypes does the model need?  (ProtoPNet's pruning pass and the activation
percentiles of its local analysis; the reference has neither.)

Per prototype the histogram of its pooled activation over a whole split, split into own-class and other-class images, and on the
local branch how often two prototypes of a class fire at the same grid cell.  Per batch one eval forward and one
`ppf_proto_stats_update` call per branch fold what `ppf_proto_fwd` left on the device into small int32 tables that stay there and are
read once at the end; nothing of size [B, P] is read back.  Everything derived from the tables (AUROC of own against other images,
percentiles, overlaps, the keep decision) is integer / fp64 numpy on the host, so it is the same wherever the tables are.

    python -m protopformer_amd.protostats --resume CKPT --data_set CUB2011U --data_path ... --output_dir OUT [--split train] [--bins 64]
                                          [--range LO HI] [--max_images N]
                                          [--prune [--min_auroc 0.5] [--max_overlap 0.9] [--min_keep 1] [--save-pruned PATH]]
                                          + the model flags of train.py

writes OUT/prototype_stats.npz (the tables of PrototypeStats.result, the range and the bin count) and OUT/prototype_stats.json
(stats_report: per prototype branch, class, counts, AUROC, mean and median activation, the overlaps above 0.5 with their partners; with
--prune also the keep decision with the reason for every dropped prototype, acc@1 on the test split before and after, and the path of
the pruned checkpoint)."""
import json
import math
import os

import numpy as np
import torch

BRANCHES = ("local", "global")
WEIGHT_OF = {"local": "last_layer.weight", "global": "last_layer_global.weight"}
TABLES = ("hist", "nan_count", "coloc", "images", "bad")
MAX_BATCH = 1024                       # ppf_proto_stats_update accepts 1 <= B <= 1024: larger batches go in slices
MIN_BINS, MAX_BINS = 8, 128


# ------------------------------------------------------------------------------------------------ the bin rule and the referee
def inv_width_of(bins, lo, hi):
    """fl(bins / fl(hi - lo)) in fp32: the scale ppf_proto_stats_update is given (rounded here, once)."""
    lo, hi = np.float32(lo), np.float32(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
        raise ValueError(f"prototype statistics: the range [{lo}, {hi}] must be finite and not empty")
    with np.errstate(all="ignore"):
        w = np.float32(np.float32(bins) / np.float32(hi - lo))
    if not (np.isfinite(w) and w > 0):
        raise ValueError(f"prototype statistics: {bins} bins over [{lo}, {hi}] give the scale {w}")
    return w


def bin_index(a, bins, lo, inv_width):
    """(bin, is_nan) of fp32 activations under the kernel's rule: t = fl(fl(a - lo) * inv_width) in float32, two roundings; bin 0 when
    t < 0 (-inf included), bins - 1 when t >= bins (+inf included), else int(t).  NaN has no bin (is_nan; its bin entry is 0)."""
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(all="ignore"):
        t = (a - np.float32(lo)) * np.float32(inv_width)                    # float32 throughout: numpy rounds after each operation
    nan = np.isnan(a)
    return np.clip(np.where(nan, np.float32(0), t), 0, int(bins) - 1).astype(np.int64), nan


def _np(t, dtype):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


def stats_from_outputs(act_max, argmax, idx, labels, ppc, bins, lo, hi, device=False):
    """The tables of ONE branch from collected outputs: act_max [B, P] pooled activations, labels [B]; the local branch adds argmax
    [B, P] and idx [B, T] (both None: the global branch, coloc is None then).  Returns dict(hist [P, 2, bins], nan_count [P, 2], coloc
    [P, ppc] or None, images [P // ppc], bad [1]) of int32; the contract is ppf_proto_stats_update's (include/ppf_hip.h).
    device=False: the numpy referee of the kernel (host arrays in and out).  device=True: the kernel itself on CUDA tensors, batches
    above 1024 in slices (device tensors out)."""
    ppc, bins = int(ppc), int(bins)
    w = inv_width_of(bins, lo, hi)
    if device:
        from . import ops
        (B, P), dev = act_max.shape, act_max.device
        out = dict(hist=ops.zeros((P, 2, bins), torch.int32, dev), nan_count=ops.zeros((P, 2), torch.int32, dev),
                   coloc=ops.zeros((P, ppc), torch.int32, dev) if argmax is not None else None,
                   images=ops.zeros((max(P // max(ppc, 1), 0),), torch.int32, dev), bad=ops.zeros((1,), torch.int32, dev))
        labels = torch.as_tensor(labels).to(device=dev, dtype=torch.int64).contiguous()
        for b in range(0, B, MAX_BATCH):
            e = min(B, b + MAX_BATCH)
            ops.proto_stats_update(act_max[b:e].contiguous(), None if argmax is None else argmax[b:e].contiguous(),
                                   None if idx is None else idx[b:e].contiguous(), labels[b:e], ppc, float(np.float32(lo)), float(w), out["hist"],
                                   out["nan_count"], out["coloc"], out["images"], out["bad"])
        return out
    act, argmax, idx, labels = _np(act_max, np.float32), _np(argmax, np.int64), _np(idx, np.int64), _np(labels, np.int64)
    B, P = act.shape
    if not (1 <= ppc <= 64 and P >= 1 and P % ppc == 0 and MIN_BINS <= bins <= MAX_BINS) or (argmax is None) != (idx is None):
        raise ValueError(f"stats_from_outputs: P={P} ppc={ppc} bins={bins} outside ppf_proto_stats_update's limits, or argmax without idx")
    C = P // ppc
    ok = (labels >= 0) & (labels < C)
    images = np.bincount(labels[ok], minlength=C).astype(np.int32)
    a, lab = act[ok], labels[ok]
    slot = ((np.arange(P) // ppc)[None, :] != lab[:, None]).astype(np.int64)             # 0: own class, 1: another class
    cell2 = np.arange(P)[None, :] * 2 + slot
    b, nan = bin_index(a, bins, lo, w)
    hist = np.bincount((cell2 * bins + b)[~nan], minlength=P * 2 * bins).reshape(P, 2, bins).astype(np.int32)
    nan_count = np.bincount(cell2[nan], minlength=P * 2).reshape(P, 2).astype(np.int32)
    coloc = None
    if argmax is not None:
        T = idx.shape[1]
        coloc = np.zeros((P, ppc), dtype=np.int32)
        for s in np.nonzero(ok)[0]:
            c = int(labels[s])
            am = argmax[s, c * ppc:(c + 1) * ppc]
            valid = (am >= 0) & (am < T)
            cell = idx[s, np.clip(am, 0, T - 1)]
            coloc[c * ppc:(c + 1) * ppc] += valid[:, None] & valid[None, :] & (cell[:, None] == cell[None, :])
    return dict(hist=hist, nan_count=nan_count, coloc=coloc, images=images, bad=np.array([int((~ok).sum())], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ derived quantities (host, exact)
def auroc_counts(hist):
    """(numerator, denominator) int64 [P] of the AUROC as an exact ratio: sum_k own[k] * (2 * other_below[k] + other[k]) over
    2 * n_own * n_other (a tie inside a bin counts half)."""
    h = np.asarray(hist).astype(np.int64)
    own, other = h[:, 0], h[:, 1]
    below = np.cumsum(other, axis=1) - other
    return (own * (2 * below + other)).sum(axis=1), 2 * own.sum(axis=1) * other.sum(axis=1)


def auroc(hist):
    """Per prototype the probability that a random own-class image activates it more than a random other-class image, ties within a
    bin counting half; NaN when the prototype saw no own-class or no other-class image.  hist [P, 2, bins]; fp64 [P]."""
    num, den = auroc_counts(hist)
    with np.errstate(all="ignore"):
        return np.where(den > 0, num.astype(np.float64) / np.where(den > 0, den, 1), np.nan)


def _counts(hist, p, which):
    h = np.asarray(hist)[int(p)].astype(np.int64)
    if which not in ("all", "own", "other"):
        raise ValueError(f"prototype statistics: which must be 'all', 'own' or 'other', got {which!r}")
    return h[0] + h[1] if which == "all" else h[0 if which == "own" else 1]


def percentile(tables, p, a, which="all"):
    """Where does the activation `a` of prototype p stand among the recorded images?  The share (0..1) of them strictly below a's
    bin plus half of that bin, among all / the own-class / the other-class images.  tables: one branch of PrototypeStats.result() (its
    'hist', 'lo' and 'hi').  NaN for a NaN activation or when nothing was recorded."""
    hist = np.asarray(tables["hist"])
    cnt = _counts(hist, p, which)
    b, nan = bin_index(np.float32(a), hist.shape[2], tables["lo"], inv_width_of(hist.shape[2], tables["lo"], tables["hi"]))
    n = int(cnt.sum())
    if bool(nan) or n == 0:
        return float("nan")
    return float((2 * int(cnt[:int(b)].sum()) + int(cnt[int(b)])) / (2.0 * n))


def overlap(coloc, images=None):
    """[P, ppc] fp64: coloc[p][q] / coloc[p][p % ppc], the share of p's own-class images (with a valid cell) in which prototype q of the
    same class fires at p's cell; NaN where that diagonal is 0.  images [C] (optional) is only checked against coloc's class count."""
    coloc = np.asarray(coloc).astype(np.int64)
    P, ppc = coloc.shape
    if images is not None and np.asarray(images).shape != (P // ppc,):
        raise ValueError(f"overlap: images {np.asarray(images).shape} does not fit coloc {coloc.shape}")
    diag = coloc[np.arange(P), np.arange(P) % ppc]
    with np.errstate(all="ignore"):
        return np.where(diag[:, None] > 0, coloc.astype(np.float64) / np.where(diag > 0, diag, 1)[:, None], np.nan)


def bin_centres(bins, lo, hi):
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    return lo + (np.arange(int(bins), dtype=np.float64) + 0.5) * ((hi - lo) / int(bins))


def mean_median(hist, lo, hi):
    """(mean, median) fp64 [P, 2] of the bin centres per prototype and slot (own, other); the median is the centre of the lowest bin at
    which the cumulative count reaches half; NaN where nothing was recorded."""
    h = np.asarray(hist).astype(np.int64)
    centres, n = bin_centres(h.shape[2], lo, hi), h.sum(axis=2)
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, (h * centres).sum(axis=2) / np.where(n > 0, n, 1), np.nan)
    k = (2 * np.cumsum(h, axis=2) >= n[:, :, None]).argmax(axis=2)
    return mean, np.where(n > 0, centres[k], np.nan)


def keep_decisions(stats, min_auroc=0.5, max_overlap=0.9, min_keep=1):
    """({branch: bool [P]}, {branch: {dropped prototype: reason}}) -- keep_mask with its reasons."""
    keep, why = {}, {}
    for br in BRANCHES:
        t = stats[br]
        au = auroc(t["hist"])
        P = au.shape[0]
        ppc = P // np.asarray(t["images"]).shape[0]
        ov = overlap(t["coloc"]) if br == "local" and t.get("coloc") is not None else None
        keep[br], why[br] = np.zeros(P, dtype=bool), {}
        for c in range(P // ppc):
            ids = np.arange(c * ppc, (c + 1) * ppc)
            nan = np.isnan(au[ids])
            order = ids[np.lexsort((ids, np.where(nan, 0.0, -au[ids]), nan))]          # known AUROCs first, larger first, equal by smaller id
            kept = []
            for rank, p in enumerate(int(v) for v in order):
                reason = None
                if np.isnan(au[p]):
                    reason = "no own-class or no other-class image: AUROC undefined"
                elif au[p] < min_auroc:
                    reason = f"AUROC {au[p]:.6g} below {min_auroc:g}"
                elif ov is not None:
                    for q in kept:
                        o = max((v for v in (ov[p, q % ppc], ov[q, p % ppc]) if not np.isnan(v)), default=-1.0)
                        if o >= max_overlap:
                            reason = f"overlap {o:.6g} with kept prototype {q} reaches {max_overlap:g}"
                            break
                if reason is None or rank < min_keep:
                    kept.append(p)
                    keep[br][p] = True
                else:
                    why[br][p] = reason
    return keep, why


def keep_mask(stats, min_auroc=0.5, max_overlap=0.9, min_keep=1):
    """{'local' | 'global': bool [P]}: the prototypes worth keeping, decided per class and deterministically from the tables of
    PrototypeStats.result().  1. a prototype whose AUROC is NaN or below min_auroc is dropped; 2. the rest are visited by descending
    AUROC, equal values by smaller id; 3. one is dropped when its overlap with an already kept prototype reaches max_overlap in either
    direction (local branch only: the global branch has no cells); 4. the best min_keep of a class are always kept."""
    return keep_decisions(stats, min_auroc, max_overlap, min_keep)[0]


@torch.no_grad()
def prune_(ppnet, keep):
    """Zero the last-layer columns of the dropped prototypes (keep: {'local' | 'global': bool [P]}; a missing branch is left alone).
    Shapes stay, so the checkpoint loads into an unmodified model and every other tool keeps working; goes through load_state_dict, the
    path PrototypeBank.project_ takes.  Returns {branch: number of prototypes dropped}."""
    new, dropped = {}, {}
    for br in BRANCHES:
        if keep.get(br) is None:
            continue
        w = ppnet.state_dict()[WEIGHT_OF[br]].detach()
        k = torch.as_tensor(np.asarray(keep[br], dtype=bool), device=w.device)
        if k.shape != (w.shape[1],):
            raise ValueError(f"prune_: keep['{br}'] has {tuple(k.shape)} entries, {WEIGHT_OF[br]} has {w.shape[1]} columns")
        new[WEIGHT_OF[br]] = torch.where(k[None, :], w, torch.zeros_like(w))
        dropped[br] = int((~k).sum())
    ppnet.load_state_dict(new, strict=False)             # in-place copies into the flat store's views + invalidation of its shadows
    return dropped


# ------------------------------------------------------------------------------------------------ the accumulator
class PrototypeStats:
    """The tables of both branches in device memory, fed by update() / merge() and read by result() in one host read.  Integer counts:
    the result does not depend on how the images were batched or ordered.
    range=None: [0, fl(log(1 / epsilon))] for the 'log' activation, which contains every value of that activation.  A 'linear' model
    needs an explicit (lo, hi): a range taken from the data would make the result depend on the order of the batches.
    The model may live on the CPU to hold tables made elsewhere (result() works there, update() needs the GPU)."""

    def __init__(self, ppnet, bins=64, range=None):
        if not MIN_BINS <= int(bins) <= MAX_BINS:
            raise ValueError(f"PrototypeStats: bins={bins} outside [{MIN_BINS}, {MAX_BINS}]")
        if range is None:
            if ppnet.prototype_activation_function != "log":
                raise ValueError(f"PrototypeStats: the '{ppnet.prototype_activation_function}' activation has no natural range: pass range=(lo, hi)")
            range = (0.0, math.log(1.0 / ppnet.epsilon))
        self.ppnet, self.bins = ppnet, int(bins)
        self.lo, self.hi = np.float32(range[0]), np.float32(range[1])
        self.inv_width = inv_width_of(self.bins, self.lo, self.hi)
        self.num = {"local": ppnet.num_prototypes, "global": ppnet.num_prototypes_global}
        self.ppc = {"local": ppnet.num_prototypes_per_class, "global": ppnet.global_proto_per_class}
        self.shapes = {}
        for br in BRANCHES:
            P, ppc = self.num[br], self.ppc[br]
            self.shapes[br] = dict(hist=(P, 2, self.bins), nan_count=(P, 2), coloc=(P, ppc) if br == "local" else (0,), images=(P // ppc,), bad=(1,))
        sizes = [int(np.prod(self.shapes[br][k])) for br in BRANCHES for k in TABLES]
        self.buf = torch.zeros(sum(sizes), dtype=torch.int32, device=ppnet.prototype_vectors.device)          # one buffer: one read-back
        parts = iter(torch.split(self.buf, sizes))
        self.state = {br: {k: next(parts).view(self.shapes[br][k]) for k in TABLES} for br in BRANCHES}

    @torch.no_grad()
    def update(self, x, labels):
        """One batch through the model's eval branch (PPNet.eval_branches), then both branches into the tables."""
        r = self.ppnet.eval_branches(x)
        self.merge("local", r.act_max_local, r.argmax, r.idx, labels)
        self.merge("global", r.act_max_global, None, None, labels)

    def merge(self, branch, act_max, argmax, idx, labels):
        """Low-level: add one batch's pooled activations of `branch`.  act_max [B, P] fp32, argmax [B, P] int32 and idx [B, T] int32
        (both None for 'global'), labels int64 [B]."""
        from . import ops
        if branch not in BRANCHES:
            raise ValueError(f"PrototypeStats.merge: branch must be one of {BRANCHES}")
        if (branch == "global") != (argmax is None) or (argmax is None) != (idx is None):
            raise ValueError("PrototypeStats.merge: the local branch comes with argmax and idx, the global branch without")
        s, B = self.state[branch], act_max.shape[0]
        labels = torch.as_tensor(labels).to(device=act_max.device, dtype=torch.int64).contiguous()
        for b in range(0, B, MAX_BATCH):
            e = min(B, b + MAX_BATCH)
            ops.proto_stats_update(act_max[b:e].contiguous(), None if argmax is None else argmax[b:e].contiguous(),
                                   None if idx is None else idx[b:e].contiguous(), labels[b:e], self.ppc[branch], float(self.lo), float(self.inv_width),
                                   s["hist"], s["nan_count"], s["coloc"] if branch == "local" else None, s["images"], s["bad"])

    def result(self):
        """One host read.  {'local' | 'global': dict(hist [P, 2, bins], nan_count [P, 2], coloc [P, ppc] (None on the global branch),
        images [C], bad [1], lo, hi (fp32 scalars))} of int32 numpy arrays."""
        host = self.buf.cpu().numpy()
        out, o = {}, 0
        for br in BRANCHES:
            out[br] = {}
            for k in TABLES:
                n = int(np.prod(self.shapes[br][k]))
                out[br][k] = host[o:o + n].reshape(self.shapes[br][k]).copy()
                o += n
            if br == "global":
                out[br]["coloc"] = None
            out[br].update(lo=self.lo, hi=self.hi)
        return out

    def state_dict(self):
        return {"bins": self.bins, "lo": float(self.lo), "hi": float(self.hi), "tables": self.buf.detach().cpu()}

    def load_state_dict(self, sd):
        if int(sd["bins"]) != self.bins or np.float32(sd["lo"]) != self.lo or np.float32(sd["hi"]) != self.hi:
            raise ValueError(f"PrototypeStats.load_state_dict: saved with bins={sd['bins']} range=[{sd['lo']}, {sd['hi']}], this object has "
                             f"bins={self.bins} range=[{self.lo}, {self.hi}]")
        t = sd["tables"]
        if t.shape != self.buf.shape or t.dtype != self.buf.dtype:
            raise ValueError(f"PrototypeStats.load_state_dict: tables are {tuple(t.shape)} {t.dtype}, expected {tuple(self.buf.shape)} {self.buf.dtype}")
        self.buf.copy_(t)


def prototype_stats(ppnet, loader, bins=64, range=None, max_images=0):
    """The filled PrototypeStats of the whole of `loader` (batches (x, labels, ...); at most max_images images when > 0)."""
    from .tooling import take_images
    stats = PrototypeStats(ppnet, bins=bins, range=range)
    for x, y, *_ in take_images(loader, max_images):
        stats.update(x if x.is_cuda else x.cuda(), y)
    return stats


# ------------------------------------------------------------------------------------------------ files and the report
def save_stats(path, result):
    """prototype_stats.npz: <branch>_<table> of PrototypeStats.result(), lo, hi and bins."""
    arrays = {f"{br}_{k}": result[br][k] for br in BRANCHES for k in TABLES if result[br][k] is not None}
    np.savez(path, lo=np.float32(result["local"]["lo"]), hi=np.float32(result["local"]["hi"]), bins=np.int32(result["local"]["hist"].shape[2]),
             **arrays)


def load_stats(path):
    """The result() dict back from a prototype_stats.npz."""
    z = np.load(path)
    out = {}
    for br in BRANCHES:
        out[br] = {k: (z[f"{br}_{k}"] if f"{br}_{k}" in z.files else None) for k in TABLES}
        out[br].update(lo=np.float32(z["lo"]), hi=np.float32(z["hi"]))
    return out


def _num(v):
    return None if v is None or np.isnan(v) else float(v)


def stats_report(result, overlap_above=0.5):
    """The JSON document of the tool: {'bins', 'range', 'images': {branch: n}, 'bad_labels', 'prototypes': [{'branch', 'prototype',
    'class', 'own_images', 'other_images', 'nan_own', 'nan_other', 'auroc', 'mean_own', 'mean_other', 'median_own', 'median_other',
    'overlaps': [{'with', 'share'}] (local branch: the partners whose cell coincides in more than overlap_above of this prototype's
    own-class images)}]}; undefined values are null."""
    protos = []
    for br in BRANCHES:
        t = result[br]
        hist = np.asarray(t["hist"])
        P, ppc = hist.shape[0], hist.shape[0] // t["images"].shape[0]
        au, (mean, med) = auroc(hist), mean_median(hist, t["lo"], t["hi"])
        ov = overlap(t["coloc"]) if t["coloc"] is not None else None
        n = hist.sum(axis=2)
        for p in range(P):
            rec = {"branch": br, "prototype": p, "class": p // ppc, "own_images": int(n[p, 0]), "other_images": int(n[p, 1]),
                   "nan_own": int(t["nan_count"][p, 0]), "nan_other": int(t["nan_count"][p, 1]), "auroc": _num(au[p]), "mean_own": _num(mean[p, 0]),
                   "mean_other": _num(mean[p, 1]), "median_own": _num(med[p, 0]), "median_other": _num(med[p, 1])}
            if ov is not None:
                first = p - p % ppc
                rec["overlaps"] = [{"with": first + q, "share": float(ov[p, q])} for q in range(ppc)
                                   if first + q != p and not np.isnan(ov[p, q]) and ov[p, q] > overlap_above]
            protos.append(rec)
    loc = result["local"]
    return dict(bins=int(loc["hist"].shape[2]), range=[float(loc["lo"]), float(loc["hi"])], images={br: int(result[br]["images"].sum()) for br in BRANCHES},
                bad_labels=int(loc["bad"][0]), prototypes=protos)


# ------------------------------------------------------------------------------------------------ the tool
def get_args_parser():
    from .tooling import tool_parser
    p = tool_parser("ProtoPFormer prototype statistics: selectivity, overlap and pruning of the prototypes", "train", "measured")
    a = p.add_argument
    a("--bins", type=int, default=64, help=f"histogram bins per prototype ({MIN_BINS}..{MAX_BINS})")
    a("--range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="activation range of the histograms (default: [0, log(1 / epsilon)] "
      "of the 'log' activation; required for 'linear')")
    a("--prune", action="store_true", default=False, help="decide which prototypes to keep, zero the others' last-layer columns and save the model")
    a("--min_auroc", type=float, default=0.5, help="--prune: drop a prototype whose own-vs-other AUROC is below this")
    a("--max_overlap", type=float, default=0.9, help="--prune: drop a local prototype that shares its cell with a kept one in this share of images")
    a("--min_keep", type=int, default=1, help="--prune: prototypes always kept per class and branch")
    a("--save-pruned", type=str, default="", metavar="PATH", help="where --prune writes (default <output_dir>/checkpoints/pruned.pth)")
    return p


def main(args, model=None):
    from . import engine as E
    from .tooling import eval_loader, load_for_eval, model_from_args
    from .train import set_seed
    set_seed(args.seed)
    device = torch.device(args.device)
    ds, nb_classes, loader = eval_loader(args, device, with_ids=False)
    model = load_for_eval(model_from_args(args, nb_classes) if model is None else model, args, device)
    stats = prototype_stats(model, loader, bins=args.bins, range=None if args.range is None else tuple(args.range), max_images=args.max_images)
    result = stats.result()
    if int(result["local"]["bad"][0]) != 0:
        raise ValueError(f"protostats: {int(result['local']['bad'][0])} labels lie outside [0, {nb_classes})")
    os.makedirs(args.output_dir, exist_ok=True)
    npz, js = os.path.join(args.output_dir, "prototype_stats.npz"), os.path.join(args.output_dir, "prototype_stats.json")
    save_stats(npz, result)
    doc = stats_report(result)
    if args.prune:
        keep, why = keep_decisions(result, args.min_auroc, args.max_overlap, args.min_keep)
        split = args.split
        args.split = "test"
        try:
            _, _, test_loader = eval_loader(args, device, with_ids=False)
        finally:
            args.split = split
        before = E.evaluate_epoch(test_loader, model, device)["acc1"]
        dropped = prune_(model, keep)
        after = E.evaluate_epoch(test_loader, model, device)["acc1"]
        path = args.save_pruned or os.path.join(args.output_dir, "checkpoints", "pruned.pth")
        E.save_checkpoint(path, model, E.FlatAdamW(model), None, 0, args=args)
        doc["prune"] = dict(min_auroc=args.min_auroc, max_overlap=args.max_overlap, min_keep=args.min_keep, dropped=dropped,
                            keep={br: [bool(v) for v in keep[br]] for br in BRANCHES},
                            reasons={br: {str(p): r for p, r in sorted(why[br].items())} for br in BRANCHES},
                            acc1_before=before, acc1_after=after, checkpoint=path)
        print(f"pruned {dropped['local']} local and {dropped['global']} global prototypes, test acc@1 {before:.2f} -> {after:.2f}: {path}", flush=True)
    with open(js, "w") as f:
        json.dump(doc, f, indent=1)
    print(f"prototype statistics over {doc['images']['local']} {args.split} images: {npz} {js}", flush=True)
    return stats


if __name__ == "__main__":
    cli_args = get_args_parser().parse_args()
    main(cli_args)
