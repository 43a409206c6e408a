"""Cost of the part-intervention kernels (csrc/partcheck.hip, csrc/synth.hip), reported not gated: ppf_part_mass on the maps of a
deit_small batch (256 rows of 224 x 224 scores against the partmaps of 256 rendered 256 x 256 frames, K = 4) next to ppf_grad_box_mass on a
[256, 1, 224, 224] tensor IN THE SAME RUN -- the project's existing one-workgroup-per-row fp64 reduction over the same score bytes --, the
ratio of the two next to the byte ratio (the scores plus one gathered byte per pixel over the scores), and the device torch alternative
(gather the codes, one-hot, einsum).  ppf_synth_edit is latency-bound: it stands next to a one-element fill, the cost of a launch.
Event pairs of scripts/bench_common.py around single launches with preallocated outputs.

    python scripts/bench_partcheck.py [--reps 20] [--out profiles/partcheck_cost.txt]
    python -m protopformer_amd.build --variant pmselect PPF_PART_MASS_BINS=0       # beforehand: the other form of the bins
    python -m protopformer_amd.build --variant pmnogather PPF_PART_MASS_KO=1      # knock-outs: the code from the pixel index, no gather
    python -m protopformer_amd.build --variant pmnobins PPF_PART_MASS_KO=2        #             every pixel to bin 0, no bins
    python scripts/bench_partcheck.py --variant-lib "select chain in registers=protopformer_amd/lib/libppf_hip_pmselect.so" ...

A variant library runs in a child process (the library is chosen when the binding loads); a knock-out is a measurement, not a result."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

B, S, FRAME, K = 256, 224, 256, 4


def mass_rows(reps, tag=""):
    import torch
    from bench_common import row, timed
    from protopformer_amd import _lib
    from protopformer_amd import data as D
    from protopformer_amd import ops
    spec = D.PartsWorldSpec(parts=K, height=FRAME, width=FRAME)
    ids = torch.arange(B, dtype=torch.int64, device="cuda")
    _, pm = ops.synth_render(spec, ops.synth_scene(spec, ids), ids, partmap=True)
    torch.manual_seed(0)
    score = torch.randn((B, S, S), device="cuda")
    nb = 3 + K
    pos, neg = torch.empty((B, nb), dtype=torch.float64, device="cuda"), torch.empty((B, nb), dtype=torch.float64, device="cuda")
    cnt, bad = torch.empty((B, nb), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    score_bytes = score.numel() * 4
    t = timed(lambda: _lib.call("ppf_part_mass", score, pm, B, 1, S, FRAME, FRAME, K, pos, neg, cnt, bad), reps)
    rows = [row(f"ppf_part_mass{tag}, R={B} {S}x{S} scores, partmaps {FRAME}x{FRAME}, K={K}", t, score_bytes + score.numel(), workgroups=B)]
    if tag:
        return rows
    box = torch.tensor([[76, 148, 76, 148]], dtype=torch.int32, device="cuda").expand(B, 4).contiguous()
    inside, total = torch.empty(B, dtype=torch.float64, device="cuda"), torch.empty(B, dtype=torch.float64, device="cuda")
    g = score.reshape(B, 1, S, S)
    y = timed(lambda: _lib.call("ppf_grad_box_mass", g, box, B, 1, S, S, inside, total, bad), reps)
    rows.append(row(f"ppf_grad_box_mass (the yardstick), R={B} 1x{S}x{S}, boxes of 72 x 72", y, score_bytes, workgroups=B))
    rows.append(dict(what="ppf_part_mass over the yardstick", time_ratio_at_median=round(t["us_median"] / y["us_median"], 3),
                     byte_ratio=round((score_bytes + score.numel()) / score_bytes, 3)))
    i = torch.arange(S, device="cuda")
    fy, fx = ((2 * i + 1) * FRAME) // (2 * S), ((2 * i + 1) * FRAME) // (2 * S)

    def torch_form():
        codes = pm[:, fy][:, :, fx].reshape(B, S * S).long()
        hot = torch.nn.functional.one_hot(codes, nb).double()
        s = score.reshape(B, S * S).double()
        return torch.einsum("rp,rpc->rc", s.clamp(min=0), hot), torch.einsum("rp,rpc->rc", (-s).clamp(min=0), hot), hot.sum(1)
    rows.append(row("device torch alternative: gather the codes, one_hot, two einsums and a sum (many launches, a [256, 50176, 7] fp64 one-hot)",
                    timed(torch_form, max(3, reps // 4)), score_bytes + score.numel()))
    scene = ops.synth_scene(spec, ids)
    from protopformer_amd.interpret import standard_edits
    edits = torch.tensor(standard_edits(spec), dtype=torch.int32, device="cuda")[None].expand(B, -1, -1).contiguous()
    E = edits.shape[1]
    out, changed = torch.empty((B, E, ops.SYNTH_WORDS), dtype=torch.int32, device="cuda"), torch.empty((B, E), dtype=torch.int32, device="cuda")
    C, Kp, Dn, _, _, gr, _, _ = ops._synth_words(spec)
    rows.append(row(f"ppf_synth_edit, B={B} x E={E} rows", timed(lambda: _lib.call("ppf_synth_edit", out, changed, scene, edits, B, E, C, Kp, Dn, gr), reps),
                    out.numel() * 4 + scene.numel() * 4, workgroups=B * E))
    one = torch.zeros(1, device="cuda")
    rows.append(row("a one-element fill (Tensor.fill_): the cost of a launch", timed(lambda: one.fill_(1.0), reps), 4))
    return rows


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "partcheck_cost.txt"))
    p.add_argument("--variant-lib", action="append", default=[], metavar="NAME=PATH",
                   help="a library built with python -m protopformer_amd.build --variant; its ppf_part_mass row is added under NAME")
    p.add_argument("--rows-only", default="", help="internal: print the ppf_part_mass row as JSON under this tag and exit")
    args = p.parse_args()
    if args.rows_only:
        print("ROWS " + json.dumps(mass_rows(args.reps, args.rows_only)))
        return
    import torch
    rows = mass_rows(args.reps)
    for item in args.variant_lib:
        name, path = item.rsplit("=", 1)                                       # the name may hold a '=' of its own
        env = dict(os.environ, PPF_LIB_PATH=os.path.abspath(path))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-only", f" [{name}]", "--reps", str(args.reps)], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"the run with {path} failed:\n{r.stderr[-2000:]}")
        rows += json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    name = torch.cuda.get_device_name(0)
    with open(args.out, "w") as f:
        f.write(f"# scripts/bench_partcheck.py --reps {args.reps} on {name}\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
