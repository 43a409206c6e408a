"""CPU-side checks of the training driver (protopformer_amd/train.py): its argument parser against the reference's (a committed table),
the bookkeeping of the epoch loop with the train / eval callables replaced by fakes, --resume's start epoch, and EvalMeter.reduce_
over two gloo ranks."""
import json
import logging
import os
import socket
import subprocess
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_ARGS = os.path.join(HERE, "golden", "train_args.json")
OURS = {"no_pretrained", "step"}


def _table(parser):
    types_of = {}
    for act in parser._actions:
        types_of[act.dest] = getattr(act.type, "__name__", None) if act.type is not None else None
    defaults = vars(parser.parse_args([]))
    return {dest: {"default": defaults[dest], "type": types_of[dest]} for dest in types_of}


def test_parser_matches_the_reference_table():
    """Every dest of main.py:get_args_parser (tests/golden/train_args.json, written by make_golden_args.py from the reference's parser) is
    present with an equal default and an equal type name; --no-pretrained and --step are the only additional dests."""
    from protopformer_amd.train import get_args_parser
    gold = json.load(open(GOLDEN_ARGS))
    mine = _table(get_args_parser())
    assert len(gold) >= 80
    assert set(mine) - set(gold) == OURS
    assert set(gold) - set(mine) == set()
    for dest, ref in gold.items():
        assert mine[dest]["type"] == ref["type"], dest
        assert mine[dest]["default"] == ref["default"] and type(mine[dest]["default"]) is type(ref["default"]), (dest, mine[dest], ref)


def test_parser_takes_the_reference_scripts_argument_list():
    """The argument list of scripts/train_cub.sh (deit_small, 4 GPUs' worth of flags), spelled as the script spells it."""
    from protopformer_amd.train import get_args_parser
    argv = ("--base_architecture=deit_small_patch16_224 --data_set=CUB2011U --data_path=datasets --input_size=224 --output_dir=out/x "
            "--model=deit_small_patch16_224 --batch_size=128 --seed=1028 --opt=adamw --sched=cosine --warmup-epochs=5 --warmup-lr=1e-4 "
            "--decay-epochs=10 --decay-rate=0.1 --weight_decay=0.05 --epochs=200 --finetune=protopformer --features_lr=1e-4 "
            "--add_on_layers_lr=3e-3 --prototype_vectors_lr=3e-3 --prototype_shape 2000 192 1 1 --reserve_layers 11 --reserve_token_nums 81 "
            "--use_global=True --use_ppc_loss=True --ppc_cov_thresh=1. --ppc_mean_thresh=2. --global_coe=0.5 --global_proto_per_class=10 "
            "--ppc_cov_coe=0.1 --ppc_mean_coe=0.5").split()
    a = get_args_parser().parse_args(argv)
    assert a.use_global is True and a.use_ppc_loss is True and a.prototype_shape == [2000, 192, 1, 1] and a.reserve_layers == [11]
    assert a.warmup_lr == 1e-4 and a.decay_epochs == 10.0 and a.model_ema is True and a.step is None and a.no_pretrained is False
    with pytest.raises(SystemExit):
        get_args_parser().parse_args(["--step", "graph"])


@pytest.mark.reference
def test_reference_table_is_current(tmp_path):
    """Regenerate the table from the reference's parser (a child process: the generator installs stand-in modules) and compare."""
    out = tmp_path / "train_args.json"
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_golden_args.py"), str(out)], check=True, timeout=300)
    assert json.load(open(out)) == json.load(open(GOLDEN_ARGS))
    assert open(out).read() == open(GOLDEN_ARGS).read()


# ------------------------------------------------------------------------------------------------ the epoch loop's bookkeeping
def _run(tmp_path, acc1s, save_ep_freq, start_epoch=0):
    from protopformer_amd.train import SCALARS, get_args_parser, run_epochs
    args = get_args_parser().parse_args(["--output_dir", str(tmp_path), "--epochs", str(len(acc1s)), "--save_ep_freq", str(save_ep_freq)])
    calls, saved = [], []

    def train_epoch(epoch):
        calls.append(("train", epoch))
        return {"loss": 2.0 - 0.1 * epoch, "lr": 1e-4}

    def eval_epoch(epoch):
        calls.append(("eval", epoch))
        return {"acc1": acc1s[epoch], "acc5": 50.0, "global_acc1": 1.0, "local_acc1": 2.0, "loss": 3.0, "n": 4}

    def save(name, epoch):
        calls.append(("save", name, epoch))
        saved.append((name, epoch))

    records = run_epochs(args, start_epoch, train_epoch, eval_epoch, lambda epoch: calls.append(("sched", epoch)), save,
                         logging.getLogger("test_train_driver"), n_parameters=7, n_val=4)
    lines = [json.loads(ln) for ln in open(tmp_path / "train-logs" / "scalars.jsonl")]
    return records, saved, calls, lines, SCALARS


def test_epoch_loop_best_checkpoint_and_periodic_checkpoints(tmp_path):
    records, saved, calls, lines, names = _run(tmp_path, [10.0, 10.0, 30.0, 20.0], save_ep_freq=2)
    # epoch-best only where acc1 STRICTLY exceeds the best so far (0.0 at the start): epochs 0 and 2
    assert [e for n, e in saved if n == "epoch-best.pth"] == [0, 2]
    # checkpoint-e exactly where (e + 1) % save_ep_freq == 0
    assert [(n, e) for n, e in saved if n != "epoch-best.pth"] == [("checkpoint-1.pth", 1), ("checkpoint-3.pth", 3)]
    # order inside an epoch: train, scheduler step, periodic checkpoint, evaluation, best checkpoint (main.py:418-471)
    assert calls[:5] == [("train", 0), ("sched", 0), ("eval", 0), ("save", "epoch-best.pth", 0), ("train", 1)]
    assert calls[5:9] == [("sched", 1), ("save", "checkpoint-1.pth", 1), ("eval", 1), ("train", 2)]
    assert [r["epoch"] for r in records] == [0, 1, 2, 3]
    assert records[2]["test_acc1"] == 30.0 and records[2]["train_loss"] == pytest.approx(1.8) and records[2]["n_parameters"] == 7
    assert len(lines) == 4
    for e, ln in enumerate(lines):
        assert ln["epoch"] == e and all(k in ln for k in names) and len(names) == 6
    assert lines[3]["epoch/val_acc1"] == 20.0 and lines[3]["epoch/val_acc5"] == 50.0 and lines[1]["epoch/train_loss"] == pytest.approx(1.9)


def test_epoch_loop_never_saves_a_best_at_zero_accuracy(tmp_path):
    records, saved, _, lines, _ = _run(tmp_path, [0.0, 0.0], save_ep_freq=1)
    assert saved == [("checkpoint-0.pth", 0), ("checkpoint-1.pth", 1)] and len(lines) == 2 and len(records) == 2


def test_epoch_loop_starts_at_start_epoch(tmp_path):
    records, saved, calls, lines, _ = _run(tmp_path, [10.0, 10.0, 30.0, 20.0], save_ep_freq=400, start_epoch=2)
    assert [r["epoch"] for r in records] == [2, 3] and calls[0] == ("train", 2) and [ln["epoch"] for ln in lines] == [2, 3]
    assert saved == [("epoch-best.pth", 2)]


class _FakeOptimizer:
    ema = None

    def __init__(self):
        self.loaded = None

    def load_state_dict(self, sd):
        self.loaded = sd

    def load_ema_state_dict(self, sd):
        self.ema = sd


def test_resume_from_epoch_1_starts_at_2(tmp_path):
    from protopformer_amd.train import get_args_parser, resume
    lin = torch.nn.Linear(3, 2)
    sched = types.SimpleNamespace(state=None)
    sched.load_state_dict = lambda sd: setattr(sched, "state", sd)
    path = tmp_path / "checkpoint-1.pth"
    torch.save({"model": {k: v + 1.0 for k, v in lin.state_dict().items()}, "optimizer": {"marker": 5}, "lr_scheduler": {"t": 1}, "epoch": 1,
                "model_ema": {"w": torch.ones(1)}, "args": None}, path)
    before = lin.weight.detach().clone()
    args = get_args_parser().parse_args(["--resume", str(path)])
    opt = _FakeOptimizer()
    assert resume(args, lin, opt, sched, logging.getLogger("test_train_driver")) == 2 and args.start_epoch == 2
    assert torch.equal(lin.weight, before + 1.0) and opt.loaded == {"marker": 5} and sched.state == {"t": 1} and opt.ema is not None
    # --eval: the model only, the start epoch stays
    args = get_args_parser().parse_args(["--resume", str(path), "--eval"])
    opt2 = _FakeOptimizer()
    assert resume(args, lin, opt2, sched, logging.getLogger("test_train_driver")) == 0 and opt2.loaded is None
    with pytest.raises(ValueError, match="URL"):
        resume(get_args_parser().parse_args(["--resume", "https://example.org/x.pth"]), lin, opt, sched, logging.getLogger("test_train_driver"))


# ------------------------------------------------------------------------------------------------ EvalMeter across ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _meter_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from protopformer_amd.engine import EvalMeter
    m = EvalMeter("cpu")
    #            n    ce sum        top-1 top-5 global local bad reserved
    m.acc.copy_(torch.tensor([[3.0, 1.5, 1.0, 2.0, 1.0, 0.0, 0.0, 0.0], [5.0, 2.5, 3.0, 5.0, 2.0, 4.0, 0.0, 0.0]][rank], dtype=torch.float64))
    m.reduce_()
    r = m.result()
    ok = m.acc.tolist() == [8.0, 4.0, 4.0, 7.0, 3.0, 4.0, 0.0, 0.0]
    ok = ok and r == dict(acc1=50.0, acc5=87.5, global_acc1=37.5, local_acc1=50.0, loss=0.5, n=8)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_eval_meter_reduce_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_meter_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_eval_meter_single_process():
    from protopformer_amd.engine import EvalMeter
    m = EvalMeter("cpu")
    m.reduce_()                                            # no process group: nothing happens
    assert m.acc.dtype == torch.float64 and m.acc.tolist() == [0.0] * 8
    with pytest.raises(ValueError, match="no sample"):
        m.result()
    m.acc[0], m.acc[6] = 4.0, 1.0
    with pytest.raises(ValueError, match="outside"):
        m.result()
    m.reset()
    assert m.acc.tolist() == [0.0] * 8
    with pytest.raises(ValueError, match="device tensor"):   # no CPU path for the metrics themselves
        m.update(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64))
