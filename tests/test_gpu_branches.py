"""PPNet._branches' named record and PPNet.eval_branches: the pooled activations carry the prototype layer's graph, the arg-max is the
one the max-pool took, the record aliases nothing a later forward rewrites, and the eval pass leaves the mode as found."""
import pytest
import torch

from helpers import build_micro, micro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model_and_batches():
    sd, cfg, z = micro("micro_deit.npz")
    x = torch.from_numpy(z["img"][:2]).cuda()
    g = torch.Generator().manual_seed(5)
    return build_micro(cfg, sd), x, torch.randn(x.shape, generator=g).cuda()


def bits(t):
    return t.contiguous().view(torch.int32)


def test_record_fields_and_identities(model_and_batches):
    from protopformer_amd.protopformer import Branches
    m, x, x2 = model_and_batches
    m.train()
    assert m.prototype_vectors.requires_grad
    r = m._branches(x, want_dist=False)
    B, P = x.shape[0], m.num_prototypes
    assert isinstance(r, Branches) and r._fields == ("f", "cls_attn", "idx", "act_full", "dist", "logits", "logits_global", "logits_local",
                                                      "act_max_local", "act_max_global", "argmax")
    assert r.act_max_local.grad_fn is not None and r.act_max_global.grad_fn is not None
    assert r.argmax.dtype == torch.int32 and tuple(r.argmax.shape) == (B, P) and m._last_argmax is r.argmax and not r.argmax.requires_grad
    assert tuple(r.act_max_local.shape) == (B, P) and tuple(r.act_max_global.shape) == (B, m.num_prototypes_global)
    assert torch.equal(bits(r.act_max_local), bits(r.act_full.max(-1).values))
    assert torch.equal(bits(r.act_full.gather(-1, r.argmax.long()[..., None])[..., 0]), bits(r.act_max_local))
    assert not hasattr(m, "_last_act_max")
    # a later forward on another batch rewrites nothing the record holds
    before = [None if t is None else t.detach().clone() for t in r]
    r2 = m.eval_branches(x2)
    assert m.training and not torch.equal(r2.logits, r.logits)
    for name, t, was in zip(r._fields, r, before):
        same = torch.equal(t.detach().contiguous().view(torch.uint8), was.contiguous().view(torch.uint8))
        assert t.dtype == was.dtype and same, f"{name} changed under a later forward"
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("start", [True, False], ids=["train", "eval"])
def test_eval_branches(model_and_batches, start):
    m, x, _ = model_and_batches
    m.train(start)
    r = m.eval_branches(x)
    assert m.training is start and all(q.training is start for q in m.modules())
    assert all(t is None or (t.grad_fn is None and not t.requires_grad) for t in r)
    m.eval()
    with torch.no_grad():
        logits = m(x)[0]
    assert torch.equal(bits(r.logits), bits(logits))
