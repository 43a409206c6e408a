"""PPNet on the MI355X kernels: the reference's model API (protopformer.py:12-401, 455-487) as a drop-in.

``construct_PPNet(...)`` / ``PPNet.forward`` / ``get_PPC_loss`` / ``push_forward`` keep the reference's signatures,
return tuples, attribute names and state-dict keys; underneath, every FLOP runs in the HIP library
(protopformer_amd/lib/libppf_hip.so, C ABI in include/ppf_hip.h).  Python here wires shapes, autograd and buffers.
There is no CPU / eager fallback: without the built library or off a GPU, forward() raises.
"""
import contextlib
import math
import os
import weakref
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops
from .backbone import DEIT_FNS, TokensFn, droppath_scales, wgrad_lane
from .deit import MyVisionTransformer
from .flat import FlatStore
from .mixup import (LabelSmoothingCrossEntropy, Mixup, SoftCrossEntropyFn, SoftTargetCrossEntropy, create_criterion,  # noqa: F401
                    create_mixup, dense_target)

ARCHS = {
    "deit_tiny_patch16_224": dict(kind="deit", embed_dim=192, depth=12, num_heads=3),
    "deit_small_patch16_224": dict(kind="deit", embed_dim=384, depth=12, num_heads=6),
    "deit_base_patch16_224": dict(kind="deit", embed_dim=768, depth=12, num_heads=12),           # deit:315-328
    "cait_xxs24_224": dict(kind="cait", embed_dim=192, depth=24, num_heads=4, init_scale=1e-5),
    # cait_s24_224 (cait:379-383: 8 heads) is NOT offered: csrc/cait.hip keeps all heads of the talking-heads mix in registers and is
    # specialised for H <= 4 (cait_xxs24 / xs24 shapes); construct_PPNet raises KeyError for it instead of running something else.
}


def _load_pretrained(model, name):
    """The reference downloads ImageNet weights (deit:296-301); there is no network here, so a local file is required."""
    root = os.environ.get("PPF_PRETRAINED_DIR", "")
    path = os.path.join(root, name + ".pth")
    if not root or not os.path.exists(path):
        raise FileNotFoundError(f"pretrained=True needs {name}.pth under $PPF_PRETRAINED_DIR (no network access); "
                                "pass pretrained=False for seeded random init")
    ck = torch.load(path, map_location="cpu")
    model.load_state_dict(ck.get("model", ck), strict=False)


def build_features(base_architecture, pretrained=False, img_size=224, drop_path=0.1):
    """tools/deit_features.py:65-90, tools/cait_features.py:4-25: the `features` module of a PPNet."""
    cfg = dict(ARCHS[base_architecture])
    kind = cfg.pop("kind")
    if kind == "deit":
        m = MyVisionTransformer(img_size=img_size, patch_size=16, drop_path_rate=drop_path, **cfg)
    else:
        from .cait import MyCait
        m = MyCait(img_size=img_size, patch_size=16, drop_path_rate=drop_path, **cfg)
    if pretrained:
        _load_pretrained(m, base_architecture)
    return m


# ------------------------------------------------------------------------------------------------ autograd nodes
_KEEP_DIST = os.environ.get("PPF_PROTO_KEEP_DIST", "0") != "0"      # A/B: write and save the (B,P,k) distance map in training as before round 5


# The PPC loss only sends a gradient to the ppc prototypes of each sample's own class.  Instead of scattering it into a dense (B,P,T)
# tensor that the prototype-layer backward would scan twice, PPCLossFn.backward hands autograd a zero-stride placeholder of that shape
# and parks the block rows here, keyed by the placeholder's storage; ProtoLayerFn.backward picks them up (ppf_proto_bwd_rows).  Only taken
# when the activation map comes straight (through views) from ProtoLayerFn; a gradient that autograd had to combine with another one
# arrives dense (placeholder zeros + the other gradient) and gets the parked rows added (_rows_for).
_PROTO_ROWS = True          # (module attribute, no environment switch: tests/test_gpu_train_state.py sets it to False to get the dense exchange as the referee)
_PENDING_ROWS = {}


def _rows_for(g_full):
    """(rows, label, ppc), g_full: the block rows parked for this gradient (then g_full is None), or (None, g_full) for an ordinary dense
    tensor.  When autograd has ADDED the placeholder (zeros) to another consumer's gradient, g_full arrives dense with the rows still
    parked: they are folded into a copy of it (rare path, plain indexing) so that such a graph gets the right gradient by default."""
    if not _PENDING_ROWS:
        return None, g_full
    if g_full is not None and not any(g_full.stride()):
        hit = _PENDING_ROWS.pop(g_full.data_ptr(), None)
        if hit is not None:
            return hit[1:], None
    if g_full is not None and len(_PENDING_ROWS) == 1:
        _, (_, rows, label, ppc) = _PENDING_ROWS.popitem()
        B, P = g_full.shape[0], g_full.shape[1]
        g = g_full.reshape(B, P // ppc, ppc, -1).clone()
        g[torch.arange(B, device=g.device), label] += rows.reshape(B, ppc, -1)
        return None, g.reshape(g_full.shape)
    _PENDING_ROWS.clear()
    raise RuntimeError("protopformer_amd: a block-form PPC gradient is parked but the prototype layer received no activation-map gradient "
                       "to attach it to")


_ZERO_POOL = {}


def _zero_holder(device):
    """One element of a per-device pool of fp32 zeros (never written; rotating, so that two pending gradients get distinct addresses)."""
    ent = _ZERO_POOL.get(device)
    if ent is None:
        ent = _ZERO_POOL[device] = [ops.zeros((64,), torch.float32, device), 0]
    ent[1] = (ent[1] + 1) % 64
    return ent[0][ent[1]:ent[1] + 1]


def _check_rows_consumed():
    if _PENDING_ROWS:
        _PENDING_ROWS.clear()
        raise RuntimeError("protopformer_amd: a block-form PPC gradient was produced but no prototype-layer backward consumed it; "
                           "(the activation map was consumed outside ProtoLayerFn)")


def _from_proto_layer(t):
    fn = t.grad_fn
    for _ in range(4):                                    # through reshape / view nodes
        if fn is None:
            return False
        if type(fn).__name__ == "ProtoLayerFnBackward":
            return True
        nxt = [f for f, _ in fn.next_functions if f is not None]
        if len(nxt) != 1 or "View" not in type(fn).__name__ and "Reshape" not in type(fn).__name__:
            return False
        fn = nxt[0]
    return False


class ProtoLayerFn(torch.autograd.Function):
    """get_activations for both branches (protopformer.py:236-247, 311-312)."""

    @staticmethod
    def forward(ctx, f, protos_local, protos_global, ppnet, want_dist):
        B, T1, Dp = f.shape
        k = T1 - 1
        act_kind = 0 if ppnet.prototype_activation_function == "log" else 1
        pl = protos_local.reshape(protos_local.shape[0], Dp)
        pg = protos_global.reshape(protos_global.shape[0], Dp)
        need_bwd = any(ctx.needs_input_grad)
        # training keeps ONE (B,P,k) map: the backward takes d act / d dist from the activations themselves (ppf_proto_bwd map_is_act), so the
        # distance map (166 MB at config 3) is only written when the caller asks for it (eval / push)
        # (k == 1: the pooled branch degenerates to one token and takes the single-token backward, which reads the distance map)
        keep_dist = need_bwd and (_KEEP_DIST or k == 1)
        act_l, argmax, dist, act_full = ops.proto_fwd(f, 1, k, pl, act_kind, ppnet.epsilon, want_dist=keep_dist or want_dist, want_act=True)
        act_g, _, dist_g, _ = ops.proto_fwd(f, 0, 1, pg, act_kind, ppnet.epsilon, want_dist=need_bwd, want_act=False)
        ctx.set_materialize_grads(False)
        if need_bwd:
            ctx.save_for_backward(f, protos_local, protos_global, dist if keep_dist else act_full)
            ctx.aux = (argmax, not keep_dist, dist_g, act_kind, ppnet)
        if dist is None:
            dist = act_full.new_empty(0)
        ctx.mark_non_differentiable(*(t for t in (dist, argmax) if t is not None))
        return act_l, act_full, act_g, dist, argmax          # argmax: None when the local branch has one token (ops.proto_fwd)

    @staticmethod
    def backward(ctx, g_l, g_full, g_g, _g_dist, _g_argmax):
        f, _, _, dist = ctx.saved_tensors                 # dist: the distance map, or (from_act) the activation map
        argmax, from_act, dist_g, act_kind, ppnet = ctx.aux
        protos_local, protos_global = ppnet.prototype_vectors, ppnet.prototype_vectors_global
        store = ppnet.flat_store()
        store.attach_all_grads()
        B, T1, Dp = f.shape
        # every token row is written when both branches carry a gradient (the local rows 1.., the cls row 0): no zero fill then
        full = (g_l is not None or g_full is not None) and g_g is not None        # (a block-form g_full is a placeholder tensor, not None)
        df = torch.empty(f.shape, dtype=f.dtype, device=f.device) if full else ops.zeros(f.shape, f.dtype, f.device)
        lane = wgrad_lane(store)      # prototype gradients feed only the optimizer: side stream, under the backbone backward
        torch.autograd.Variable._execution_engine.queue_callback(lane.join)     # ... joined when this backward pass ends
        rows, g_full = _rows_for(g_full)

        def branch(t0, T, protos, dmap, gf, gm, am, rows=None, from_act=False):
            """One branch's backward: prototype gradients on the side stream, token gradients (into df) on the main stream."""
            pv = protos.reshape(-1, Dp)
            kw = dict(rows=rows, from_act=from_act)
            side = lambda: ops.proto_bwd(f, t0, T, pv, dmap, gf, gm, am, None, store.grad_view(protos).reshape(-1, Dp), act_kind, ppnet.epsilon, **kw)
            reads = [t for t in (f, dmap, gf, gm, am) + (rows[:2] if rows is not None else ()) if t is not None]
            # the side stream starts on the prototype gradients BEFORE the main stream's token-gradient kernels are enqueued: the two
            # only share inputs, and the lane orders itself behind whatever the main stream has enqueued at submit time
            # (+1.4 % in round 2, +0.6 % again in round 6 against the other order: profiles/r6_proto_order.txt)
            lane.submit(side, reads, tag="PROTO")
            ops.proto_bwd(f, t0, T, pv, dmap, gf, gm, am, df, None, act_kind, ppnet.epsilon, **kw)

        if g_l is not None or g_full is not None or rows is not None:
            branch(1, T1 - 1, protos_local, dist, g_full.contiguous() if g_full is not None else None, g_l.contiguous() if g_l is not None else None,
                   argmax, rows=rows, from_act=from_act)
        if g_g is not None:
            branch(0, 1, protos_global, dist_g, None, g_g.contiguous(), None)
        return df, None, None, None, None


class LogitsFn(torch.autograd.Function):
    """logits = coe * act_g W_g^T + (1 - coe) * act_l W_l^T with frozen W (protopformer.py:314-316)."""

    @staticmethod
    def forward(ctx, act_g, act_l, w_g, w_l, coe):
        B, C = act_g.shape[0], w_g.shape[0]
        lg = torch.empty((B, C), dtype=torch.float32, device=act_g.device)
        ll = torch.empty_like(lg)
        logits = torch.empty_like(lg)
        ops.sgemm_pair(act_g, w_g, lg, C, act_g.shape[1], (act_g.shape[1], 1), (w_g.shape[1], 1), 1.0,
                       act_l, w_l, ll, C, act_l.shape[1], (act_l.shape[1], 1), (w_l.shape[1], 1), 1.0, B, total=logits, c0=coe, c1=1.0 - coe)
        ctx.save_for_backward(w_g, w_l)
        ctx.coe = coe
        ctx.mark_non_differentiable(lg, ll)
        return logits, lg, ll

    @staticmethod
    def backward(ctx, dlogits, _dlg, _dll):
        w_g, w_l = ctx.saved_tensors
        dlogits = dlogits.contiguous()
        B, C = dlogits.shape
        dg = torch.empty((B, w_g.shape[1]), dtype=torch.float32, device=dlogits.device)
        dl = torch.empty((B, w_l.shape[1]), dtype=torch.float32, device=dlogits.device)
        # dg[b, p] = coe * sum_c dlogits[b, c] W_g[c, p]: "B" operand indexed [n = p, k = c] -> strides (1, P)
        ops.sgemm_pair(dlogits, w_g, dg, w_g.shape[1], C, (C, 1), (1, w_g.shape[1]), ctx.coe,
                       dlogits, w_l, dl, w_l.shape[1], C, (C, 1), (1, w_l.shape[1]), 1.0 - ctx.coe, B)
        return dg, dl, None, None, None


class PPCLossFn(torch.autograd.Function):
    """get_PPC_loss (protopformer.py:259-288): returns (cov_loss, mean_loss)."""

    @staticmethod
    def forward(ctx, act_full, idx, label, ppc, side, cov_thresh, mean_thresh):
        act = act_full.reshape(act_full.shape[0], act_full.shape[1], -1).contiguous()
        loss, gcov, gmean = ops.ppc_loss(act, idx, label, ppc, side, cov_thresh, mean_thresh)
        ctx.save_for_backward(gcov, gmean, label)
        ctx.shape = act_full.shape
        ctx.block_rows = _PROTO_ROWS and ppc <= 16 and act.shape[2] >= 2 and _from_proto_layer(act_full)
        ctx.set_materialize_grads(False)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, up_cov, up_mean):
        gcov, gmean, label = ctx.saved_tensors
        uc = up_cov.reshape(1).float().contiguous() if up_cov is not None else None
        um = up_mean.reshape(1).float().contiguous() if up_mean is not None else None
        if ctx.block_rows:
            rows = ops.ppc_loss_bwd_rows(gcov, gmean, uc, um)
            holder = _zero_holder(gcov.device)        # its storage address is the key; zeros, so that a sum with another gradient stays exact
            _PENDING_ROWS[holder.data_ptr()] = (holder, rows, label, gcov.shape[1])
            torch.autograd.Variable._execution_engine.queue_callback(_check_rows_consumed)
            return holder.expand(ctx.shape), None, None, None, None, None, None
        g_full = ops.ppc_loss_bwd(gcov, gmean, uc, um, label, ctx.shape[1])
        return g_full.reshape(ctx.shape), None, None, None, None, None, None


class CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label):
        loss, dlogits = ops.cross_entropy(logits.contiguous(), label)
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, up):
        (dlogits,) = ctx.saved_tensors
        if ops.is_const_one(up):                                                    # seeded by the train loop's cached one: nothing to scale
            return dlogits, None
        return ops.scale_by_scalar(dlogits, up.float().contiguous()), None          # chain rule with the upstream (device) scalar


class WeightedLossFn(torch.autograd.Function):
    """loss = ce + c_cov * cov + c_mean * mean (tools/engine_proto.py:61-64) as one launch; the backward hands out cached constants when
    it is seeded with the cached one (ops.const_scalar), so the loss arithmetic costs no further launches."""

    @staticmethod
    def forward(ctx, ce, cov, mean, c_cov, c_mean):
        ctx.c = (float(c_cov), float(c_mean))
        return ops.axpbypcz(ce.reshape(1), cov.reshape(1), mean.reshape(1), 1.0, c_cov, c_mean).reshape(())

    @staticmethod
    def backward(ctx, up):
        c_cov, c_mean = ctx.c
        if ops.is_const_one(up):
            return up, ops.const_scalar(up.device, c_cov), ops.const_scalar(up.device, c_mean), None, None
        return up, up * c_cov, up * c_mean, None, None


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() (main.py:390) on the HIP kernel.  Like torch's, it also takes probability targets: a floating-point [B, C]
    target (CutMix-only Mixup under the reference's flag defaults, main.py:384-390) runs the dense soft-target kernel."""

    def forward(self, logits, target):
        if target.is_floating_point():
            return SoftCrossEntropyFn.apply(logits, dense_target(logits, target), None, 0.0)
        return CrossEntropyFn.apply(logits, target)


# ------------------------------------------------------------------------------------------------ PPNet
class Branches(NamedTuple):
    """What one pass of PPNet._branches leaves on the device.  f (B, 1 + k, Dp) latent tokens (cls first), cls_attn (B, Np) rollout scores,
    idx (B, k) int32 grid cells of the reserved tokens, act_full (B, P, k) the local activation map, dist its distance map (empty unless
    asked for), logits / logits_global / logits_local (B, C), act_max_local (B, P) / act_max_global (B, P_global) the pooled activations
    (ProtoLayerFn's own outputs: they carry its grad_fn), argmax (B, P) int32 the token each local max-pool selected (None when k == 1)."""
    f: torch.Tensor
    cls_attn: torch.Tensor
    idx: torch.Tensor
    act_full: torch.Tensor
    dist: torch.Tensor
    logits: torch.Tensor
    logits_global: torch.Tensor
    logits_local: torch.Tensor
    act_max_local: torch.Tensor
    act_max_global: torch.Tensor
    argmax: Optional[torch.Tensor]


class PPNet(nn.Module):
    def __init__(self, features, img_size, prototype_shape, proto_layer_rf_info, num_classes, reserve_layers=[],
                 reserve_token_nums=[], use_global=False, use_ppc_loss=False, ppc_cov_thresh=2., ppc_mean_thresh=2,
                 global_coe=0.3, global_proto_per_class=10, init_weights=True, prototype_activation_function='log',
                 add_on_layers_type='bottleneck'):
        super().__init__()
        if not use_global or len(reserve_layers) != 1:
            # the reference's use_global=False / empty reserve_layers branches are broken (SURVEY quick facts)
            raise NotImplementedError("only the working reference configuration is supported: use_global=True with one reserve layer")
        if prototype_activation_function not in ('log', 'linear'):
            raise NotImplementedError("prototype_activation_function must be 'log' or 'linear'")
        self.img_size = img_size
        self.prototype_shape = list(prototype_shape)
        self.num_prototypes = prototype_shape[0]
        self.num_classes = num_classes
        self.reserve_layers = list(reserve_layers)
        self.reserve_token_nums = list(reserve_token_nums)
        self.use_global, self.use_ppc_loss = use_global, use_ppc_loss
        self.ppc_cov_thresh, self.ppc_mean_thresh = ppc_cov_thresh, ppc_mean_thresh
        self.global_coe = global_coe
        self.global_proto_per_class = global_proto_per_class
        self.epsilon = 1e-4
        self.reserve_layer_nums = list(zip(self.reserve_layers, self.reserve_token_nums))
        self.num_prototypes_global = num_classes * global_proto_per_class
        self.prototype_shape_global = [self.num_prototypes_global] + self.prototype_shape[1:]
        self.prototype_activation_function = prototype_activation_function
        assert self.num_prototypes % num_classes == 0
        self.num_prototypes_per_class = self.num_prototypes // num_classes
        ident = torch.zeros(self.num_prototypes, num_classes)
        ident[torch.arange(self.num_prototypes), torch.arange(self.num_prototypes) // self.num_prototypes_per_class] = 1
        ident_g = torch.zeros(self.num_prototypes_global, num_classes)
        ident_g[torch.arange(self.num_prototypes_global), torch.arange(self.num_prototypes_global) // global_proto_per_class] = 1
        self.prototype_class_identity, self.prototype_class_identity_global = ident, ident_g
        self.proto_layer_rf_info = proto_layer_rf_info
        self.features = features
        features._ppf_root = weakref.ref(self)
        k = self.reserve_token_nums[0]
        assert int(round(math.sqrt(k))) ** 2 == k, "reserve token number must be a perfect square (protopformer.py:165)"
        in_ch = features.embed_dim
        self.num_patches = features.patch_embed.num_patches
        if add_on_layers_type == 'bottleneck':
            # protopformer.py:90-107 (the signature default): pairs of 1x1 convolutions, the width halved pair by pair down to the prototype
            # dimension; ReLU after each, Sigmoid after the last.  Same Sequential indices (0, 2, 4, ...) as the reference's state dict.
            mods, cur, dp = [], in_ch, self.prototype_shape[1]
            while cur > dp or not mods:
                out = max(dp, cur // 2)
                mods += [nn.Conv2d(cur, out, kernel_size=1), nn.ReLU(), nn.Conv2d(out, out, kernel_size=1)]
                mods.append(nn.ReLU() if out > dp else nn.Sigmoid())
                cur = cur // 2
            self.add_on_layers = nn.Sequential(*mods)
        else:
            self.add_on_layers = nn.Sequential(nn.Conv2d(in_ch, self.prototype_shape[1], kernel_size=1), nn.Sigmoid())
        self.prototype_vectors = nn.Parameter(torch.rand(self.prototype_shape), requires_grad=True)
        self.prototype_vectors_global = nn.Parameter(torch.rand(self.prototype_shape_global), requires_grad=True)
        self.ones = nn.Parameter(torch.ones(self.prototype_shape), requires_grad=False)
        self.last_layer = nn.Linear(self.num_prototypes, num_classes, bias=False)
        self.last_layer_global = nn.Linear(self.num_prototypes_global, num_classes, bias=False)
        self.last_layer.weight.requires_grad = False
        self.last_layer_global.weight.requires_grad = False
        self.all_attn_mask = None
        self.teacher_model = None
        self.scale = self.prototype_shape[1] ** -0.5
        self._flat = None
        self._ppc_cache = None
        self.precise = False            # True (or PPF_PRECISE=1): fp32 verification forward (protopformer_amd/precise.py), no_grad only
        from .backbone import DEIT_FNS
        if isinstance(features, MyVisionTransformer):
            self._arch_fns = DEIT_FNS
        else:
            from .cait import CAIT_FNS
            self._arch_fns = CAIT_FNS
        if init_weights:
            self._initialize_weights()

    # ---- flat parameter store (lazy: built at first use on the device the module lives on)
    def flat_store(self):
        if self._flat is None or not self._flat.still_flat():
            dev = self.prototype_vectors.device
            if dev.type != "cuda":
                raise RuntimeError("protopformer_amd runs on an MI355X only: move the model to cuda (no CPU fallback path)")
            # entry names are the model's state-dict keys
            groups = [("features", [("features." + n, p) for n, p in self.features.named_parameters()]),
                      ("add_on_layers", [("add_on_layers." + n, p) for n, p in self.add_on_layers.named_parameters()]),
                      ("prototype_vectors", [("prototype_vectors", self.prototype_vectors)]),
                      ("prototype_vectors_global", [("prototype_vectors_global", self.prototype_vectors_global)])]
            self._flat = FlatStore(self, groups)
            wgrad_lane(self._flat)             # create the side stream now, before any communication stream claims a hardware queue
        return self._flat

    def _hook_params(self):
        hp = self.__dict__.get("_hook_cache")
        if hp is None:                  # the module tree walk costs ~0.4 ms: once, not per step
            hp = [p for p in list(self.features.parameters()) + list(self.add_on_layers.parameters()) if p.requires_grad]
            self.__dict__["_hook_cache"] = hp
        return hp

    def _apply(self, fn, *a, **k):
        """.to()/.cuda()/.float(): if the parameters were really re-materialised the flat views are re-created lazily (an optimizer
        built on the old store then refuses to step, FlatAdamW._check_store); a no-op move keeps the store."""
        out = super()._apply(fn, *a, **k)
        self.__dict__.pop("_hook_cache", None)
        if self._flat is not None and not self._flat.still_flat():
            self._flat = None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        if self._flat is not None:
            self._flat.invalidate()
        return out

    # ---- reference API
    def distance_2_similarity(self, distances):
        """protopformer.py:228-234 on an arbitrary tensor (elementwise helper kept for API parity; eval tools call it)."""
        if self.prototype_activation_function == 'log':
            return torch.log((distances + 1) / (distances + self.epsilon))
        return -distances

    def _tokens(self, x):
        B = x.shape[0]
        rates = self.features.droppath_rates()
        dp = droppath_scales(rates, B, x.device, self.training)
        if self.precise or os.environ.get("PPF_PRECISE", "0") != "0":
            from . import precise
            self.flat_store()
            return precise.tokens(self, x, dp)
        return TokensFn.apply(x, self, dp, *self._hook_params())

    def _branches(self, x, want_dist):
        f, cls_attn, idx = self._tokens(x)
        act_l, act_full, act_g, dist, argmax = ProtoLayerFn.apply(f, self.prototype_vectors, self.prototype_vectors_global, self, want_dist)
        logits, lg, ll = LogitsFn.apply(act_g, act_l, self.last_layer_global.weight, self.last_layer.weight, float(self.global_coe))
        self._last_argmax = argmax               # test-facing only; the tools take everything from the record
        return Branches(f, cls_attn, idx, act_full, dist, logits, lg, ll, act_l, act_g, argmax)

    @contextlib.contextmanager
    def eval_mode(self):
        """Eval mode for the block, then the mode that was found (also when the block raises).  Needs nothing of PPNet but nn.Module."""
        was_training = self.training
        self.eval()
        try:
            yield self
        finally:
            self.train(was_training)

    def eval_branches(self, x):
        """The record of one eval pass without a graph; the training mode is left as found."""
        with self.eval_mode(), torch.no_grad():
            return self._branches(x, want_dist=False)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("protopformer_amd.PPNet.forward needs a CUDA/HIP tensor (no CPU fallback path)")
        B = x.shape[0]
        k = self.reserve_token_nums[0]
        s = int(round(math.sqrt(k)))
        if not self.training:
            with torch.no_grad():
                r = self._branches(x, want_dist=True)
            return r.logits, (r.cls_attn, r.dist.reshape(B, self.num_prototypes, s, s), r.logits_global, r.logits_local)
        r = self._branches(x, want_dist=False)
        self._ppc_cache = (r.cls_attn, r.idx)
        total_proto_act = r.act_full.reshape(B, self.num_prototypes, s, s)
        attn_loss = ops.const_scalar(r.logits.device, 0.0).reshape(1)    # protopformer.py:333 (a constant zero: cached, never written)
        return r.logits, (None, attn_loss, total_proto_act, r.cls_attn, self.num_patches)

    def push_forward(self, x):
        with torch.no_grad():
            r = self._branches(x, want_dist=False)
        k = self.reserve_token_nums[0]
        s = int(round(math.sqrt(k)))
        return r.cls_attn, r.act_full.reshape(x.shape[0], self.num_prototypes, s, s)

    def get_PPC_loss(self, total_proto_act, cls_attn_rollout, original_fea_len, label):
        if label.is_floating_point() or label.dim() != 1:
            # the kernel reads int64 class labels (it picks each sample's prototypes by its label); the reference breaks on Mixup's
            # [B, C] targets too (protopformer.py:268-270)
            raise ValueError(f"get_PPC_loss needs integer class labels [B], got {tuple(label.shape)} {label.dtype}: the PPC loss cannot "
                             "be used with Mixup / CutMix soft targets")
        k = total_proto_act.shape[-1] * total_proto_act.shape[-2]
        cache = self._ppc_cache
        if cache is not None and cache[0] is cls_attn_rollout:
            idx = cache[1]                                  # same top-k + sort result the backbone already produced
        else:
            idx = ops.topk_sorted(cls_attn_rollout.contiguous().float(), k)
        side = int(original_fea_len ** 0.5)
        return PPCLossFn.apply(total_proto_act, idx, label.contiguous(), self.num_prototypes_per_class, side,
                               float(self.ppc_cov_thresh), float(self.ppc_mean_thresh))

    def set_last_layer_incorrect_connection(self, incorrect_strength):
        pos = torch.t(self.prototype_class_identity)
        self.last_layer.weight.data.copy_(pos + incorrect_strength * (1 - pos))
        pos_g = torch.t(self.prototype_class_identity_global)
        self.last_layer_global.weight.data.copy_(pos_g + incorrect_strength * (1 - pos_g))

    def _initialize_weights(self):
        for m in self.add_on_layers.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.set_last_layer_incorrect_connection(incorrect_strength=-0.5)

    def __repr__(self):
        return (f"PPNet(\n\tfeatures: {self.features.__class__.__name__},\n\timg_size: {self.img_size},\n\tprototype_shape: "
                f"{self.prototype_shape},\n\tproto_layer_rf_info: {self.proto_layer_rf_info},\n\tnum_classes: {self.num_classes},\n"
                f"\tepsilon: {self.epsilon}\n)")


def construct_PPNet(base_architecture, pretrained=True, img_size=224, prototype_shape=(2000, 512, 1, 1), num_classes=200,
                    reserve_layers=[], reserve_token_nums=[], use_global=False, use_ppc_loss=False, ppc_cov_thresh=1.,
                    ppc_mean_thresh=2., global_coe=0.5, global_proto_per_class=10, prototype_activation_function='log',
                    add_on_layers_type='bottleneck'):
    """Same signature and defaults as the reference (protopformer.py:455-487)."""
    features = build_features(base_architecture, pretrained=pretrained, img_size=img_size)
    return PPNet(features=features, img_size=img_size, prototype_shape=list(prototype_shape), proto_layer_rf_info=[14, 16, 16, 8.0],
                 num_classes=num_classes, reserve_layers=reserve_layers, reserve_token_nums=reserve_token_nums, use_global=use_global,
                 use_ppc_loss=use_ppc_loss, ppc_cov_thresh=ppc_cov_thresh, ppc_mean_thresh=ppc_mean_thresh, global_coe=global_coe,
                 global_proto_per_class=global_proto_per_class, init_weights=True,
                 prototype_activation_function=prototype_activation_function, add_on_layers_type=add_on_layers_type)
