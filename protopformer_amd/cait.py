"""CaiT backbone of ProtoPFormer on the HIP kernels (host-side orchestration only).

Mirrors the reference's ``MyCait`` (tools/cait_models_attn.py:188-345): 24 LayerScale blocks with talking-heads attention on the
patch tokens, then 2 class-attention blocks that update only the cls token, attention rollout + token reservation before class
block ``reserve_layer`` (cait:326-339).  Parameter names equal the reference's (``blocks.{i}.{gamma_1,gamma_2,norm1,attn.{qkv,proj,
proj_l,proj_w},norm2,mlp.{fc1,fc2}}``, ``blocks_token_only.{i}.{gamma_1,gamma_2,norm1,attn.{q,k,v,proj},norm2,mlp}``, ``pos_embed``
``(1,Np,D)``, ``cls_token``, ``norm``).  nn modules are parameter containers only; all arithmetic is in csrc/cait.hip + the GEMMs.
"""
import functools
import os

import torch
import torch.nn as nn

from . import ops
from .backbone import (LN_EPS, _ROLL_BATCH, _dp, _wgrad, block_bwd, block_fwd, branch_out, chunk_ready, dyb_ring, embed_bwd, embed_tokens, head_bwd,
                       mlp_bwd, row_tile_bwd, row_tile_fwd, t16_params, wgrad_lane)
from .deit import _Mlp, _PatchEmbed, _init_vit
from .ops import EPI_ATOMIC, EPI_BF16, EPI_F32, EPI_GELU, EPI_RESID


class _TalkingHeadAttn(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.proj_l = nn.Linear(num_heads, num_heads)
        self.proj_w = nn.Linear(num_heads, num_heads)


class _ClassAttn(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.q = nn.Linear(dim, dim, bias=True)
        self.k = nn.Linear(dim, dim, bias=True)
        self.v = nn.Linear(dim, dim, bias=True)
        self.proj = nn.Linear(dim, dim)


class LayerScaleBlock(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, drop_path, init_values, attn_cls):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = attn_cls(dim, num_heads)
        self.drop_path_rate = float(drop_path)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.gamma_1 = nn.Parameter(init_values * torch.ones(dim))
        self.gamma_2 = nn.Parameter(init_values * torch.ones(dim))


class MyCait(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=192, depth=24, num_heads=4, mlp_ratio=4., drop_path_rate=0.1,
                 init_scale=1e-5, depth_token_only=2, **_unused):
        super().__init__()
        self.embed_dim, self.depth, self.num_heads = embed_dim, depth, num_heads
        self.layer_nums = [depth, depth_token_only]
        self.patch_embed = _PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches, embed_dim))
        self.blocks = nn.ModuleList([LayerScaleBlock(embed_dim, num_heads, mlp_ratio, drop_path_rate, init_scale, _TalkingHeadAttn)
                                     for _ in range(depth)])                                         # constant rate (cait:206)
        self.blocks_token_only = nn.ModuleList([LayerScaleBlock(embed_dim, num_heads, 4.0, 0.0, init_scale, _ClassAttn)
                                                for _ in range(depth_token_only)])
        self.norm = nn.LayerNorm(embed_dim, eps=LN_EPS)
        nn.init.trunc_normal_(self.pos_embed, std=.02)
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.apply(_init_vit)

    def droppath_rates(self):
        return [r for blk in self.blocks for r in (blk.drop_path_rate, blk.drop_path_rate)]

    def __repr__(self):
        return "MyCait(hip)" + super().__repr__()[len("MyCait"):]

    def _store(self):
        root = getattr(self, "_ppf_root", None)
        if root is None:
            raise RuntimeError("features module must be owned by a protopformer_amd.PPNet (flat parameter store)")
        return root().flat_store()

    @torch.no_grad()
    def forward_feature_patch_embed_all(self, x):
        """cait:303-312 (inference-only compatibility wrapper): returns (cls_tokens [B,1,D], x [B,Np,D])."""
        xe = embed_tokens(self, self._store(), x, lead=0)
        return self.cls_token.expand(x.shape[0], -1, -1), xe

    @torch.no_grad()
    def forward_feature_mask_train_direct(self, cls_embed, x_embed, token_attn=None, reserve_layer_nums=[]):
        """cait:314-345 (inference-only compatibility wrapper)."""
        (layer, k), = reserve_layer_nums
        u, cls_attn, idx, _ = cait_blocks_fwd(self, self._store(), x_embed.contiguous(), layer, k, dp=None, save=False)
        B, N1, D = u.shape
        y, _, _ = ops.layernorm_fwd(u.reshape(B * N1, D), self.norm.weight, self.norm.bias, LN_EPS)
        return y.float().reshape(B, N1, D), (cls_attn, None)


# ------------------------------------------------------------------------------------------------ forward
def require_th_cover(H, N, D, training):
    """Raises ValueError unless the talking-heads kernels cover (heads, tokens, width); training also needs th_grads' cover.  There is
    no other path: a shape outside the cover is refused by name, not run slower.  Host predicates only (no GPU needed)."""
    if ops.th_fused_ok(H, N, D) and (not training or ops.th_grads_ok(H, N, D)):
        return
    raise ValueError(f"talking-heads attention with H={H} heads, N={N} tokens, D={D} width is outside the kernels' cover"
                     f"{' for training' if training and ops.th_fused_ok(H, N, D) else ''}: head width D/H must be 32, 48 or 64, "
                     "with 2 or 4 heads, the K and V images of all heads (2*H*N*(D/H)*2 bytes) within 160 KiB, and N <= 208 to train, <= 224 to infer")


def _th_attention_fwd(blk, qkv, B, H, N, D, hm_slot):
    """Talking-heads attention (cait:115-130) from packed qkv; returns (out bf16 [B*N,D], (rowmax, zinv), A bf16).  One launch up to and
    including A.V, nothing of size N x N in fp32: only the softmax statistics (and the bf16 A the dV product reads) are kept for backward."""
    a16, rowmax, zinv, ao = ops.th_fwd(qkv, blk.attn.proj_l.weight, blk.attn.proj_l.bias, blk.attn.proj_w.weight, blk.attn.proj_w.bias, hm_slot, B, H, N, D)
    return ao, (rowmax, zinv), a16


def cait_blocks_fwd(feats, store, x, reserve_layer, reserve_k, dp, save):
    """24 talking-heads blocks + class-attention blocks with rollout/reservation (cait:314-345).
    x fp32 [B,Np,D] -> (u_out [B,1+Np,D] fp32 = cat(cls, x), cls_token_attn [B,Np], idx int32 [B,k], saved)."""
    B, N, D = x.shape
    H = feats.num_heads
    require_th_cover(H, N, D, training=save)
    M = B * N
    NP = (N + 3) // 4 * 4
    depth = len(feats.blocks)
    hm = torch.empty((depth, B, N, NP), dtype=torch.float32, device=x.device)
    thr = torch.empty((depth, B), dtype=torch.int32, device=x.device)          # rollout discard thresholds per (layer, sample)
    lane = wgrad_lane(store)
    layers = []
    x = x.reshape(M, D)
    row_tile = row_tile_fwd(M, N, D, feats.blocks[0].mlp.fc1.out_features)      # every block has the same shape
    pre = None                                    # the coming block's norm1 out of the previous block's fc2 launch (backbone.block_fwd)

    def attn(blk, qkv):                           # attention of block i (the loop below) + what the side stream gets behind it
        ao, prob, a16 = _th_attention_fwd(blk, qkv, B, H, N, D, hm[i])
        # the rollout's order statistic of every layer, off the critical path (_ROLL_BATCH layers per main-stream event record)
        lane.submit(lambda i=i: ops.rollout_threshold(hm[i], thr[i], N), (hm, thr), defer=(i % _ROLL_BATCH != _ROLL_BATCH - 1) and i != depth - 1)
        return ao, dict(prob=prob, a16=a16)

    for i, blk in enumerate(feats.blocks):
        x, pre, L = block_fwd(blk, store, x, N, attn, (_dp(dp, 2 * i), _dp(dp, 2 * i + 1)), row_tile, pre, feats.blocks[i + 1] if i + 1 < depth else None, save)
        if save:
            layers.append(L)
    # ---- class-attention stage: only the cls token changes
    N1 = N + 1
    # (every sub-matrix copy of this stage goes through the library -- ops.gather_rows / copy_2d / cat_rows -- not through ATen: a
    # recorded step, engine.ReplayedTrainStep, replays library calls only)
    cls = ops.gather_rows(feats.cls_token.detach().reshape(1, D), _zero_rows(B, x.device))        # cls_token broadcast to [B, D]
    xt = x.reshape(B, N, D)
    policy = cls_attn = idx = None
    ca_layers = []
    rowmeans = torch.empty((len(feats.blocks_token_only), B, N1), dtype=torch.float32, device=x.device)
    for j, blk in enumerate(feats.blocks_token_only):
        if j == reserve_layer:
            init_rows = rowmeans[:j]                                              # class-attention rows produced so far (cait:249-251)
            lane.join()
            cls_attn, idx, policy = ops.rollout(hm, depth, B, N, reserve_k, lead=0, init_rows=init_rows, thr=thr)
        u = ops.cat_rows(cls, xt).reshape(B * N1, D)
        n, mean1, rstd1 = ops.layernorm_fwd(u, blk.norm1.weight, blk.norm1.bias, LN_EPS)
        kk = ops.gemm(n, store.w16(blk.attn.k.weight), epi=EPI_BF16, bias=blk.attn.k.bias)
        vv = ops.gemm(n, store.w16(blk.attn.v.weight), epi=EPI_BF16, bias=blk.attn.v.bias)
        qq = ops.gemm(n, store.w16(blk.attn.q.weight), epi=EPI_BF16, bias=blk.attn.q.bias, lda=N1 * D)      # the cls rows of n: row stride N1*D
        out, attn, zinv, _ = ops.class_attn_fwd(qq, kk, vv, policy, B, H, N1, D, rowmean=rowmeans[j])
        raw1 = torch.empty((B, D), dtype=torch.bfloat16, device=x.device) if save else None
        cls1 = ops.gemm(out, store.w16(blk.attn.proj.weight), epi=EPI_RESID, bias=blk.attn.proj.bias, res=cls, colscale=blk.gamma_1, aux_out=raw1)
        n2, mean2, rstd2 = ops.layernorm_fwd(cls1, blk.norm2.weight, blk.norm2.bias, LN_EPS)
        h = torch.empty((B, blk.mlp.fc1.out_features), dtype=torch.uint8, device=x.device)
        g = ops.gemm(n2, store.w16(blk.mlp.fc1.weight), epi=EPI_GELU, bias=blk.mlp.fc1.bias, aux_out=h)
        raw2 = torch.empty((B, D), dtype=torch.bfloat16, device=x.device) if save else None
        cls2 = ops.gemm(g, store.w16(blk.mlp.fc2.weight), epi=EPI_RESID, bias=blk.mlp.fc2.bias, res=cls1, colscale=blk.gamma_2, aux_out=raw2)
        if save:
            ca_layers.append(dict(u=u, n=n, mean1=mean1, rstd1=rstd1, q=qq, k=kk, v=vv, attn=attn, zinv=zinv, out=out, cls=cls, cls1=cls1,
                                  n2=n2, mean2=mean2, rstd2=rstd2, h=h, g=g, raw1=raw1, raw2=raw2, policy=policy))
        cls = cls2
    lane.join()
    u_out = ops.cat_rows(cls, xt)
    return u_out, cls_attn, idx, dict(sa=layers, ca=ca_layers)


_ZERO_ROWS = {}


def _zero_rows(B, device):
    """int32 [B] of zeros: the row map that broadcasts one source row to B rows (ops.gather_rows); cached per batch size."""
    key = (B, str(device))
    t = _ZERO_ROWS.get(key)
    if t is None:
        t = _ZERO_ROWS[key] = torch.zeros(B, dtype=torch.int32, device=device)
    return t


# ------------------------------------------------------------------------------------------------ backward
def _th_attention_bwd(store, blk, L, dao, B, H, N, D):
    """Backward of the talking-heads attention: returns dqkv bf16 [B*N, 3D]; accumulates proj_l / proj_w grads."""
    qkv, (rowmax, zinv), a16 = L["qkv"], L["prob"], L["a16"]
    gv = store.grad_view
    dqkv = torch.empty_like(qkv)
    # dA, the two head mixes and the softmax backward in registers; the parameter-gradient sums leave the main stream
    ds16, partial = ops.th_bwd(qkv, dao, blk.attn.proj_l.weight, blk.attn.proj_l.bias, blk.attn.proj_w.weight, rowmax, zinv, B, H, N, D)
    wgrad_lane(store).submit(lambda: ops.th_param_reduce(partial, B, H, N, gv(blk.attn.proj_w.weight), gv(blk.attn.proj_w.bias), gv(blk.attn.proj_l.bias),
                                                         gv(blk.attn.proj_l.weight)), (partial,),
                             defer=True)    # launched with the qkv weight gradient: one event record
    return ops.th_grads(qkv, dao, ds16, a16, dqkv, B, H, N, D)      # dQ, dK, dV in one launch


def cait_backward(ppnet, store, saved, df):
    feats = ppnet.features
    sa, ca = saved["layers"]["sa"], saved["layers"]["ca"]
    head = saved["head"]
    u_last = saved["x_last"]                               # [B, N1, D]
    B, N1, D = u_last.shape
    N, H = N1 - 1, feats.num_heads
    M = B * N
    dev = u_last.device
    gv = store.grad_view
    lane = wgrad_lane(store)
    # column-sum reductions (parameter grads) go to the side stream, each launched at once: parked until the lane's next submit measured
    # -6 % on this backbone, whose scale / cast passes are followed by main-stream work first (ops.layernorm_bwd)
    lnb = functools.partial(ops.layernorm_bwd, lane=lane)
    dnf = head_bwd(ppnet, store, saved, df)
    du = ops.zeros((B * N1, D), torch.float32, dev)
    lnb(dnf, u_last.reshape(B * N1, D), feats.norm.weight, head["meanf"], head["rstdf"], gv(feats.norm.weight),
                      gv(feats.norm.bias), dx_out=du, row_map=head["row_map"])
    du3 = du.reshape(B, N1, D)
    du2 = du.reshape(B, N1 * D)
    dcls = ops.copy_2d(torch.empty((B, D), dtype=torch.float32, device=dev), du2[:, :D])
    gs = getattr(ppnet, "_grad_sync", None)            # data-parallel: the final norm + add-on + prototype gradients are complete (round 6: this
    if gs is not None:                                 # chunk was launched LAST, 45 us of exchange behind the last backward kernel)
        chunk_ready(gs, lane, gs.tail_chunk)
    # ---- class-attention blocks (reverse)
    for j in range(len(ca) - 1, -1, -1):
        L, blk = ca[j], feats.blocks_token_only[j]
        dyb = lane.track(torch.empty((B, D), dtype=torch.bfloat16, device=dev))
        lnb(None, None, None, None, None, None, None, dres_in=dcls, cast_out=dyb, colscale=blk.gamma_2,
                          dbias_next=gv(blk.mlp.fc2.bias), branch=L["raw2"], dcolscale=gv(blk.gamma_2))
        dn2 = ops.gemm(mlp_bwd(store, blk, L, dyb, True), store.w16(blk.mlp.fc1.weight), trans_b=True, epi=EPI_BF16)
        lane.before_overwrite(dyb)
        lnb(dn2, L["cls1"], blk.norm2.weight, L["mean2"], L["rstd2"], gv(blk.norm2.weight), gv(blk.norm2.bias), dres_in=dcls,
                          dx_out=dcls, cast_out=dyb, colscale=blk.gamma_1, dbias_next=gv(blk.attn.proj.bias), branch=L["raw1"],
                          dcolscale=gv(blk.gamma_1))
        _wgrad(store, dyb, L["out"], blk.attn.proj.weight)
        dout = ops.gemm(dyb, store.w16(blk.attn.proj.weight), trans_b=True, epi=EPI_BF16)
        dq, dk, dv = ops.class_attn_bwd(L["q"], L["k"], L["v"], L["attn"], L["zinv"], dout, B, H, N1, D)
        # projections q (cls rows only), k, v
        # (q saw the cls rows of n only: row stride N1*D; the contraction is the batch, on the main stream and without split-K scratch)
        ops.gemm(dq, L["n"], trans_a=True, trans_b=True, epi=EPI_ATOMIC, out=gv(blk.attn.q.weight), colsum=gv(blk.attn.q.bias), ldb=N1 * D,
                 workspace=False)
        _wgrad(store, dk, L["n"], blk.attn.k.weight, blk.attn.k.bias)
        _wgrad(store, dv, L["n"], blk.attn.v.weight, blk.attn.v.bias)
        dnk = ops.gemm(dk, store.w16(blk.attn.k.weight), trans_b=True, epi=EPI_F32)
        dnv = ops.gemm(dv, store.w16(blk.attn.v.weight), trans_b=True, epi=EPI_F32)
        dnq = ops.gemm(dq, store.w16(blk.attn.q.weight), trans_b=True, epi=EPI_F32)
        dn16 = ops.merge3_cast(dnk, dnv, dnq, N1)
        ops.copy_2d(du2[:, :D], dcls)                      # gradient reaching this block's cls input through the residual path
        lnb(dn16, L["u"], blk.norm1.weight, L["mean1"], L["rstd1"], gv(blk.norm1.weight), gv(blk.norm1.bias), dres_in=du, dx_out=du)
        dcls = ops.copy_2d(torch.empty((B, D), dtype=torch.float32, device=dev), du2[:, :D])
    # cls_token parameter: sum over the batch of the cls gradient (column sums via the scale/cast pass)
    scratch = torch.empty((B, D), dtype=torch.bfloat16, device=dev)
    lnb(None, None, None, None, None, None, None, dres_in=dcls, cast_out=scratch, dbias_next=gv(feats.cls_token).reshape(D))
    # ---- talking-heads blocks (reverse)
    dx = ops.copy_2d(torch.empty((B, N * D), dtype=torch.float32, device=dev), du2[:, D:]).reshape(M, D)
    dyb = lane.track(torch.empty((M, D), dtype=torch.bfloat16, device=dev))
    last = feats.blocks[-1]
    lnb(None, None, None, None, None, None, None, dres_in=dx, dbias_next=gv(last.mlp.fc2.bias),
        **branch_out(store, dyb, sa[-1]["s2"], N, last.gamma_2, sa[-1]["raw2"]))
    # Input gradient of fc1 / qkv + LayerNorm backward + LayerScale terms of the branch below as one full-row kernel (csrc/rowgemm.hip,
    # RG_LNBWD_LS) wherever the shape is covered.  Half-sample tiles as in the forward pass (measured on this backbone, same box: 8 885 vs
    # 8 300 img/s with whole samples -- the opposite of deit_tiny, whose side stream carries relatively more weight-gradient work).
    # Where the input gradients are launches of their own, they read W transposed through the generic kernel.
    bwd = functools.partial(block_bwd, next_dyb=dyb_ring(lane, D), lnb=lnb, row_tile=row_tile_bwd(store, last, D, ops.rowgemm_tile_rows(M, N)),
                            dgrad=lambda dy16, weight, rows, which: ops.gemm(dy16, store.w16(weight), trans_b=True, epi=EPI_BF16),
                            attn_bwd=lambda blk, L, dao: _th_attention_bwd(store, blk, L, dao, B, H, N, D))
    bias_done = True                       # the producer of the current dyb has already accumulated the bias gradient of the Linear above it
    for i in range(len(sa) - 1, -1, -1):
        dyb, bias_done = bwd(feats.blocks[i], store, sa[i], dx, dyb, bias_done, (feats.blocks[i - 1], sa[i - 1]) if i > 0 else None)
        if gs is not None and i in gs.block_chunk:
            chunk_ready(gs, lane, gs.block_chunk[i])
    return embed_bwd(ppnet, store, saved, dx, 0)


CAIT_FNS = dict(embed=functools.partial(embed_tokens, lead=0), blocks=cait_blocks_fwd, backward=cait_backward, t16_params=t16_params)
