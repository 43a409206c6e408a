"""Thin host-side wrappers over the C-ABI kernels (no arithmetic here: allocation, shapes, launch)."""
import torch

from . import _lib

EPI_BF16, EPI_F32, EPI_GELU, EPI_SIGMOID_F32, EPI_RESID, EPI_DGELU, EPI_ATOMIC = range(7)


# the kernel bench.py's roofline probe (ppf_gemm_probe, HIP events inside the C entry point) reports on
DOMINANT_NAME = ("weight-gradient bf16 MFMA GEMM, split over the contraction, ordered partial tiles: wgrad8_kernel<4,2> / <2,4> (256x128 / 128x256 tiles) "
                 "and gemm_kernel<TA=1,TB=1,EPI_PARTIAL,COLSUM> (128x128)")


_WORKSPACE = {}        # general scratch, by (device, stream)
_GEMM_WS = {}          # split-K scratch of the weight-gradient GEMMs, by (device, stream)
_RETIRED_WS = []


def _workspace(device, nbytes, pool=_WORKSPACE):
    """Reusable scratch from `pool`, grown on demand: one buffer per (device, stream) -- the weight-gradient lane (backbone.WgradLane)
    runs its GEMMs on a second stream, concurrently with main-stream kernels that also use a workspace.
    pool=_GEMM_WS is used by the weight-gradient GEMMs and nothing else: every weight gradient writes its partial tiles into the same
    28 MB and the ordered reduce reads them straight back (they stay in the L2 / memory-side cache; giving every GEMM its own range
    and summing later was measured slower: profiles/r4_reduce_batch.txt)."""
    key = (device, _lib.stream_ptr())
    buf = pool.get(key)
    if buf is None or buf.numel() < nbytes:
        # a buffer that is outgrown stays allocated: a side stream may still be using it and torch's allocator knows nothing of that stream
        if buf is not None:
            _RETIRED_WS.append(buf)
        buf = torch.empty(max(nbytes, 64 << 20), dtype=torch.uint8, device=device)
        pool[key] = buf
    return buf


def _chk(t, dtype=None):
    assert t.is_cuda and t.is_contiguous(), "kernel operands must be contiguous CUDA tensors"
    if dtype is not None:
        assert t.dtype == dtype, f"expected {dtype}, got {t.dtype}"
    return t


def gemm(a, b, *, trans_a=False, trans_b=False, epi=EPI_BF16, out=None, bias=None, res=None, rowscale=None,
         rows_per_group=1, colscale=None, aux_in=None, aux_out=None, colsum=None, alpha=1.0, lda=None, ldb=None, workspace=True):
    """C[M,N] (+)= epi(sum_kc A(m,kc) B(n,kc)); a/b are 2-D bf16. Storage: a is [M,K] ([K,M] if trans_a),
    b is [N,K] ([K,N] if trans_b).  lda / ldb: a row stride larger than the row length -- the operand's rows are the first shape[1]
    entries of every lda (ldb) elements of the tensor (the cls rows of a [B*N1, D] token matrix: lda = N1*D).
    workspace=False: EPI_ATOMIC without the split-K scratch (fp32 atomics where the contraction is split at all)."""
    _chk(a, torch.bfloat16), _chk(b, torch.bfloat16)
    lda = a.shape[1] if lda is None else lda
    ldb = b.shape[1] if ldb is None else ldb
    M, K = (a.shape[1], a.numel() // lda) if trans_a else (a.numel() // lda, a.shape[1])
    N, Kb = (b.shape[1], b.numel() // ldb) if trans_b else (b.numel() // ldb, b.shape[1])
    assert K == Kb, f"contraction mismatch {K} vs {Kb}"
    if out is None:
        odt = torch.float32 if epi in (EPI_F32, EPI_SIGMOID_F32, EPI_RESID, EPI_ATOMIC) else torch.bfloat16
        out = torch.empty((M, N), dtype=odt, device=a.device)
        if epi == EPI_ATOMIC:
            zero_(out)
    ldaux = 0
    for t in (aux_in, aux_out):
        if t is not None:
            # EPI_GELU / EPI_DGELU: gelu' as 8-bit codes, ldaux counts BYTES (ABI >= 6); EPI_RESID: the bf16 unscaled branch
            _chk(t, torch.uint8 if epi in (EPI_GELU, EPI_DGELU) else torch.bfloat16)
            ldaux = t.shape[-1]
    ws = None
    if epi == EPI_ATOMIC and workspace:
        ws = _workspace(a.device, _lib.lib().ppf_gemm_workspace_bytes(M, N, K), _GEMM_WS)
    _lib.call("ppf_gemm_bf16", a, b, out, M, N, K, lda, ldb, out.shape[-1], int(trans_a), int(trans_b), epi,
              bias, res, res.shape[-1] if res is not None else 0, rowscale, rows_per_group, colscale, aux_in, aux_out, ldaux,
              colsum, float(alpha), ws, ws.numel() if ws is not None else 0)
    return out


# ------------------------------------------------------------------------------------------------ full-row GEMM + fused LayerNorm
def rowgemm_ok(D, K, rows_per_tile):
    """True when csrc/rowgemm.hip takes a product with output width D, contraction K and tiles of rows_per_tile rows."""
    return bool(_lib.lib().ppf_rowgemm_supported(int(D), int(K), int(rows_per_tile)))


_CU_COUNT = {}


def rowgemm_tile_rows(M, rows_per_sample, device=None, backward=False):
    """Tile height for the full-row GEMMs: one sample per workgroup, or less when whole samples would leave a third of the CUs without a
    workgroup (batch 128 on 256 CUs: 128 tiles of 197 rows).  Tiles need not end on sample boundaries: every epilogue is row-wise and the
    DropPath scale is indexed by the global row (rows_per_group).
    Forward: half a sample (255 tiles of 99 rows).  backward=True (callers whose side stream is busy with weight-gradient GEMMs while
    these one-per-CU workgroups run): tiles for ~62 % of the CUs, the rest stays free for the side stream -- measured on deit_tiny batch
    128, img/s: whole samples 24.3k, 144-176 rows 24.9-25.0k, half samples 23.6k."""
    dev = torch.cuda.current_device() if device is None else device
    cus = _CU_COUNT.get(dev)
    if cus is None:
        cus = _CU_COUNT[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    tiles = (M + rows_per_sample - 1) // rows_per_sample
    if 3 * tiles > 2 * cus or rows_per_sample <= 16:
        return rows_per_sample
    half = (rows_per_sample + 1) // 2
    if backward:
        target = max(1, int(0.62 * cus))
        return max(half, min(rows_per_sample, (M + target - 1) // target))
    return half


def rowgemm_bf16(a, b, rows_per_tile, bias=None):
    """bf16 [M, D] = a [M, K] @ b [D, K]^T (+ bias)."""
    _chk(a, torch.bfloat16), _chk(b, torch.bfloat16)
    M, K = a.shape
    D = b.shape[0]
    out = torch.empty((M, D), dtype=torch.bfloat16, device=a.device)
    _lib.call("ppf_rowgemm_bf16", a, b, M, D, K, K, b.shape[1], rows_per_tile, bias, out)
    return out


def rowgemm_resid_ln(a, b, res, rows_per_tile, bias=None, rowscale=None, rows_per_group=1, ln_w=None, ln_b=None, eps=1e-6, colscale=None, aux_out=None):
    """x_out = res + rowscale * colscale * (a @ b^T + bias) (fp32) and, with ln_w / ln_b, n = bf16(LN(x_out)), mean, rstd of the LayerNorm
    that follows; aux_out (bf16 [M, D], optional) receives the unscaled branch a @ b^T + bias.
    Returns (x_out, n, mean, rstd) (the last three None without a LayerNorm)."""
    _chk(a, torch.bfloat16), _chk(b, torch.bfloat16), _chk(res, torch.float32)
    M, K = a.shape
    D = b.shape[0]
    xout = torch.empty((M, D), dtype=torch.float32, device=a.device)
    n = mean = rstd = None
    if ln_w is not None:
        n = torch.empty((M, D), dtype=torch.bfloat16, device=a.device)
        mean = torch.empty(M, dtype=torch.float32, device=a.device)
        rstd = torch.empty(M, dtype=torch.float32, device=a.device)
    _lib.call("ppf_rowgemm_resid_ln", a, b, M, D, K, K, b.shape[1], rows_per_tile, bias, res, xout, rowscale, rows_per_group, colscale, aux_out,
              ln_w, ln_b, n, mean, rstd, float(eps))
    return xout, n, mean, rstd


def rowgemm_lnbwd(a, b, x, mean, rstd, w, dw, db, rows_per_tile, dres_in=None, dx_out=None, cast_out=None, rowscale=None, rows_per_group=1,
                  lane=None, defer_reduce=False, colscale=None, branch=None, dcolscale=None):
    """dn = a @ b^T is the gradient w.r.t. the output of LN(x); dx_out = dres_in + LN'(dn) (fp32), cast_out = bf16(rowscale * dx_out);
    dw / db (the LayerNorm's parameter gradients) += the column sums, reduced in a fixed order by a second small kernel (on `lane`,
    the side stream, when given).  colscale / branch / dcolscale: CaiT's LayerScale on the branch below (cast_out additionally times
    colscale, dcolscale += sum_m rowscale * dx_out * branch)."""
    _chk(a, torch.bfloat16), _chk(b, torch.bfloat16), _chk(x, torch.float32)
    M, K = a.shape
    D = b.shape[0]
    tiles = (M + rows_per_tile - 1) // rows_per_tile
    nparts = 3 if colscale is not None else 2
    part = torch.empty(tiles * nparts * D, dtype=torch.float32, device=a.device)
    if dx_out is None:
        dx_out = torch.empty((M, D), dtype=torch.float32, device=a.device)
    _lib.call("ppf_rowgemm_lnbwd", a, b, M, D, K, K, b.shape[1], rows_per_tile, x, mean, rstd, w, dres_in, dx_out, cast_out, rowscale, rows_per_group,
              colscale, branch, part, part.numel() * 4)
    red = lambda: _lib.call("ppf_rowgemm_colsum", part, tiles, D, nparts, dw, db, dcolscale)
    if lane is not None:
        lane.submit(red, (part,), defer=defer_reduce)
    else:
        red()
    return dx_out


def transpose_bf16_batched(src, dst, desc, n, total_tiles):
    _lib.call("ppf_transpose_bf16_batched", src, dst, desc, n, total_tiles)


def layernorm_fwd(x, w, b, eps=1e-6, row_map=None):
    """x fp32 [R, D] -> (y bf16 [rows, D], mean, rstd); rows = len(row_map) gathers source rows."""
    _chk(x, torch.float32)
    D = x.shape[-1]
    rows = row_map.numel() if row_map is not None else x.numel() // D
    y = torch.empty((rows, D), dtype=torch.bfloat16, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _lib.call("ppf_layernorm_fwd", x, row_map, w, b, y, mean, rstd, rows, D, float(eps))
    return y, mean, rstd


def layernorm_bwd(dy, x, w, mean, rstd, dw, db, *, dres_in=None, dx_out=None, row_map=None, cast_out=None, rowscale=None,
                  rows_per_group=1, colscale=None, dbias_next=None, branch=None, dcolscale=None, lane=None, defer_reduce=False):
    """dx_out[src] = dres_in[src] + LN'(dy); dw/db accumulate (+=). dy=None: pure scale/cast/colsum pass.
    Large calls write per-workgroup column partials and add them up in a second, deterministic kernel; with `lane`
    (backbone.WgradLane) that reduction -- parameter gradients only -- runs on the side stream; defer_reduce launches it together with
    the lane's next submit (one main-stream ordering event for both: +0.5 % on DeiT, where a weight gradient follows immediately;
    measured -6 % on CaiT, whose scale / cast passes are followed by main-stream work first)."""
    D = x.shape[-1] if x is not None else dres_in.shape[-1]
    if dy is not None:
        rows = dy.numel() // D
    else:
        rows = dres_in.numel() // D
    sums = (dw if dy is not None else None, db if dy is not None else None, dbias_next if cast_out is not None else None,
            dcolscale if (cast_out is not None and branch is not None) else None)
    part = None
    # fixed-order two-pass column sums at every size (bit-identical from run to run)
    if any(t is not None for t in sums):
        dev = (dy if dy is not None else dres_in).device
        part = torch.empty(_lib.lib().ppf_layernorm_bwd_blocks(rows) * 4 * D, dtype=torch.float32, device=dev)
    _lib.call("ppf_layernorm_bwd", dy, x, row_map, w, mean, rstd, dres_in, dx_out, dw, db, cast_out, rowscale, rows_per_group,
              colscale, dbias_next, branch, dcolscale, rows, D, part, part.numel() * 4 if part is not None else 0)
    if part is not None:
        red = lambda: _lib.call("ppf_layernorm_bwd_reduce", part, rows, D, *sums)
        if lane is not None:
            lane.submit(red, (part,), defer=defer_reduce, tag="LNRED")
        else:
            red()


def cast_bf16(src, dst=None):
    _chk(src, torch.float32)
    n = src.numel()
    assert n % 8 == 0
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    _lib.call("ppf_cast_f32_bf16", src, dst, n)
    return dst


def im2col_patch(img, patch):
    _chk(img, torch.float32)
    B, C, H, W = img.shape
    cols = torch.empty((B * (H // patch) * (W // patch), C * patch * patch), dtype=torch.bfloat16, device=img.device)
    _lib.call("ppf_im2col_patch", img, cols, B, C, H, W, patch)
    return cols


def assemble_tokens(tok, cls, pos, B, Np, D, lead):
    x = torch.empty((B, Np + lead, D), dtype=torch.float32, device=tok.device)
    _lib.call("ppf_assemble_tokens", tok, cls, pos, x, B, Np, D, lead)
    return x


def assemble_tokens_bwd(dx, dpos, dcls, B, Np, D, lead):
    dtok = torch.empty((B * Np, D), dtype=torch.bfloat16, device=dx.device)
    _lib.call("ppf_assemble_tokens_bwd", dx, dtok, dpos, dcls, B, Np, D, lead)
    return dtok


def attn_fwd_hm_ok(H, N, D):
    """The one-launch forward + head-mean kernel (csrc/attention.hip attn_fwd16_kernel) covers this (heads, tokens, width)."""
    return bool(_lib.lib().ppf_attn_fwd_hm_supported(H, N, D))


def attn_fwd(qkv, B, H, N, D, policy=None, self_keep=True, eps_n=0, headmean=None):
    """qkv bf16 [B*N, 3D] -> (out bf16 [B*N, D], rowmax, zinv [B,H,N]).  headmean (fp32 [B, N, NP], only where attn_fwd_hm_ok): the
    head-mean probability map of deit:104, written by the same launch."""
    _chk(qkv, torch.bfloat16)
    out = torch.empty((B * N, D), dtype=torch.bfloat16, device=qkv.device)
    rowmax = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    zinv = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    if headmean is not None:
        NP = (N + 3) // 4 * 4
        _lib.call("ppf_attn_fwd_hm", qkv, out, policy, rowmax, zinv, headmean, NP, B, H, N, D, int(self_keep), int(eps_n))
    else:
        _lib.call("ppf_attn_fwd", qkv, out, policy, rowmax, zinv, B, H, N, D, int(self_keep), int(eps_n))
    return out, rowmax, zinv


def attn_headmean(qkv, rowmax, zinv, B, H, N, D, policy=None, self_keep=True, out=None, eps_n=0):
    NP = (N + 3) // 4 * 4
    if out is None:
        out = torch.empty((B, N, NP), dtype=torch.float32, device=qkv.device)
    _lib.call("ppf_attn_headmean", qkv, policy, rowmax, zinv, out, NP, B, H, N, D, int(self_keep), int(eps_n))
    return out


def attn_bwd(qkv, out, dout, rowmax, zinv, B, H, N, D, policy=None, self_keep=True, eps_n=0):
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    _lib.call("ppf_attn_bwd", qkv, out, dout, dqkv, policy, rowmax, zinv, delta, B, H, N, D, int(self_keep), int(eps_n))
    return dqkv


def rollout_threshold(hm_layer, thr_out, N, discard_ratio=0.9):
    """thr_out [B] int32 <- per-sample key of the int(N*N*ratio)-th smallest entry of one layer's head-mean map [B, N, NP]."""
    B, _, NP = hm_layer.shape
    _lib.call("ppf_rollout_threshold", hm_layer, B, N, NP, int(N * N * discard_ratio), thr_out)


def rollout_outputs(B, N, k, lead, device):
    """(cls_attn [B,N-lead], idx int32 [B,k], policy [B,N-lead+1]) buffers for rollout(out=...)."""
    Nk = N - lead
    return (torch.empty((B, Nk), dtype=torch.float32, device=device), torch.empty((B, k), dtype=torch.int32, device=device),
            torch.empty((B, Nk + 1), dtype=torch.float32, device=device))


def rollout(hm, L, B, N, k, lead=1, init_rows=None, discard_ratio=0.9, identity=0.2, thr=None, out=None):
    """hm: [L,B,N,NP] fp32 head-mean attention. Returns (cls_attn [B,N-lead], idx int32 [B,k] ascending, policy [B,N-lead+1]);
    out = rollout_outputs(...) to write into existing buffers (no allocation: usable on the side-stream lane)."""
    _chk(hm, torch.float32)
    NP = hm.shape[-1]
    cls_attn, idx, policy = out if out is not None else rollout_outputs(B, N, k, lead, hm.device)
    n_init = init_rows.shape[0] if init_rows is not None else 0
    # discard counts in double precision, exactly like the reference's int(numel * ratio)
    kdrop, kdrop_init = int(N * N * discard_ratio), int((N + 1) * discard_ratio)
    _lib.call("ppf_rollout", hm, B * N * NP, L, B, N, NP, init_rows, n_init, lead, kdrop, kdrop_init, float(identity), k, thr, cls_attn, idx, policy)
    return cls_attn, idx, policy


def proto_fwd(tokens, t0, T, protos, act_kind=0, eps=1e-4, want_dist=True, want_act=True):
    """tokens fp32 [B, Ttot, Dp]; uses tokens[:, t0:t0+T]. protos fp32 [P, Dp]."""
    _chk(tokens, torch.float32), _chk(protos, torch.float32)
    B, Ttot, Dp = tokens.shape
    P = protos.shape[0]
    dev = tokens.device
    act_max = torch.empty((B, P), dtype=torch.float32, device=dev)
    argmax = torch.empty((B, P), dtype=torch.int32, device=dev) if T > 1 else None
    dist = torch.empty((B, P, T), dtype=torch.float32, device=dev) if want_dist else None
    act = torch.empty((B, P, T), dtype=torch.float32, device=dev) if want_act else None
    ws = _workspace(dev, _lib.lib().ppf_proto_fwd_workspace(P, Dp)) if T > 1 else None      # pre-split prototype planes (per-stream scratch)
    _lib.call("ppf_proto_fwd", tokens, Ttot * Dp, t0, T, protos, B, P, Dp, act_kind, float(eps), act_max, argmax, dist, act,
              ws, ws.numel() if ws is not None else 0)
    return act_max, argmax, dist, act


def proto_bwd(tokens, t0, T, protos, dist, g_full, g_max, argmax, dtok, dprotos, act_kind=0, eps=1e-4, rows=None, from_act=False):
    """Backward of proto_fwd.  g_full [B,P,T] is the dense gradient of the activation maps; rows = (g_rows [B,ppc,T], label int64 [B], ppc)
    gives the same gradient in the block form of the PPC loss instead (ppf_proto_bwd_rows: nothing of shape (B,P,T) is touched).
    from_act: `dist` is the activation map act_full of the forward (the derivative is taken from it; T > 1 only)."""
    B, Ttot, Dp = tokens.shape
    P = protos.shape[0]
    if T == 1 and from_act:
        raise ValueError("proto_bwd: from_act applies to the pooled branch (T > 1)")
    if T == 1 and (g_full is None) != (g_max is None):
        # one token per sample: every (sample, prototype) pair carries a gradient -> two dense fp32 products instead of the gather
        ws = _workspace(tokens.device, _lib.lib().ppf_proto_bwd_single_workspace(B, P, Dp))
        _lib.call("ppf_proto_bwd_single", tokens, Ttot * Dp, t0, protos, B, P, Dp, act_kind, float(eps), dist, g_max if g_max is not None else g_full,
                  dtok, Ttot * Dp, dprotos, ws, ws.numel())
        return
    # the zeroed bitmap of the token gradients, then the scratch of the tiled prototype gradients: the two sizes add up
    bitmap = _lib.lib().ppf_proto_bwd_workspace(B, T, P, Dp, 1, 0) if dtok is not None else 0
    need = bitmap + (_lib.lib().ppf_proto_bwd_workspace(B, T, P, Dp, 0, 1) if dprotos is not None else 0)
    if dtok is not None:
        ws = torch.empty(need, dtype=torch.uint8, device=tokens.device)
        _lib.call("ppf_memset_zero", ws, bitmap)                  # the scratch behind the bitmap is write-first
    else:
        ws = _workspace(tokens.device, need) if need else None    # prototype gradients only: per-stream scratch, any content
    if rows is not None:
        if g_full is not None:
            raise ValueError("proto_bwd: pass the activation-map gradient either dense (g_full) or in block form (rows), not both")
        g_rows, label, ppc = rows
        _lib.call("ppf_proto_bwd_rows", tokens, Ttot * Dp, t0, T, protos, B, P, Dp, act_kind, float(eps), dist, int(from_act), g_rows, label, int(ppc), g_max,
                  argmax, dtok, Ttot * Dp, dprotos, ws, need)
        return
    _lib.call("ppf_proto_bwd", tokens, Ttot * Dp, t0, T, protos, B, P, Dp, act_kind, float(eps), dist, int(from_act), g_full, g_max, argmax, dtok,
              Ttot * Dp, dprotos, ws, need)


def ppc_loss(act, idx, label, ppc, side, cov_thresh, mean_thresh):
    """act [B,P,T] fp32, idx [B,T] int32, label [B] int64 -> (loss[2] = (cov, mean), gcov, gmean [B,ppc,T])."""
    B, P, T = act.shape
    dev = act.device
    partial = torch.empty((B, 2), dtype=torch.float32, device=dev)
    gcov = torch.empty((B, ppc, T), dtype=torch.float32, device=dev)
    gmean = torch.empty((B, ppc, T), dtype=torch.float32, device=dev)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    _lib.call("ppf_ppc_loss", act, idx, label, B, P, T, ppc, side, float(cov_thresh), float(mean_thresh), partial, gcov, gmean, loss)
    return loss, gcov, gmean


def ppc_loss_bwd_rows(gcov, gmean, up_cov, up_mean):
    """up_cov * gcov + up_mean * gmean as [B, ppc, T]: the PPC gradient in block form (row k of sample b belongs to prototype label[b]*ppc + k)."""
    B, ppc, T = gcov.shape
    rows = torch.empty_like(gcov)
    _lib.call("ppf_ppc_loss_bwd", gcov, gmean, up_cov, up_mean, _zero_labels(gcov.device, B), rows, B, ppc, T, ppc)
    return rows


_ZERO_LABELS = {}


def _zero_labels(device, B):
    t = _ZERO_LABELS.get(device)
    if t is None or t.numel() < B:
        t = zeros((max(B, 1024),), torch.int64, device)
        _ZERO_LABELS[device] = t
    return t


def ppc_loss_bwd(gcov, gmean, up_cov, up_mean, label, P):
    B, ppc, T = gcov.shape
    g_full = zeros((B, P, T), torch.float32, gcov.device)
    _lib.call("ppf_ppc_loss_bwd", gcov, gmean, up_cov, up_mean, label, g_full, B, P, T, ppc)
    return g_full


def cross_entropy(logits, label):
    B, C = logits.shape
    per = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    _lib.call("ppf_cross_entropy", logits, label, per, dlogits, loss, B, C)
    return loss, dlogits


def soft_cross_entropy(logits, target=None, label=None, smoothing=0.0):
    """Mean cross-entropy against a dense target [B, C] fp32 or against int64 labels with label smoothing -> (loss[1], dlogits)."""
    B, C = logits.shape
    per = torch.empty(B, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    _lib.call("ppf_soft_cross_entropy", logits, target, label, float(smoothing), per, dlogits, loss, B, C)
    return loss, dlogits


EVAL_SLOTS = 8                       # acc of ppf_eval_metrics: n, ce sum, top-1, top-5, global top-1, local top-1, bad labels, reserved


def eval_metrics(acc, logits, label, logits_global=None, logits_local=None):
    """Add one batch's evaluation metrics into acc (device float64[8], include/ppf_hip.h); launches only, nothing is read back."""
    if acc.dtype != torch.float64 or acc.numel() != EVAL_SLOTS or not acc.is_contiguous() or not acc.is_cuda:
        raise ValueError("eval_metrics: acc must be a contiguous float64[8] device tensor")
    if logits.dim() != 2 or label.dim() != 1 or label.shape[0] != logits.shape[0] or label.dtype != torch.int64:
        raise ValueError(f"eval_metrics: logits [B, C] and int64 labels [B] expected, got {tuple(logits.shape)} and {tuple(label.shape)} {label.dtype}")
    B, C = logits.shape
    rows = []
    for t in (logits, logits_global, logits_local):
        if t is not None:
            if t.shape != logits.shape or t.dtype != torch.float32 or t.device != acc.device:
                raise ValueError(f"eval_metrics: fp32 [B, C] logits on {acc.device} expected, got {tuple(t.shape)} {t.dtype} on {t.device}")
            t = t.contiguous()
        rows.append(t)
    _lib.call("ppf_eval_metrics", rows[0], rows[1], rows[2], label.contiguous(), acc, B, C)


def proto_topk_init(val, img, pos):
    """Empty per-prototype lists: val [P, K] fp32 = -inf, img / pos [P, K] int32 = -1."""
    _chk(val, torch.float32), _chk(img, torch.int32), _chk(pos, torch.int32)
    P, K = val.shape
    if img.shape != val.shape or pos.shape != val.shape:
        raise ValueError("proto_topk_init: val, img and pos must share the shape [P, K]")
    _lib.call("ppf_proto_topk_init", val, img, pos, P, K)


def proto_topk_merge(act_max, argmax, idx, tokens, t0, label, image_id, ppc, val, img, pos, best_feat):
    """Merge one batch into the running per-prototype top-K lists (ppf_proto_topk_merge, include/ppf_hip.h); launches only.
    act_max [B, P] fp32 and argmax [B, P] int32 as proto_fwd returns them (argmax None: global branch, then idx None too);
    idx [B, k] int32; tokens fp32 [B, Ttot, Dp], the candidate's token is tokens[b, t0 + argmax[b, p]]; label int64 [B] (None with
    ppc == 0), image_id int32 [B]; val / img / pos [P, K] and best_feat [P, Dp] are updated in place."""
    _chk(act_max, torch.float32), _chk(tokens, torch.float32), _chk(image_id, torch.int32)
    _chk(val, torch.float32), _chk(img, torch.int32), _chk(pos, torch.int32), _chk(best_feat, torch.float32)
    B, P = act_max.shape
    K = val.shape[1]
    _, Ttot, Dp = tokens.shape
    if (argmax is None) != (idx is None):
        raise ValueError("proto_topk_merge: argmax and idx come together (both None on the global branch)")
    k = 0
    if argmax is not None:
        _chk(argmax, torch.int32), _chk(idx, torch.int32)
        k = idx.shape[1]
        if argmax.shape != act_max.shape or idx.shape[0] != B or t0 + k > Ttot:
            raise ValueError(f"proto_topk_merge: argmax {tuple(argmax.shape)} / idx {tuple(idx.shape)} do not fit act_max {tuple(act_max.shape)} "
                             f"and {Ttot} tokens from t0={t0}")
    if tokens.shape[0] != B or image_id.shape != (B,) or t0 >= Ttot:
        raise ValueError(f"proto_topk_merge: tokens {tuple(tokens.shape)} / image_id {tuple(image_id.shape)} do not fit a batch of {B}")
    if val.shape != (P, K) or img.shape != (P, K) or pos.shape != (P, K) or best_feat.shape != (P, Dp):
        raise ValueError(f"proto_topk_merge: the state must be val / img / pos [{P}, K] and best_feat [{P}, {Dp}]")
    if ppc > 0:
        if label is None or label.dtype != torch.int64 or label.shape != (B,):
            raise ValueError("proto_topk_merge: class-specific mode needs int64 labels [B]")
        _chk(label)
    _lib.call("ppf_proto_topk_merge", act_max, argmax, idx, k, tokens, Ttot * Dp, t0, Dp, label if ppc > 0 else None, image_id, int(ppc), B, P, K,
              val, img, pos, best_feat)


def proto_stats_update(act_max, argmax, idx, label, ppc, lo, inv_width, hist, nan_count, coloc, images, bad):
    """Add one batch into the int32 prototype statistics hist [P, 2, NB], nan_count [P, 2], coloc [P, ppc] (None on the global branch),
    images [P // ppc], bad [1] (ppf_proto_stats_update, include/ppf_hip.h); launches only.  act_max [B, P] fp32 and argmax [B, P] int32 as
    proto_fwd returns them (argmax None: global branch, then idx None too and coloc is not touched); idx [B, T] int32; label int64 [B];
    lo and inv_width = fl(NB / fl(hi - lo)) as fp32 values.  The limits on B, ppc, NB, lo and inv_width are the entry point's."""
    _chk(act_max, torch.float32)
    if act_max.dim() != 2 or hist.dim() != 3:
        raise ValueError(f"proto_stats_update: act_max [B, P] and hist [P, 2, NB] expected, got {tuple(act_max.shape)} and {tuple(hist.shape)}")
    (B, P), NB, dev, ppc = act_max.shape, hist.shape[2], act_max.device, int(ppc)
    if (argmax is None) != (idx is None):
        raise ValueError("proto_stats_update: argmax and idx come together (both None on the global branch)")
    T = 0
    if argmax is not None:
        _chk(argmax, torch.int32), _chk(idx, torch.int32)
        T = idx.shape[1] if idx.dim() == 2 else -1
        if argmax.shape != act_max.shape or idx.shape != (B, T) or coloc is None:
            raise ValueError(f"proto_stats_update: argmax {tuple(argmax.shape)} / idx {tuple(idx.shape)} do not fit act_max {tuple(act_max.shape)}, "
                             "or the local branch came without coloc")
    if label.dtype != torch.int64 or label.shape != (B,) or not label.is_contiguous() or label.device != dev:
        raise ValueError(f"proto_stats_update: label must be a contiguous int64 tensor [{B}] on {dev}")
    tables = [("hist", hist, (P, 2, NB)), ("nan_count", nan_count, (P, 2)), ("bad", bad, (1,))]
    if ppc >= 1 and P % ppc == 0:                          # (a ppc the entry point refuses is left for it to name)
        tables += [("images", images, (P // ppc,))] + ([("coloc", coloc, (P, ppc))] if coloc is not None else [])
    for name, t, shape in tables:
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"proto_stats_update: {name} must be a contiguous int32 tensor {shape} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    _lib.call("ppf_proto_stats_update", act_max, argmax, idx, T, label, ppc, B, P, NB, float(lo), float(inv_width), hist, nan_count, coloc, images, bad)


def explain_topk(act_max, weight, scale, ppc, logits, K, *, classes=None, top_classes=1, sign=1, argmax=None, idx=None, act_full=None,
                 grid_cells=0, want_maps=False):
    """The K strongest class evidences per (sample, class) of one branch (ppf_explain_topk, include/ppf_hip.h); one launch.
    act_max [B, P] fp32 and argmax [B, P] int32 as proto_fwd returns them (argmax None: global branch, then idx / act_full None and no
    maps); idx [B, T] int32; act_full fp32 with B * P * T elements; weight [C, P] fp32; logits [B, C] fp32; classes int32 [B, M] on the
    device, or None: the kernel picks the top `top_classes` of logits.  Returns dict(classes, class_logits [B, M], prototypes,
    contributions, activations, cells [B, M, K], evidence [B, M, 2], maps [B, M, K, grid_cells] or None)."""
    _chk(act_max, torch.float32), _chk(weight, torch.float32), _chk(logits, torch.float32)
    B, P = act_max.shape
    C = weight.shape[0]
    if weight.shape != (C, P) or logits.shape != (B, C):
        raise ValueError(f"explain_topk: weight {tuple(weight.shape)} / logits {tuple(logits.shape)} do not fit act_max {tuple(act_max.shape)}")
    if (argmax is None) != (idx is None):
        raise ValueError("explain_topk: argmax and idx come together (both None on the global branch)")
    if want_maps and (argmax is None or act_full is None):
        raise ValueError("explain_topk: maps need the local branch's argmax, idx and act_full")
    T = 0
    if argmax is not None:
        _chk(argmax, torch.int32), _chk(idx, torch.int32)
        T = idx.shape[1] if idx.dim() == 2 else -1
        if argmax.shape != act_max.shape or idx.shape != (B, T):
            raise ValueError(f"explain_topk: argmax {tuple(argmax.shape)} / idx {tuple(idx.shape)} do not fit act_max {tuple(act_max.shape)}")
    if act_full is not None:
        _chk(act_full, torch.float32)
        if argmax is None or act_full.numel() != B * P * T:
            raise ValueError(f"explain_topk: act_full {tuple(act_full.shape)} is not [{B}, {P}, {T}] of the local branch")
    if classes is not None:
        _chk(classes, torch.int32)
        if classes.dim() != 2 or classes.shape[0] != B:
            raise ValueError(f"explain_topk: classes must be int32 [{B}, M], got {tuple(classes.shape)}")
        M = classes.shape[1]
    else:
        M = int(top_classes)
    K, G, dev = int(K), int(grid_cells), act_max.device
    shape = (B, max(M, 0), max(K, 0))
    out = dict(classes=torch.empty(shape[:2], dtype=torch.int32, device=dev), class_logits=torch.empty(shape[:2], dtype=torch.float32, device=dev),
               prototypes=torch.empty(shape, dtype=torch.int32, device=dev), contributions=torch.empty(shape, dtype=torch.float32, device=dev),
               activations=torch.empty(shape, dtype=torch.float32, device=dev), cells=torch.empty(shape, dtype=torch.int32, device=dev),
               evidence=torch.empty(shape[:2] + (2,), dtype=torch.float32, device=dev),
               maps=torch.empty(shape + (max(G, 0),), dtype=torch.float32, device=dev) if want_maps else None)
    _lib.call("ppf_explain_topk", act_max, argmax, idx, T, act_full, weight, float(scale), int(ppc), logits, classes, int(sign), B, P, C, M, K, G,
              out["classes"], out["class_logits"], out["prototypes"], out["contributions"], out["activations"], out["cells"], out["evidence"],
              out["maps"])
    return out


# ---- faithfulness of an explanation (csrc/faithful.hip): cell order, perturbed images, class probability
ORDER_MODES = {"evidence": 0, "attention": 1, "random": 2}


def _dev_tensor(who, name, t, dtype, shape, device=None):
    """Refuses what the C side cannot see -- device, dtype, layout, shape -- before the call."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device):
        raise ValueError(f"{who}: {name} must be a CUDA tensor" + (f" on {device}" if device is not None else ""))
    if t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {name} must be {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be contiguous, got strides {tuple(t.stride())}")
    return t


def cell_order(classes, grid_cells, mode="evidence", *, act_full=None, idx=None, token_attn=None, weight=None, scale=1.0, image_ids=None, seed=0):
    """A total order of the grid cells per (sample, class) row (ppf_cell_order, include/ppf_hip.h); one launch.  classes int32 [B, M];
    evidence: act_full fp32 [B, P, T], idx int32 [B, T], token_attn fp32 [B, G], weight fp32 [C, P]; attention: token_attn (and weight
    or nothing: the class count only decides which classes are valid); random: image_ids int64 [B].  Returns (order, rank int32 [B, M, G],
    score fp32 [B, M, G])."""
    who = "cell_order"
    if mode not in ORDER_MODES:
        raise ValueError(f"{who}: mode must be one of {sorted(ORDER_MODES)}, got {mode!r}")
    if not isinstance(classes, torch.Tensor) or classes.dim() != 2:
        raise ValueError(f"{who}: classes must be an int32 CUDA tensor [B, M]")
    B, M = classes.shape
    dev, G = classes.device, int(grid_cells)
    _dev_tensor(who, "classes", classes, torch.int32, (B, M))
    P = T = 0
    C = 1 << 30                                  # without a weight every non-negative class is valid
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
            raise ValueError(f"{who}: weight must be an fp32 CUDA tensor [C, P]")
        C, P = weight.shape
        _dev_tensor(who, "weight", weight, torch.float32, (C, P), dev)
    if mode == "evidence":
        if weight is None or act_full is None or idx is None or token_attn is None:
            raise ValueError(f"{who}: the evidence order needs act_full, idx, token_attn and weight")
        T = idx.shape[1] if isinstance(idx, torch.Tensor) and idx.dim() == 2 else -1
        _dev_tensor(who, "idx", idx, torch.int32, (B, T), dev)
        if not isinstance(act_full, torch.Tensor) or act_full.numel() != B * P * T:
            raise ValueError(f"{who}: act_full must hold [{B}, {P}, {T}] elements")
        _dev_tensor(who, "act_full", act_full, torch.float32, act_full.shape, dev)
    else:
        act_full = idx = None
    if mode == "random":
        if image_ids is None:
            raise ValueError(f"{who}: the random order needs image_ids")
        _dev_tensor(who, "image_ids", image_ids, torch.int64, (B,), dev)
        token_attn = None
    else:
        if token_attn is None:
            raise ValueError(f"{who}: the {mode} order needs token_attn")
        _dev_tensor(who, "token_attn", token_attn, torch.float32, (B, G), dev)
        image_ids = None
    order = torch.empty((B, M, max(G, 0)), dtype=torch.int32, device=dev)
    rank, score = torch.empty_like(order), torch.empty(order.shape, dtype=torch.float32, device=dev)
    _lib.call("ppf_cell_order", act_full, idx, token_attn, weight if mode == "evidence" else None, float(scale), classes, image_ids,
              int(seed) & 0xFFFFFFFFFFFFFFFF, ORDER_MODES[mode], B, P, C, T, G, M, order, rank, score)
    return order, rank, score


def patch_perturb(x, rank, counts, insertion=False, baseline=0.0, out=None):
    """The perturbed images out fp32 [S, B, M, Cc, H, W] of x fp32 [B, Cc, H, W] for rank int32 [B, M, G] and counts int32 [S] on the device
    (ppf_patch_perturb, include/ppf_hip.h); one launch.  baseline: a number, or an fp32 tensor like x."""
    who = "patch_perturb"
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [B, Cc, H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    B, Cc, H, W = x.shape
    if not isinstance(rank, torch.Tensor) or rank.dim() != 3 or rank.shape[0] != B:
        raise ValueError(f"{who}: rank must be an int32 CUDA tensor [{B}, M, G]")
    _dev_tensor(who, "rank", rank, torch.int32, rank.shape, x.device)
    M, G = rank.shape[1:]
    if not isinstance(counts, torch.Tensor) or counts.dim() != 1:
        raise ValueError(f"{who}: counts must be an int32 CUDA tensor [S]")
    _dev_tensor(who, "counts", counts, torch.int32, counts.shape, x.device)
    S = counts.shape[0]
    base_t, base_c = None, 0.0
    if isinstance(baseline, torch.Tensor):
        base_t = _dev_tensor(who, "baseline", baseline, torch.float32, x.shape, x.device)
    else:
        base_c = float(baseline)
    shape = (S, B, M, Cc, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_tensor(who, "out", out, torch.float32, shape, x.device)
    _lib.call("ppf_patch_perturb", x, rank, counts, S, 1 if insertion else 0, base_t, base_c, B, M, Cc, H, W, G, out)
    return out


def class_prob(logits, cls):
    """prob fp32 [R] = softmax(logits[r])[cls[r]] of logits fp32 [R, C], cls int32 [R] (ppf_class_prob); one launch, no softmax rows."""
    who = "class_prob"
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"{who}: logits must be an fp32 CUDA tensor [R, C]")
    _dev_tensor(who, "logits", logits, torch.float32, logits.shape)
    R, C = logits.shape
    _dev_tensor(who, "cls", cls, torch.int32, (R,), logits.device)
    prob = torch.empty(R, dtype=torch.float32, device=logits.device)
    _lib.call("ppf_class_prob", logits, cls, R, C, prob)
    return prob


# ---- the same curves per pixel (csrc/pixel_faithful.hip): pixel order, random pixel scores, perturbed images, Gaussian blur
def pixel_order(score, classes):
    """rank int32 [R, n]: the number of pixels of row r that come before pixel i, larger score first, ties by the smaller pixel, NaN lowest,
    -0 == +0; a row with classes[r] < 0 is all -1 (ppf_pixel_order, include/ppf_hip.h); one launch.  score fp32 [R, n], classes int32 [R];
    the sort's ping-pong buffers come from the stream's workspace."""
    who = "pixel_order"
    if not isinstance(score, torch.Tensor) or score.dim() != 2:
        raise ValueError(f"{who}: score must be an fp32 CUDA tensor [R, n]")
    _dev_tensor(who, "score", score, torch.float32, score.shape)
    R, n = score.shape
    _dev_tensor(who, "classes", classes, torch.int32, (R,), score.device)
    rank = torch.empty((R, n), dtype=torch.int32, device=score.device)
    nbytes = _lib.lib().ppf_pixel_order_scratch_bytes(R, n)
    ws = _workspace(score.device, max(nbytes, 16))
    _lib.call("ppf_pixel_order", score, classes, R, n, rank, ws, ws.numel())
    return rank


def pixel_random(image_ids, pixels, seed=0):
    """score fp32 [B, pixels]: the Philox draw of (seed, image id, pixel) in [0, 1) (ppf_pixel_random); image_ids int64 [B]."""
    who = "pixel_random"
    if not isinstance(image_ids, torch.Tensor) or image_ids.dim() != 1:
        raise ValueError(f"{who}: image_ids must be an int64 CUDA tensor [B]")
    _dev_tensor(who, "image_ids", image_ids, torch.int64, image_ids.shape)
    B, n = image_ids.shape[0], int(pixels)
    score = torch.empty((B, max(n, 0)), dtype=torch.float32, device=image_ids.device)
    _lib.call("ppf_pixel_random", image_ids, int(seed) & 0xFFFFFFFFFFFFFFFF, B, n, score)
    return score


def pixel_perturb(x, rank, counts, insertion=False, baseline=0.0, out=None):
    """The perturbed images out fp32 [S, B, M, Cc, H, W] of x fp32 [B, Cc, H, W] for rank int32 [B, M, H * W] and counts int32 [S] on the
    device (ppf_pixel_perturb, include/ppf_hip.h); one launch.  baseline: a number, or an fp32 tensor like x."""
    who = "pixel_perturb"
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [B, Cc, H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    B, Cc, H, W = x.shape
    if not isinstance(rank, torch.Tensor) or rank.dim() != 3 or rank.shape[0] != B or rank.shape[2] != H * W:
        raise ValueError(f"{who}: rank must be an int32 CUDA tensor [{B}, M, {H * W}]")
    _dev_tensor(who, "rank", rank, torch.int32, rank.shape, x.device)
    M = rank.shape[1]
    if not isinstance(counts, torch.Tensor) or counts.dim() != 1:
        raise ValueError(f"{who}: counts must be an int32 CUDA tensor [S]")
    _dev_tensor(who, "counts", counts, torch.int32, counts.shape, x.device)
    S = counts.shape[0]
    base_t, base_c = None, 0.0
    if isinstance(baseline, torch.Tensor):
        base_t = _dev_tensor(who, "baseline", baseline, torch.float32, x.shape, x.device)
    else:
        base_c = float(baseline)
    shape = (S, B, M, Cc, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_tensor(who, "out", out, torch.float32, shape, x.device)
    _lib.call("ppf_pixel_perturb", x, rank, counts, S, 1 if insertion else 0, base_t, base_c, B, M, Cc, H, W, out)
    return out


def gauss_blur(x, taps):
    """out like x fp32 [..., H, W]: every plane blurred separably with taps fp32 [2r + 1] (a CUDA tensor) and a zero border
    (ppf_gauss_blur, include/ppf_hip.h); one launch."""
    who = "gauss_blur"
    if not isinstance(x, torch.Tensor) or x.dim() < 2:
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [..., H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    if not isinstance(taps, torch.Tensor) or taps.dim() != 1 or taps.shape[0] % 2 != 1:
        raise ValueError(f"{who}: taps must be an fp32 CUDA tensor [2r + 1]")
    _dev_tensor(who, "taps", taps, torch.float32, taps.shape, x.device)
    H, W = x.shape[-2:]
    out = torch.empty_like(x)
    _lib.call("ppf_gauss_blur", x, taps, (taps.shape[0] - 1) // 2, x.numel() // max(H * W, 1), H, W, out)
    return out


# ---- RISE saliency (csrc/rise.hip): node tables, masked images, the probability-weighted mean mask
def _rise_tables(who, nodes, shift, cells):
    LL = (int(cells) + 2) ** 2
    if not isinstance(nodes, torch.Tensor) or nodes.dim() != 3:
        raise ValueError(f"{who}: nodes must be a uint8 CUDA tensor [B, N, {LL}]")
    B, N = nodes.shape[:2]
    _dev_tensor(who, "nodes", nodes, torch.uint8, (B, N, LL))
    _dev_tensor(who, "shift", shift, torch.int32, (B, N, 2), nodes.device)
    return B, N


def rise_nodes(image_ids, size, masks, cells, thr, seed=0):
    """The node tables of `masks` RISE masks per image (ppf_rise_nodes, include/ppf_hip.h); one launch.  image_ids int64 [B]; size = H;
    thr = round(p * 2^24).  Returns (nodes uint8 [B, N, (cells + 2)^2], shift int32 [B, N, 2])."""
    who = "rise_nodes"
    if not isinstance(image_ids, torch.Tensor) or image_ids.dim() != 1:
        raise ValueError(f"{who}: image_ids must be an int64 CUDA tensor [B]")
    B, N, s = image_ids.shape[0], int(masks), int(cells)
    _dev_tensor(who, "image_ids", image_ids, torch.int64, (B,))
    nodes = torch.empty((B, max(N, 0), max(s + 2, 0) ** 2), dtype=torch.uint8, device=image_ids.device)
    shift = torch.empty((B, max(N, 0), 2), dtype=torch.int32, device=image_ids.device)
    _lib.call("ppf_rise_nodes", image_ids, int(seed) & 0xFFFFFFFFFFFFFFFF, int(thr), B, N, s, int(size), nodes, shift)
    return nodes, shift


def rise_apply(x, nodes, shift, cells, n0=0, count=None, baseline=0.0, out=None):
    """The masked images out fp32 [Nc, B, Cc, H, W] of x fp32 [B, Cc, H, W] under masks n0 .. n0 + count - 1 (default: to the last) of the
    tables rise_nodes wrote (ppf_rise_apply, include/ppf_hip.h); one launch.  baseline: a number, or an fp32 tensor like x."""
    who = "rise_apply"
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [B, Cc, H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    B, Cc, H, W = x.shape
    Bn, N = _rise_tables(who, nodes, shift, cells)
    if Bn != B or nodes.device != x.device:
        raise ValueError(f"{who}: nodes must be [{B}, N, L*L] on {x.device}, got {list(nodes.shape)} on {nodes.device}")
    n0 = int(n0)
    Nc = N - n0 if count is None else int(count)
    base_t, base_c = None, 0.0
    if isinstance(baseline, torch.Tensor):
        base_t = _dev_tensor(who, "baseline", baseline, torch.float32, x.shape, x.device)
    else:
        base_c = float(baseline)
    shape = (max(Nc, 0), B, Cc, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_tensor(who, "out", out, torch.float32, shape, x.device)
    _lib.call("ppf_rise_apply", x, nodes, shift, N, n0, Nc, int(cells), base_t, base_c, B, Cc, H, W, out)
    return out


def rise_accumulate(nodes, shift, prob, size, cells, grid_cells, thr):
    """(sal fp32 [B, M, H, H], cell fp32 [B, M, G]) = the probability-weighted mean mask per pixel and per grid cell, from the tables
    rise_nodes wrote and prob fp32 [N, B, M] (ppf_rise_accumulate, include/ppf_hip.h); masks regenerated, never stored."""
    who = "rise_accumulate"
    B, N = _rise_tables(who, nodes, shift, cells)
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3:
        raise ValueError(f"{who}: prob must be an fp32 CUDA tensor [N, B, M]")
    M, H, G = prob.shape[2], int(size), int(grid_cells)
    _dev_tensor(who, "prob", prob, torch.float32, (N, B, M), nodes.device)
    sal = torch.empty((B, M, max(H, 0), max(H, 0)), dtype=torch.float32, device=nodes.device)
    cell = torch.empty((B, M, max(G, 0)), dtype=torch.float32, device=nodes.device)
    _lib.call("ppf_rise_accumulate", nodes, shift, prob, B, N, M, int(cells), int(thr), H, H, G, sal, cell)
    return sal, cell


# ---- KernelSHAP cell attributions (csrc/shap.hip): coalitions, masked images, Gram sums, the constrained least-squares solve
def _shap_coal(who, coal, cells):
    """(B, N) of coal int32 [B, N, ceil(cells^2 / 32)]: the uint32 words of ppf_shap_coalitions, held as int32 (the same bits)."""
    Wd = (int(cells) ** 2 + 31) // 32
    if not isinstance(coal, torch.Tensor) or coal.dim() != 3:
        raise ValueError(f"{who}: coal must be an int32 CUDA tensor [B, N, {Wd}]")
    B, N = coal.shape[:2]
    _dev_tensor(who, "coal", coal, torch.int32, (B, N, Wd))
    return B, N


def shap_coalitions(image_ids, cells, samples, table, seed=0):
    """coal int32 [B, N, ceil(d / 32)], the membership bits of `samples` coalitions per image (ppf_shap_coalitions, include/ppf_hip.h); one
    launch.  image_ids int64 [B]; table: the size table, d - 1 integers on the host (interpret.shap_size_table), refused here when it is
    not non-decreasing or does not end at 2^24."""
    import numpy as np
    who = "shap_coalitions"
    if not isinstance(image_ids, torch.Tensor) or image_ids.dim() != 1:
        raise ValueError(f"{who}: image_ids must be an int64 CUDA tensor [B]")
    B, N, s = image_ids.shape[0], int(samples), int(cells)
    _dev_tensor(who, "image_ids", image_ids, torch.int64, (B,))
    d = s * s
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.shape != (max(d - 1, 0),) or t.size == 0 or (np.diff(t.astype(np.int64)) < 0).any() or int(t[-1]) != 1 << 24:
        raise ValueError(f"{who}: table must hold {d - 1} non-decreasing integers that end at 2^24")
    table_d = torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(image_ids.device)
    coal = torch.empty((B, max(N, 0), (d + 31) // 32), dtype=torch.int32, device=image_ids.device)
    _lib.call("ppf_shap_coalitions", image_ids, int(seed) & 0xFFFFFFFFFFFFFFFF, table_d, B, N, s, coal)
    return coal


def shap_apply(x, coal, cells, n0=0, count=None, baseline=0.0, out=None):
    """The masked images out fp32 [Nc, B, Cc, H, W] of x fp32 [B, Cc, H, W] under the coalitions n0 .. n0 + count - 1 (default: to the last)
    of coal (ppf_shap_apply, include/ppf_hip.h); one launch.  baseline: a number, or an fp32 tensor like x."""
    who = "shap_apply"
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [B, Cc, H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    B, Cc, H, W = x.shape
    Bn, N = _shap_coal(who, coal, cells)
    if Bn != B or coal.device != x.device:
        raise ValueError(f"{who}: coal must be [{B}, N, Wd] on {x.device}, got {list(coal.shape)} on {coal.device}")
    n0 = int(n0)
    Nc = N - n0 if count is None else int(count)
    base_t, base_c = None, 0.0
    if isinstance(baseline, torch.Tensor):
        base_t = _dev_tensor(who, "baseline", baseline, torch.float32, x.shape, x.device)
    else:
        base_c = float(baseline)
    shape = (max(Nc, 0), B, Cc, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        _dev_tensor(who, "out", out, torch.float32, shape, x.device)
    _lib.call("ppf_shap_apply", x, coal, N, n0, Nc, int(cells), base_t, base_c, B, Cc, H, W, out)
    return out


def shap_gram(coal, val, v0, cells):
    """(A int32 [B, d, d], bvec fp64 [B, M, d]) from coal, val fp32 [N, B, M] and v0 fp32 [B, M] (ppf_shap_gram, include/ppf_hip.h); one
    launch, integer adds and an ascending fp64 sum."""
    who = "shap_gram"
    B, N = _shap_coal(who, coal, cells)
    if not isinstance(val, torch.Tensor) or val.dim() != 3:
        raise ValueError(f"{who}: val must be an fp32 CUDA tensor [N, B, M]")
    M, d = val.shape[2], int(cells) ** 2
    _dev_tensor(who, "val", val, torch.float32, (N, B, M), coal.device)
    _dev_tensor(who, "v0", v0, torch.float32, (B, M), coal.device)
    A = torch.empty((B, d, d), dtype=torch.int32, device=coal.device)
    bvec = torch.empty((B, M, d), dtype=torch.float64, device=coal.device)
    _lib.call("ppf_shap_gram", coal, val, v0, B, N, M, int(cells), A, bvec)
    return A, bvec


def shap_solve(A, bvec, v0, v1, cells, grid_cells):
    """(phi fp64 [B, M, d], cell fp32 [B, M, G], bad int32 [B]) from the Gram matrix A int32 [B, d, d], bvec fp64 [B, M, d] and the values
    v0, v1 fp32 [B, M] of the all-baseline and the whole image (ppf_shap_solve, include/ppf_hip.h); one launch, the factor in the stream's
    workspace."""
    who = "shap_solve"
    s, G = int(cells), int(grid_cells)
    d = s * s
    if not isinstance(A, torch.Tensor) or A.dim() != 3:
        raise ValueError(f"{who}: A must be an int32 CUDA tensor [B, {d}, {d}]")
    B = A.shape[0]
    _dev_tensor(who, "A", A, torch.int32, (B, d, d))
    if not isinstance(bvec, torch.Tensor) or bvec.dim() != 3:
        raise ValueError(f"{who}: bvec must be an fp64 CUDA tensor [{B}, M, {d}]")
    M = bvec.shape[1]
    _dev_tensor(who, "bvec", bvec, torch.float64, (B, M, d), A.device)
    _dev_tensor(who, "v0", v0, torch.float32, (B, M), A.device)
    _dev_tensor(who, "v1", v1, torch.float32, (B, M), A.device)
    phi = torch.empty((B, M, d), dtype=torch.float64, device=A.device)
    cell = torch.empty((B, M, max(G, 0)), dtype=torch.float32, device=A.device)
    bad = torch.empty((B,), dtype=torch.int32, device=A.device)
    ws = _workspace(A.device, max(_lib.lib().ppf_shap_solve_scratch_bytes(B, d), 16))
    _lib.call("ppf_shap_solve", A, bvec, v0, v1, B, M, s, G, ws, ws.numel(), phi, cell, bad)
    return phi, cell, bad


# ---- "this looks like that, because" (csrc/because.hip): colour transform, bilateral filter, warp, and the score of a perturbed forward
def _host_f32(who, name, a, n):
    """A host table as a contiguous fp32 numpy array of n entries: the C side takes its address."""
    import numpy as np
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError(f"{who}: {name} must hold {n} values, got {a.size}")
    return a


def _image_batch(who, x, out, channels=3):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or (channels is not None and x.shape[1] != channels):
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor [B, {channels or 'Cc'}, H, W]")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    if out is None:
        return torch.empty_like(x)
    return _dev_tensor(who, "out", out, torch.float32, x.shape, x.device)


def color_affine(x, matrix, mean, std, offset=None, out=None):
    """out = the 3 x 3 colour transform `matrix` (host) of the de-normalised, clamped pixels of x fp32 [B, 3, H, W], plus the optional
    per-image offset fp32 [B, 3] on the device, clamped and normalised again (ppf_color_affine, include/ppf_hip.h); one launch."""
    who = "color_affine"
    out = _image_batch(who, x, out)
    B, _, H, W = x.shape
    m, mean, std = _host_f32(who, "matrix", matrix, 9), _host_f32(who, "mean", mean, 3), _host_f32(who, "std", std, 3)
    if offset is not None:
        _dev_tensor(who, "offset", offset, torch.float32, (B, 3), x.device)
    _lib.call("ppf_color_affine", x, m.ctypes.data, offset, mean.ctypes.data, std.ctypes.data, B, H, W, out)
    return out


def gray_sum(x, mean, std):
    """int32 [B]: the integer sum of the 8-bit luma over each image of x fp32 [B, 3, H, W] (ppf_gray_sum); a memset and one launch."""
    who = "gray_sum"
    _image_batch(who, x, x)
    B, _, H, W = x.shape
    mean, std = _host_f32(who, "mean", mean, 3), _host_f32(who, "std", std, 3)
    total = torch.empty(B, dtype=torch.int32, device=x.device)
    _lib.call("ppf_gray_sum", x, mean.ctypes.data, std.ctypes.data, B, H, W, total)
    return total


def contrast_offset(total, size, one_minus_f):
    """fp32 [B, 3]: (1 - f) * the mean luma of each image from gray_sum's int32 [B] (ppf_contrast_offset); one launch, no host read.
    size = (H, W)."""
    who = "contrast_offset"
    if not isinstance(total, torch.Tensor) or total.dim() != 1:
        raise ValueError(f"{who}: total must be an int32 CUDA tensor [B]")
    _dev_tensor(who, "total", total, torch.int32, total.shape)
    off = torch.empty((total.shape[0], 3), dtype=torch.float32, device=total.device)
    _lib.call("ppf_contrast_offset", total, total.shape[0], int(size[0]), int(size[1]), float(one_minus_f), off)
    return off


def bilateral(x, ws, wr, radius, mean, std, out=None):
    """out = the joint bilateral filter of x fp32 [B, 3, H, W] with the host tables ws [(2r + 1)^2] (spatial) and wr [256] (range over the
    8-bit luma difference) (ppf_bilateral, include/ppf_hip.h); one launch."""
    who = "bilateral"
    out = _image_batch(who, x, out)
    B, _, H, W = x.shape
    r = int(radius)
    ws, wr = _host_f32(who, "ws", ws, max(2 * r + 1, 1) ** 2), _host_f32(who, "wr", wr, 256)
    mean, std = _host_f32(who, "mean", mean, 3), _host_f32(who, "std", std, 3)
    _lib.call("ppf_bilateral", x, ws.ctypes.data, wr.ctypes.data, r, mean.ctypes.data, std.ctypes.data, B, H, W, out)
    return out


def warp_nodes(image_ids, cells, amp256, seed=0):
    """int32 [B, (cells + 1)^2, 2]: the node displacements (dy, dx) in 1/256 pixel of the images image_ids int64 [B] (ppf_warp_nodes)."""
    who = "warp_nodes"
    if not isinstance(image_ids, torch.Tensor) or image_ids.dim() != 1:
        raise ValueError(f"{who}: image_ids must be an int64 CUDA tensor [B]")
    B, s = image_ids.shape[0], int(cells)
    _dev_tensor(who, "image_ids", image_ids, torch.int64, (B,))
    nodes = torch.empty((B, max(s + 1, 0) ** 2, 2), dtype=torch.int32, device=image_ids.device)
    _lib.call("ppf_warp_nodes", image_ids, int(seed) & 0xFFFFFFFFFFFFFFFF, B, s, int(amp256), nodes)
    return nodes


def warp_apply(x, nodes, cells, amp256, out=None):
    """out = x fp32 [B, Cc, H, H] resampled at the positions the node table warp_nodes wrote displaces its pixels to (ppf_warp_apply,
    include/ppf_hip.h); one launch."""
    who = "warp_apply"
    out = _image_batch(who, x, out, channels=None)
    B, Cc, H, W = x.shape
    _dev_tensor(who, "nodes", nodes, torch.int32, (B, (int(cells) + 1) ** 2, 2), x.device)
    _lib.call("ppf_warp_apply", x, nodes, int(cells), int(amp256), B, Cc, H, W, out)
    return out


def because_score(act_max, protos, grid_cells=0, *, act_full=None, idx=None, cells=None):
    """(same, best fp32 [B, K], lost int32 [B, K]) of a perturbed forward's act_max fp32 [B, P], act_full fp32 [B, P, T] and idx int32
    [B, T] for the rows protos / cells int32 [B, K] (ppf_because_score, include/ppf_hip.h); one launch.  idx None: the global branch,
    (None, best, None)."""
    who = "because_score"
    if not isinstance(act_max, torch.Tensor) or act_max.dim() != 2 or not isinstance(protos, torch.Tensor) or protos.dim() != 2:
        raise ValueError(f"{who}: act_max must be an fp32 CUDA tensor [B, P] and protos an int32 CUDA tensor [B, K]")
    (B, P), K, dev = act_max.shape, protos.shape[1], act_max.device
    _dev_tensor(who, "act_max", act_max, torch.float32, (B, P))
    _dev_tensor(who, "protos", protos, torch.int32, (B, K), dev)
    best = torch.empty((B, K), dtype=torch.float32, device=dev)
    if idx is None:
        _lib.call("ppf_because_score", None, None, act_max, protos, None, B, P, 0, 0, K, None, best, None)
        return None, best, None
    T = idx.shape[1] if isinstance(idx, torch.Tensor) and idx.dim() == 2 else -1
    _dev_tensor(who, "idx", idx, torch.int32, (B, T), dev)
    if not isinstance(act_full, torch.Tensor) or act_full.numel() != B * P * T:
        raise ValueError(f"{who}: act_full must hold [{B}, {P}, {T}] elements")
    _dev_tensor(who, "act_full", act_full, torch.float32, act_full.shape, dev)
    _dev_tensor(who, "cells", cells, torch.int32, (B, K), dev)
    same, lost = torch.empty_like(best), torch.empty((B, K), dtype=torch.int32, device=dev)
    _lib.call("ppf_because_score", act_full, idx, act_max, protos, cells, B, P, T, int(grid_cells), K, same, best, lost)
    return same, best, lost


# ---- integrated gradients (csrc/ig.hip): the path point, the weighted gradient sum, attribution and its cell sums
def _ig_baseline(who, baseline, like):
    if isinstance(baseline, torch.Tensor):
        return _dev_tensor(who, "baseline", baseline, torch.float32, like.shape, like.device), 0.0
    return None, float(baseline)


def ig_point(x, alpha, baseline=0.0, out=None):
    """out = baseline + alpha * (x - baseline), every operation rounded once (ppf_ig_point, include/ppf_hip.h); one launch.  x: an fp32
    CUDA tensor of any shape; baseline: a number, or an fp32 tensor like x; out: an fp32 tensor like x to write into."""
    who = "ig_point"
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"{who}: x must be an fp32 CUDA tensor")
    _dev_tensor(who, "x", x, torch.float32, x.shape)
    base_t, base_c = _ig_baseline(who, baseline, x)
    if out is None:
        out = torch.empty_like(x)
    else:
        _dev_tensor(who, "out", out, torch.float32, x.shape, x.device)
    _lib.call("ppf_ig_point", x, base_t, base_c, float(alpha), x.numel(), out)
    return out


def ig_accumulate(g, w, acc, first=False):
    """acc (+)= w * g IN PLACE (ppf_ig_accumulate, include/ppf_hip.h); one launch.  g fp32 [R, ...] contiguous; acc: an fp32 tensor of g's
    shape whose rows acc[r] are contiguous and lie acc.stride(0) >= g[0].numel() elements apart -- a contiguous tensor, or one class
    column acc_all[:, m] of a [B, M, ...] accumulator.  first=True writes w * g without reading acc.  Returns acc."""
    who = "ig_accumulate"
    if not isinstance(g, torch.Tensor) or g.dim() < 1:
        raise ValueError(f"{who}: g must be an fp32 CUDA tensor [R, ...]")
    _dev_tensor(who, "g", g, torch.float32, g.shape)
    if not isinstance(acc, torch.Tensor) or not acc.is_cuda or acc.device != g.device or acc.dtype != torch.float32 or acc.shape != g.shape:
        raise ValueError(f"{who}: acc must be an fp32 CUDA tensor {list(g.shape)} on {g.device}")
    R = g.shape[0]
    n = g.numel() // R if R else 0
    stride = acc.stride(0) if R > 1 else n
    if R and (not acc[0].is_contiguous() or stride < n):
        raise ValueError(f"{who}: the rows of acc must be contiguous and at least {n} elements apart, got strides {tuple(acc.stride())}")
    _lib.call("ppf_ig_accumulate", g, float(w), int(bool(first)), R, n, acc, stride)
    return acc


def ig_finish(acc, x, baseline, patch):
    """(attr fp32 [B, M, C, H, W], cell64 fp64 [B, M, G]) from the averaged gradients acc fp32 [B, M, C, H, W] and x fp32 [B, C, H, W]:
    attr = (x - baseline) * acc and its fp64 sum over every patch x patch cell and the channels, G = (H / patch) * (W / patch), cells
    row-major (ppf_ig_finish, include/ppf_hip.h); one launch, one pass."""
    who = "ig_finish"
    if not isinstance(acc, torch.Tensor) or acc.dim() != 5:
        raise ValueError(f"{who}: acc must be an fp32 CUDA tensor [B, M, C, H, W]")
    _dev_tensor(who, "acc", acc, torch.float32, acc.shape)
    B, M, C, H, W = acc.shape
    _dev_tensor(who, "x", x, torch.float32, (B, C, H, W), acc.device)
    base_t, base_c = _ig_baseline(who, baseline, x)
    patch = int(patch)
    G = (H // patch) * (W // patch) if patch > 0 else 0
    attr = torch.empty_like(acc)
    cell64 = torch.empty((B, M, G), dtype=torch.float64, device=acc.device)
    _lib.call("ppf_ig_finish", acc, x, base_t, base_c, B, M, C, H, W, patch, attr, cell64)
    return attr, cell64


# ---- spatial alignment (csrc/alignment.hip): the image gradient's last step, gradient mass inside a box, the attack's step
def col2im_patch(cols, B, C, H, W, patch):
    """img fp32 [B, C, H, W] from cols fp32 [B*(H/patch)*(W/patch), C*patch*patch]: the inverse of im2col_patch / im2col_patch_f32
    (ppf_col2im_patch_f32); one launch, every element written once."""
    who = "col2im_patch"
    B, C, H, W, patch = int(B), int(C), int(H), int(W), int(patch)
    if min(B, C, H, W, patch) < 1 or H % patch or W % patch:
        raise ValueError(f"{who}: bad shape B={B} C={C} H={H} W={W} patch={patch} (patch must divide H and W)")
    _dev_tensor(who, "cols", cols, torch.float32, (B * (H // patch) * (W // patch), C * patch * patch))
    img = torch.empty((B, C, H, W), dtype=torch.float32, device=cols.device)
    _lib.call("ppf_col2im_patch_f32", cols, img, B, C, H, W, patch)
    return img


def _rows_and_boxes(who, name, t, box):
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{who}: {name} must be an fp32 CUDA tensor [R, C, H, W]")
    _dev_tensor(who, name, t, torch.float32, t.shape)
    _dev_tensor(who, "box", box, torch.int32, (t.shape[0], 4), t.device)
    return tuple(t.shape)


def grad_box_mass(g, box, want_nonfinite=True):
    """(inside fp64 [R], total fp64 [R], nonfinite int32 [R] or None) of g fp32 [R, C, H, W] and box int32 [R, 4] = (y0, y1, x0, x1),
    half-open (ppf_grad_box_mass): sums of |g|, non-finite elements left out and counted; one launch, fixed order."""
    who = "grad_box_mass"
    R, C, H, W = _rows_and_boxes(who, "g", g, box)
    inside = torch.empty(R, dtype=torch.float64, device=g.device)
    total = torch.empty_like(inside)
    bad = torch.empty(R, dtype=torch.int32, device=g.device) if want_nonfinite else None
    if R > 0:
        _lib.call("ppf_grad_box_mass", g, box, R, C, H, W, inside, total, bad)
    return inside, total, bad


def pgd_step_box(x, x0, g, box, alpha, eps, lo, hi, direction):
    """One projected signed-gradient step on x fp32 [R, C, H, W] IN PLACE outside box int32 [R, 4]; inside it x <- x0 (ppf_pgd_step_box).
    alpha / eps / lo / hi: fp32 device tensors [C]; direction +1 or -1.  Returns x."""
    who = "pgd_step_box"
    R, C, H, W = _rows_and_boxes(who, "x", x, box)
    for name, t in (("x0", x0), ("g", g)):
        _dev_tensor(who, name, t, torch.float32, x.shape, x.device)
    for name, t in (("alpha", alpha), ("eps", eps), ("lo", lo), ("hi", hi)):
        _dev_tensor(who, name, t, torch.float32, (C,), x.device)
    if direction not in (1, -1):
        raise ValueError(f"{who}: direction must be +1 or -1, got {direction!r}")
    if R > 0:
        _lib.call("ppf_pgd_step_box", x, x0, g, box, alpha, eps, lo, hi, float(direction), R, C, H, W)
    return x


# ---- interpretability post-processing (csrc/interp.hip): activation maps [M, g, g] fp32 -> S x S, bit-identical to interpret.resize_cubic
def _act_maps(name, grids, size):
    """(M, g, S) of the maps handed to a ppf_act_* entry point.  What the C side cannot see -- layout and dtype -- is refused here with
    the library's own shape error (the message form of _lib.call for PPF_ERR_SHAPE), before anything is launched."""
    def bad(why):
        return RuntimeError(f"{name} failed (rc={_lib.DEFINES['PPF_ERR_SHAPE']}): {name}: {why}")
    if not isinstance(grids, torch.Tensor) or not grids.is_cuda:
        raise bad("the maps must be a CUDA tensor (there is no host path here: interpret.resize_cubic is the host function)")
    if grids.dtype != torch.float32:
        raise bad(f"the maps must be fp32, got {grids.dtype}")
    if grids.dim() != 3 or grids.shape[1] != grids.shape[2]:
        raise bad(f"the maps must be [M, g, g], got {tuple(grids.shape)}")
    if not grids.is_contiguous():
        raise bad(f"the maps must be contiguous, got strides {tuple(grids.stride())}")
    if int(size) != size:
        raise bad(f"the output size must be an integer, got {size!r}")
    return grids.shape[0], grids.shape[1], int(size)


def act_upsample(grids, size):
    """[M, g, g] fp32 -> [M, size, size] fp32 (ppf_act_upsample)."""
    M, g, S = _act_maps("ppf_act_upsample", grids, size)
    out = torch.empty((M, max(S, 0), max(S, 0)), dtype=torch.float32, device=grids.device)
    if M > 0:
        _lib.call("ppf_act_upsample", grids, out, M, g, S)
    return out


def act_peak(grids, size, parts=None, half_size=0):
    """Peak of every up-sampled map without writing it (ppf_act_peak): (values [M] fp32, yx [M, 2] int32, table).  parts [M_img, n_parts, 3]
    int32 (valid, x, y) with M a multiple of M_img: the same launch also fills table [M, n_parts] uint8 (else None)."""
    M, g, S = _act_maps("ppf_act_peak", grids, size)
    val = torch.empty(M, dtype=torch.float32, device=grids.device)
    yx = torch.empty((M, 2), dtype=torch.int32, device=grids.device)
    table, per, n_parts = None, 0, 0
    if parts is not None:
        n_parts, per = _act_parts("ppf_act_peak", parts, M)
        table = torch.empty((M, n_parts), dtype=torch.uint8, device=grids.device)
    if M > 0:
        _lib.call("ppf_act_peak", grids, M, g, S, val, yx, parts, per, n_parts, int(half_size), table)
    return val, yx, table


def _act_parts(name, parts, M):
    if parts.dtype != torch.int32 or parts.dim() != 3 or parts.shape[2] != 3 or not parts.is_contiguous() or not parts.is_cuda:
        raise ValueError(f"{name}: parts must be a contiguous int32 CUDA tensor [M_img, n_parts, 3] of (valid, x, y)")
    if parts.shape[0] == 0 or M % parts.shape[0] != 0:
        raise ValueError(f"{name}: {M} maps do not divide over {parts.shape[0]} images")
    return parts.shape[1], M // parts.shape[0]


def act_part_table(yx, size, parts, half_size):
    """[M, n_parts] uint8 table of prototype_part_table from given peaks yx [M, 2] int32 (ppf_act_part_table)."""
    _chk(yx, torch.int32)
    M = yx.shape[0]
    n_parts, per = _act_parts("ppf_act_part_table", parts, M)
    table = torch.empty((M, n_parts), dtype=torch.uint8, device=yx.device)
    _lib.call("ppf_act_part_table", yx, M, int(size), parts, per, n_parts, int(half_size), table)
    return table


def act_order_stats(grids, size, k_lo, k_hi):
    """[M, 2] fp32: the values of ascending 0-based ranks k_lo, k_hi (k_hi - k_lo in {0, 1}) of every up-sampled map (ppf_act_order_stats)."""
    M, g, S = _act_maps("ppf_act_order_stats", grids, size)
    stats = torch.empty((M, 2), dtype=torch.float32, device=grids.device)
    if M > 0:
        _lib.call("ppf_act_order_stats", grids, M, g, S, int(k_lo), int(k_hi), stats)
    return stats


def act_box(grids, size, thr):
    """[M, 4] int32 (y0, y1, x0, x1) of up >= thr[m]; thr fp64 [M] on the device (ppf_act_box)."""
    M, g, S = _act_maps("ppf_act_box", grids, size)
    _chk(thr, torch.float64)
    if thr.shape != (M,):
        raise ValueError(f"act_box: one fp64 threshold per map expected, got {tuple(thr.shape)} for {M} maps")
    box = torch.empty((M, 4), dtype=torch.int32, device=grids.device)
    if M > 0:
        _lib.call("ppf_act_box", grids, thr, M, g, S, box)
    return box


# ---- foreground focus (csrc/interp.hip, csrc/explain.hip): maps, boxes, reserved tokens and evidence against an object box per image
def _obj_boxes(who, obj, rows, device):
    """obj int32 [B, 4] on `device` with `rows` a multiple of B >= 1: returns rows per image."""
    if not isinstance(obj, torch.Tensor) or obj.dim() != 2:
        raise ValueError(f"{who}: obj must be an int32 CUDA tensor [B, 4] of (y0, y1, x0, x1)")
    _dev_tensor(who, "obj", obj, torch.int32, (obj.shape[0], 4), device)
    if obj.shape[0] == 0 or rows % obj.shape[0] != 0:
        raise ValueError(f"{who}: {rows} rows do not divide over {obj.shape[0]} object boxes")
    return rows // obj.shape[0]


def act_focus(grids, size, obj, want_nonfinite=True):
    """Peak and positive mass of every up-sampled map against its image's object box, without writing the map (ppf_act_focus): dict of
    peak_val [M] fp32, peak_yx [M, 2] int32 (both as act_peak), hit [M] int32, inside / total [M] fp64, nonfinite [M] int32 or None.
    grids [M, g, g] fp32; obj [M_img, 4] int32 (y0, y1, x0, x1), half-open, with M a multiple of M_img.  One launch."""
    M, g, S = _act_maps("ppf_act_focus", grids, size)
    dev = grids.device
    out = dict(peak_val=torch.empty(M, dtype=torch.float32, device=dev), peak_yx=torch.empty((M, 2), dtype=torch.int32, device=dev),
               hit=torch.empty(M, dtype=torch.int32, device=dev), inside=torch.empty(M, dtype=torch.float64, device=dev),
               total=torch.empty(M, dtype=torch.float64, device=dev),
               nonfinite=torch.empty(M, dtype=torch.int32, device=dev) if want_nonfinite else None)
    if M > 0:
        per = _obj_boxes("act_focus", obj, M, dev)
        _lib.call("ppf_act_focus", grids, obj, M, g, S, per, out["peak_val"], out["peak_yx"], out["hit"], out["inside"], out["total"], out["nonfinite"])
    return out


def focus_box_terms(box, obj, size):
    """terms int32 [M, 4] = (intersection, box, object, union) areas of box [M, 4] (as act_box returns it) against obj [M_img, 4], both
    clipped to the size x size image (ppf_focus_box_terms)."""
    who = "focus_box_terms"
    if not isinstance(box, torch.Tensor) or box.dim() != 2:
        raise ValueError(f"{who}: box must be an int32 CUDA tensor [M, 4]")
    _dev_tensor(who, "box", box, torch.int32, (box.shape[0], 4))
    M = box.shape[0]
    terms = torch.empty((M, 4), dtype=torch.int32, device=box.device)
    if M > 0:
        per = _obj_boxes(who, obj, M, box.device)
        _lib.call("ppf_focus_box_terms", box, obj, M, per, int(size), terms)
    return terms


def reserve_focus(idx, obj, grid_side, patch, token_attn=None):
    """(out int32 [B, 4], attn fp64 [B, 2] or None) of the reserved cells idx int32 [B, T] against obj int32 [B, 4] on the grid_side x
    grid_side grid of patch x patch pixel cells (ppf_reserve_focus): out = (reserved pixels inside, reserved cells with centre inside, all
    cells with centre inside, valid idx entries); with token_attn fp32 [B, grid_side^2] also the rollout score over the cells with centre
    inside and over all cells."""
    who = "reserve_focus"
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2:
        raise ValueError(f"{who}: idx must be an int32 CUDA tensor [B, T]")
    B, T = idx.shape
    g, patch = int(grid_side), int(patch)
    _dev_tensor(who, "idx", idx, torch.int32, (B, T))
    _dev_tensor(who, "obj", obj, torch.int32, (B, 4), idx.device)
    out = torch.empty((B, 4), dtype=torch.int32, device=idx.device)
    attn = None
    if token_attn is not None:
        _dev_tensor(who, "token_attn", token_attn, torch.float32, (B, g * g), idx.device)
        attn = torch.empty((B, 2), dtype=torch.float64, device=idx.device)
    if B > 0:
        _lib.call("ppf_reserve_focus", idx, obj, token_attn, B, T, g, patch, out, attn)
    return out, attn


def evidence_focus(act_max, weight, scale, ppc, classes, obj, grid_side, patch, *, idx, argmax=None):
    """(ev fp64 [B, M, 4], cnt int32 [B, M, 4]) of the local branch's evidence for classes int32 [B, M] against obj int32 [B, 4]
    (ppf_evidence_focus): the sums and term counts over (own class & cell centre inside, own & not, other classes & inside, other & not).
    act_max [B, P] fp32, argmax [B, P] int32 or None (k = 1: every cell is idx[b][0]), idx [B, T] int32, weight [C, P] fp32."""
    who = "evidence_focus"
    if not isinstance(act_max, torch.Tensor) or act_max.dim() != 2 or not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise ValueError(f"{who}: act_max must be [B, P] and weight [C, P]")
    B, P = act_max.shape
    C, dev = weight.shape[0], act_max.device
    _dev_tensor(who, "act_max", act_max, torch.float32, (B, P))
    _dev_tensor(who, "weight", weight, torch.float32, (C, P), dev)
    if not isinstance(idx, torch.Tensor) or idx.dim() != 2:
        raise ValueError(f"{who}: idx must be an int32 CUDA tensor [B, T]")
    T = idx.shape[1]
    _dev_tensor(who, "idx", idx, torch.int32, (B, T), dev)
    if argmax is not None:
        _dev_tensor(who, "argmax", argmax, torch.int32, (B, P), dev)
    if not isinstance(classes, torch.Tensor) or classes.dim() != 2:
        raise ValueError(f"{who}: classes must be an int32 CUDA tensor [B, M]")
    M = classes.shape[1]
    _dev_tensor(who, "classes", classes, torch.int32, (B, M), dev)
    _dev_tensor(who, "obj", obj, torch.int32, (B, 4), dev)
    ev = torch.empty((B, M, 4), dtype=torch.float64, device=dev)
    cnt = torch.empty((B, M, 4), dtype=torch.int32, device=dev)
    if B > 0:
        _lib.call("ppf_evidence_focus", act_max, argmax, idx, T, weight, float(scale), int(ppc), classes, obj, int(grid_side), int(patch), B, P, C, M, ev, cnt)
    return ev, cnt


# ---- stability score (csrc/interp.hip): per-image Gaussian input noise and the per-class accumulators of interpret.PartMeter
def add_gauss_noise(x, image_ids, sigma, seed=0, out=None):
    """x + sigma * N(0, 1) on an fp32 CUDA batch [B, ...] (ppf_add_gauss_noise): the noise of an image is a function of (seed, its id in
    image_ids int64 [B], element) alone.  out: None (a new tensor), x itself (in place) or another tensor like x."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() < 1 or not x.is_contiguous():
        raise ValueError("add_gauss_noise: x must be a contiguous fp32 CUDA tensor [B, ...]")
    if (not isinstance(image_ids, torch.Tensor) or image_ids.dtype != torch.int64 or image_ids.shape != (x.shape[0],) or not image_ids.is_contiguous()
            or image_ids.device != x.device):
        raise ValueError(f"add_gauss_noise: image_ids must be a contiguous int64 tensor [{x.shape[0]}] on {x.device}")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("add_gauss_noise: out must be a contiguous tensor of x's shape, dtype and device")
    B = x.shape[0]
    n_per_img = 1
    for d in x.shape[1:]:
        n_per_img *= int(d)
    _lib.call("ppf_add_gauss_noise", x, out, B, n_per_img, image_ids, float(sigma), int(seed) & 0xFFFFFFFFFFFFFFFF)
    return out


def part_meter_update(tables, tables_noisy, parts, labels, hits, visible, stable, images, bad):
    """Add one batch into the int32 accumulators hits [C, ppc, n_parts], visible [C, n_parts], stable [C, ppc], images [C], bad [1]
    (ppf_part_meter_update, include/ppf_hip.h); launches only.  tables / tables_noisy (or None) uint8 [B, ppc, n_parts], parts int32
    [B, n_parts, 3], labels int64 [B]."""
    if not isinstance(tables, torch.Tensor) or tables.dtype != torch.uint8 or tables.dim() != 3 or not tables.is_contiguous() or not tables.is_cuda:
        raise ValueError("part_meter_update: tables must be a contiguous uint8 CUDA tensor [B, ppc, n_parts]")
    B, ppc, n_parts = tables.shape
    dev = tables.device
    if tables_noisy is not None and (tables_noisy.dtype != torch.uint8 or tables_noisy.shape != tables.shape or not tables_noisy.is_contiguous()
                                     or tables_noisy.device != dev):
        raise ValueError(f"part_meter_update: tables_noisy must be None or a contiguous uint8 tensor {tuple(tables.shape)} on {dev}")
    if parts.dtype != torch.int32 or parts.shape != (B, n_parts, 3) or not parts.is_contiguous() or parts.device != dev:
        raise ValueError(f"part_meter_update: parts must be a contiguous int32 tensor [{B}, {n_parts}, 3] on {dev}")
    if labels.dtype != torch.int64 or labels.shape != (B,) or not labels.is_contiguous() or labels.device != dev:
        raise ValueError(f"part_meter_update: labels must be a contiguous int64 tensor [{B}] on {dev}")
    C = images.shape[0] if images.dim() == 1 else -1
    for name, t, shape in (("hits", hits, (C, ppc, n_parts)), ("visible", visible, (C, n_parts)), ("stable", stable, (C, ppc)), ("images", images, (C,)),
                           ("bad", bad, (1,))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"part_meter_update: {name} must be a contiguous int32 tensor {shape} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    if B > 0:
        _lib.call("ppf_part_meter_update", tables, tables_noisy, parts, labels, B, ppc, n_parts, C, hits, visible, stable, images, bad)


MIX_WORDS, MIX_WSELF = _lib.DEFINES["PPF_MIX_WORDS"], _lib.DEFINES["PPF_MIX_WSELF"]          # read from include/ppf_hip.h


def mixup_apply(x, table_host, table_dev):
    """In-place Mixup / CutMix of x [B, C, H, W] fp32 by the per-sample table (pinned host int32 [B, MIX_WORDS]; uploaded to table_dev)."""
    B, Cc, H, W = x.shape
    _lib.call("ppf_mixup_apply", x, table_host, table_dev, B, Cc, H, W)


def mixup_target(label, table_dev, num_classes, off_value, on_value):
    """timm mixup_target on the weights of the uploaded mixing table: [B, num_classes] fp32."""
    B = label.shape[0]
    t = torch.empty((B, num_classes), dtype=torch.float32, device=label.device)
    _lib.call("ppf_mixup_target", label, table_dev.data_ptr() + 4 * MIX_WSELF, MIX_WORDS, float(off_value), float(on_value), t, B, num_classes)
    return t


SYNTH_WORDS = _lib.DEFINES["PPF_SYNTH_WORDS"]                                                     # read from include/ppf_hip.h


def _synth_words(spec):
    """(C, K, D, H, W, g, noise, seed) of a data.PartsWorldSpec as the entry points take them."""
    return (int(spec.classes), int(spec.parts), int(spec.distractors), int(spec.height), int(spec.width), int(spec.grid), int(spec.noise),
            int(spec.seed) & 0xFFFFFFFFFFFFFFFF)


def synth_scene(spec, ids):
    """The scene table int32 [B, SYNTH_WORDS] of image ids int64 [B] under a data.PartsWorldSpec (ppf_synth_scene, include/ppf_hip.h);
    one launch."""
    who = "synth_scene"
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
        raise ValueError(f"{who}: ids must be an int64 CUDA tensor [B]")
    B = ids.shape[0]
    _dev_tensor(who, "ids", ids, torch.int64, (B,))
    C, K, D, H, W, g, noise, seed = _synth_words(spec)
    scene = torch.empty((B, SYNTH_WORDS), dtype=torch.int32, device=ids.device)
    _lib.call("ppf_synth_scene", scene, ids, B, C, K, D, H, W, g, noise, seed)
    return scene


def synth_render(spec, scene, ids, out=None, partmap=False):
    """The frames uint8 [B, H, W, 3] of a scene table (ppf_synth_render, include/ppf_hip.h); one launch.  out: a contiguous uint8 CUDA
    tensor of B * H * W * 3 elements to render into (a slice of a DeviceDataset's flat buffer), any shape; None: a new [B, H, W, 3].
    partmap: True for a new uint8 [B, H, W], or a tensor of B * H * W elements.  Returns out, or (out, partmap)."""
    who = "synth_render"
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1:
        raise ValueError(f"{who}: ids must be an int64 CUDA tensor [B]")
    B = ids.shape[0]
    _dev_tensor(who, "ids", ids, torch.int64, (B,))
    _dev_tensor(who, "scene", scene, torch.int32, (B, SYNTH_WORDS), ids.device)
    C, K, D, H, W, g, noise, seed = _synth_words(spec)

    def buffer(name, t, shape):
        n = 1
        for s in shape:
            n *= s
        if t is None:
            return torch.empty(shape, dtype=torch.uint8, device=ids.device)
        if not isinstance(t, torch.Tensor) or t.dim() < 1:
            raise ValueError(f"{who}: {name} must be a uint8 CUDA tensor of {n} elements")
        return _dev_tensor(who, name, t, torch.uint8, t.shape if t.numel() == n else shape, ids.device)
    out = buffer("out", out, (B, H, W, 3))
    pm = None if partmap is False or partmap is None else buffer("partmap", None if partmap is True else partmap, (B, H, W))
    _lib.call("ppf_synth_render", out, pm, scene, ids, B, H, W, C, K, D, g, noise, seed)
    return out if pm is None else (out, pm)


def synth_edit(spec, scene, edits, out=None, check=True):
    """(out int32 [B, E, SYNTH_WORDS], changed int32 [B, E]) of a scene table int32 [B, SYNTH_WORDS] and edits int32 [B, E, 2] = (op, arg)
    (ppf_synth_edit, include/ppf_hip.h); one launch.  out: an int32 CUDA tensor of B * E * SYNTH_WORDS elements to write into, or None.
    check: read `changed` back (the one read) and raise on any -1, naming the first invalid edit; False: no read, the -1 stays in
    `changed` for the caller.  A chain of edits is a sequence of calls with out[:, e] as the next scene."""
    who = "synth_edit"
    if not isinstance(scene, torch.Tensor) or scene.dim() != 2 or not isinstance(edits, torch.Tensor) or edits.dim() != 3:
        raise ValueError(f"{who}: scene must be an int32 CUDA tensor [B, {SYNTH_WORDS}] and edits one of [B, E, 2]")
    B, E = scene.shape[0], edits.shape[1]
    _dev_tensor(who, "scene", scene, torch.int32, (B, SYNTH_WORDS))
    _dev_tensor(who, "edits", edits, torch.int32, (B, E, 2), scene.device)
    C, K, D, _, _, g, _, _ = _synth_words(spec)
    if out is None:
        out = torch.empty((B, E, SYNTH_WORDS), dtype=torch.int32, device=scene.device)
    elif not isinstance(out, torch.Tensor) or out.numel() != B * E * SYNTH_WORDS:
        raise ValueError(f"{who}: out must be an int32 CUDA tensor of {B * E * SYNTH_WORDS} elements")
    else:
        _dev_tensor(who, "out", out, torch.int32, out.shape, scene.device)
    changed = torch.empty((B, E), dtype=torch.int32, device=scene.device)
    _lib.call("ppf_synth_edit", out, changed, scene, edits, B, E, C, K, D, g)
    if check:
        bad = (changed.cpu() < 0).nonzero()
        if len(bad):
            b, e = (int(v) for v in bad[0])
            raise ValueError(f"{who}: {len(bad)} invalid edits, the first is edit {e} of image {b}: (op, arg) = {tuple(edits[b, e].tolist())} "
                             f"with K={K} parts and D={D} distractors (unknown op, a mask bit or k out of range, attr >= 24, or a colour above 0xFFFFFF)")
    return out.view(B, E, SYNTH_WORDS), changed


def part_mass(score, partmap, rows_per_img, K, want_nonfinite=True):
    """(pos fp64 [R, 3 + K], neg fp64 [R, 3 + K], count int32 [R, 3 + K], nonfinite int32 [R] or None) of score fp32 [R, S, S] and
    partmap uint8 [R / rows_per_img, H, W] (ppf_part_mass, include/ppf_hip.h): the positive and the negative mass of every row on
    each primitive code, seen through the view rule; one launch, fixed order."""
    who = "part_mass"
    if not isinstance(score, torch.Tensor) or score.dim() != 3 or score.shape[1] != score.shape[2]:
        raise ValueError(f"{who}: score must be an fp32 CUDA tensor [R, S, S]")
    if not isinstance(partmap, torch.Tensor) or partmap.dim() != 3:
        raise ValueError(f"{who}: partmap must be a uint8 CUDA tensor [R / rows_per_img, H, W]")
    R, S = int(score.shape[0]), int(score.shape[1])
    rows_per_img, K = int(rows_per_img), int(K)
    _dev_tensor(who, "score", score, torch.float32, score.shape)
    nb = max(3 + K, 1)
    pos = torch.empty((R, nb), dtype=torch.float64, device=score.device)
    neg = torch.empty_like(pos)
    count = torch.empty((R, nb), dtype=torch.int32, device=score.device)
    bad = torch.empty(R, dtype=torch.int32, device=score.device) if want_nonfinite else None
    if rows_per_img >= 1 and R % rows_per_img == 0:                        # anything else is the library's to refuse by name
        _dev_tensor(who, "partmap", partmap, torch.uint8, (R // rows_per_img,) + tuple(partmap.shape[1:]), score.device)
    _lib.call("ppf_part_mass", score, partmap, R, rows_per_img, S, int(partmap.shape[1]), int(partmap.shape[2]), K, pos, neg, count, bad)
    return pos, neg, count, bad


def sgemm(a, b, out, M, N, K, sam, sak, sbn, sbk, alpha=1.0, beta=0.0):
    ws = _workspace(out.device, 16 * M * N * 4)
    _lib.call("ppf_sgemm", a, b, out, M, N, K, sam, sak, sbn, sbk, out.shape[-1], float(alpha), float(beta), ws, ws.numel() // 4)
    return out


def sgemm_pair(a0, b0, out0, N0, K0, sa0, sb0, alpha0, a1, b1, out1, N1, K1, sa1, sb1, alpha1, M, total=None, c0=0.0, c1=0.0):
    """out_i = alpha_i A_i B_i^T (i = 0, 1) and total = c0 A0 B0^T + c1 A1 B1^T in one launch + one reduction; sa_i = (row stride, k stride)
    of A_i, sb_i = (row stride, k stride) of B_i (B_i indexed [n, k])."""
    nfl = _lib.lib().ppf_sgemm_pair_workspace(M, N0, K0, N1, K1)
    ws = _workspace(a0.device, nfl * 4)
    _lib.call("ppf_sgemm_pair", a0, b0, out0, N0, K0, sa0[0], sa0[1], sb0[0], sb0[1], out0.shape[-1] if out0 is not None else 0, float(alpha0),
              a1, b1, out1, N1, K1, sa1[0], sa1[1], sb1[0], sb1[1], out1.shape[-1] if out1 is not None else 0, float(alpha1),
              total, total.shape[-1] if total is not None else 0, float(c0), float(c1), M, ws, ws.numel() // 4)


def axpbypcz(x, y, z, a, b, c):
    out = torch.empty_like(x)
    _lib.call("ppf_axpbypcz", x, y, z, out, float(a), float(b), float(c), x.numel())
    return out


_CONST = {}


def const_scalar(device, value):
    """A cached one-element fp32 device tensor (never written): seed / fixed coefficients of the loss backward without a fill launch."""
    key = (device, float(value))
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((), float(value), dtype=torch.float32, device=device)
    return t


def is_const_one(t):
    c = _CONST.get((t.device, 1.0))
    return c is not None and t.data_ptr() == c.data_ptr()


def axpby(x, y, a, b, out=None):
    if out is None:
        out = torch.empty_like(x)
    _lib.call("ppf_axpby", x, y, out, float(a), float(b), x.numel())
    return out


def topk_sorted(scores, k):
    """Ascending indices (int32) of the k largest entries of each row of scores [B, n<=256]."""
    _chk(scores, torch.float32)
    B, n = scores.shape
    idx = torch.empty((B, k), dtype=torch.int32, device=scores.device)
    _lib.call("ppf_topk_sorted", scores, B, n, k, idx)
    return idx


def sigmoid_bwd(df, f, dbias):
    rows, cols = f.shape
    dz = torch.empty((rows, cols), dtype=torch.bfloat16, device=f.device)
    part = torch.empty(_lib.lib().ppf_sigmoid_bwd_blocks(rows) * cols, dtype=torch.float32, device=f.device) if dbias is not None else None
    _lib.call("ppf_sigmoid_bwd", df, f, dz, dbias, rows, cols, part, part.numel() * 4 if part is not None else 0)
    return dz


# ------------------------------------------------------------------------------------------------ plumbing kernels
def zeros(shape, dtype, device):
    """torch.zeros on the library's own memset node (keeps a captured step free of ATen fill kernels)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    _lib.call("ppf_memset_zero", t, t.numel() * t.element_size())
    return t


def zero_(t):
    _lib.call("ppf_memset_zero", t, t.numel() * t.element_size())
    return t


def copy_2d(dst, src):
    """dst[...] = src[...] for 2-D views (rows, cols) whose rows are contiguous: strided sub-matrix copy on the library's launch path
    (recordable; replaces torch.cat / slice.contiguous() / slice.copy_ in the CaiT class-attention stage)."""
    assert dst.dim() == 2 and src.dim() == 2 and dst.shape == src.shape and dst.stride(1) == 1 and src.stride(1) == 1 and dst.dtype == src.dtype
    es = dst.element_size()
    _lib.call("ppf_copy_2d", dst, dst.stride(0) * es, src, src.stride(0) * es, dst.shape[1] * es, dst.shape[0])
    return dst


def cat_rows(first, rest):
    """torch.cat([first [B,1,D], rest [B,N,D]], dim=1) -> [B, 1+N, D] with two strided copies."""
    B, N, D = rest.shape
    out = torch.empty((B, N + 1, D), dtype=rest.dtype, device=rest.device)
    o2 = out.reshape(B, (N + 1) * D)
    copy_2d(o2[:, :D], first.reshape(B, D))
    copy_2d(o2[:, D:], rest.reshape(B, N * D))
    return out


def reserved_rows_map(idx, N):
    """Flat source rows [B*(1+k)] int32 of [cls, 1+idx...] in the [B*N] token matrix."""
    B, k = idx.shape
    rows = torch.empty(B * (k + 1), dtype=torch.int32, device=idx.device)
    _lib.call("ppf_reserved_rows_map", idx, rows, B, k, N)
    return rows


def gather_rows(src, rows):
    """dst[r] = src[rows[r]] for a 2-D contiguous src."""
    _chk(src)
    dst = torch.empty((rows.numel(), src.shape[1]), dtype=src.dtype, device=src.device)
    _lib.call("ppf_gather_rows", src, rows, dst, rows.numel(), src.shape[1] * src.element_size())
    return dst


def scatter_rows(src, rows, nrows_dst):
    """zeros(nrows_dst, D) with dst[rows[r]] = src[r]."""
    _chk(src)
    dst = torch.empty((nrows_dst, src.shape[1]), dtype=src.dtype, device=src.device)
    _lib.call("ppf_scatter_rows", src, rows, dst, src.shape[0], nrows_dst, src.shape[1] * src.element_size())
    return dst


def droppath_draw(out, keep, seed, state):
    """out [nslot, B] <- floor(keep + U)/keep; advances the device-resident step counter `state` (int64[1])."""
    nslot, B = out.shape
    _lib.call("ppf_droppath_scales", out, keep, nslot, B, int(seed) & 0xFFFFFFFFFFFFFFFF, state)
    return out


def scale_by_scalar(x, scalar):
    out = torch.empty_like(x)
    _lib.call("ppf_scale_by_scalar", x, scalar, out, x.numel())
    return out


# ------------------------------------------------------------------------------------------------ CaiT
def th_fused_ok(H, N, D):
    """The talking-heads kernels th_fwd / th_bwd (csrc/cait.hip) cover this (heads, tokens, width)."""
    return bool(_lib.lib().ppf_th_fused_supported(H, N, D))


def th_fwd(qkv, wl, bl, ww, bw, hm_out, B, H, N, D):
    """cait:119-128 in one launch: returns (a16 bf16 [B,H,N,NPK] = proj_w(softmax(proj_l(scale q k^T))), rowmax, zinv [B,H,N], out);
    hm_out [B,N,NP] receives the head mean of the mixed probabilities (rollout input); out = a16 @ v as bf16 [B*N, D]."""
    NP, NPK = (N + 3) // 4 * 4, (N + 7) // 8 * 8
    a16 = torch.empty((B, H, N, NPK), dtype=torch.bfloat16, device=qkv.device)
    rowmax = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
    zinv = torch.empty_like(rowmax)
    out = torch.empty((B * N, D), dtype=torch.bfloat16, device=qkv.device)
    _lib.call("ppf_th_fwd", qkv, wl, bl, ww, bw, a16, hm_out, rowmax, zinv, out, B, H, N, D, NP, NPK)
    return a16, rowmax, zinv, out


def th_bwd(qkv, dout, wl, bl, ww, rowmax, zinv, B, H, N, D):
    """Backward of th_fwd up to dS: returns (ds16 bf16 [B,H,N,NPK], partial) -- partial holds the per-workgroup parameter-gradient
    sums for th_param_reduce."""
    NPK = (N + 7) // 8 * 8
    ds16 = torch.empty((B, H, N, NPK), dtype=torch.bfloat16, device=qkv.device)
    partial = torch.empty((int(_lib.lib().ppf_th_bwd_partial_floats(B, H, N)),), dtype=torch.float32, device=qkv.device)
    _lib.call("ppf_th_bwd", qkv, dout, wl, bl, ww, rowmax, zinv, ds16, partial, B, H, N, D, NPK)
    return ds16, partial


def th_grads_ok(H, N, D):
    """th_grads, and with it training, covers this (heads, tokens, width)."""
    return bool(_lib.lib().ppf_th_grads_supported(H, N, D))


def th_grads(qkv, dout, ds16, a16, dqkv, B, H, N, D):
    """dqkv bf16 [B*N, 3D] <- dQ | dK | dV of the talking-heads attention from dS (th_bwd), A (th_fwd), q / k (packed qkv) and dO: one launch."""
    _lib.call("ppf_th_grads", qkv, dout, ds16, a16, dqkv, B, H, N, D, a16.shape[-1])
    return dqkv


def th_param_reduce(partial, B, H, N, dww, dbw, dbl, dwl):
    _lib.call("ppf_th_param_reduce", partial, B, H, N, dww, dbw, dbl, dwl)


def class_attn_fwd(q, k, v, policy, B, H, N1, D, rowmean=None):
    dev = q.device
    attn = torch.empty((B, H, N1), dtype=torch.float32, device=dev)
    zinv = torch.empty((B, H), dtype=torch.float32, device=dev)
    if rowmean is None:
        rowmean = torch.empty((B, N1), dtype=torch.float32, device=dev)
    out = torch.empty((B, D), dtype=torch.bfloat16, device=dev)
    _lib.call("ppf_class_attn_fwd", q, k, v, policy, attn, zinv, rowmean, out, B, H, N1, D)
    return out, attn, zinv, rowmean


def class_attn_bwd(q, k, v, attn, zinv, dout, B, H, N1, D):
    dq = torch.empty_like(q)
    dk = torch.empty_like(k)
    dv = torch.empty_like(v)
    _lib.call("ppf_class_attn_bwd", q, k, v, attn, zinv, dout, dq, dk, dv, B, H, N1, D)
    return dq, dk, dv


def merge3_cast(a, b, cq, N1):
    rows, D = a.shape
    out = torch.empty((rows, D), dtype=torch.bfloat16, device=a.device)
    _lib.call("ppf_merge3_cast", a, b, cq, out, rows, D, N1)
    return out


# ------------------------------------------------------------------------------------------------ fp32 verification path
def linear_f32(x, w, bias=None, kind=0, res=None, rowscale=None, rows_per_group=1, colscale=None):
    """fp32 y = epilogue(x W^T + b) through ppf_sgemm (fp32 FMA) + ppf_epilogue_f32.  x [M,K] (row stride may exceed K), w [N,K]."""
    M, K = x.shape
    N = w.shape[0]
    w2 = w.reshape(N, -1)
    assert w2.shape[1] == K and w2.is_contiguous() and x.stride(1) == 1
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    ws = _workspace(x.device, 16 * M * N * 4) if M * N <= (1 << 22) else None
    _lib.call("ppf_sgemm", x, w2, out, M, N, K, x.stride(0), 1, K, 1, N, 1.0, 0.0, ws, ws.numel() // 4 if ws is not None else 0)
    _lib.call("ppf_epilogue_f32", out, bias, kind, res, rowscale, rows_per_group, colscale, M, N)
    return out


def layernorm_fwd_f32(x, w, b, eps=1e-6, row_map=None):
    D = x.shape[-1]
    rows = row_map.numel() if row_map is not None else x.numel() // D
    y = torch.empty((rows, D), dtype=torch.float32, device=x.device)
    _lib.call("ppf_layernorm_fwd_f32", x, row_map, w, b, y, rows, D, float(eps))
    return y


def im2col_patch_f32(img, patch):
    B, C, H, W = img.shape
    cols = torch.empty((B * (H // patch) * (W // patch), C * patch * patch), dtype=torch.float32, device=img.device)
    _lib.call("ppf_im2col_patch_f32", img, cols, B, C, H, W, patch)
    return cols


def attn_fwd_f32(qkv, B, H, N, D, policy=None, self_keep=True, headmean=None, eps_n=0):
    out = torch.empty((B * N, D), dtype=torch.float32, device=qkv.device)
    NP = headmean.shape[-1] if headmean is not None else 0
    _lib.call("ppf_attn_fwd_f32", qkv, out, policy, headmean, NP, B, H, N, D, int(self_keep), int(eps_n))
    return out


def th_attn_fwd_f32(qkv, wl, bl, ww, bw, B, H, N, D, headmean):
    out = torch.empty((B * N, D), dtype=torch.float32, device=qkv.device)
    _lib.call("ppf_th_attn_fwd_f32", qkv, wl, bl, ww, bw, out, headmean, headmean.shape[-1], B, H, N, D)
    return out


def class_attn_fwd_f32(q, k, v, policy, B, H, N1, D):
    out = torch.empty((B, D), dtype=torch.float32, device=q.device)
    attn_mean = torch.empty((B, N1), dtype=torch.float32, device=q.device)
    _lib.call("ppf_class_attn_fwd_f32", q, k, v, policy, attn_mean, out, B, H, N1, D)
    return out, attn_mean


# ------------------------------------------------------------------------------------------------ fp32 verification mode: backward pieces
def layernorm_bwd_f32(dy, x, w, dw, db, dx_out, dres_in=None, row_map=None, eps=1e-6):
    """dx_out[xrow] = (dres_in[xrow] or 0) + LN'(dy); dw / db += (fp32 atomics); rows of dy <-> rows row_map[r] of x (None: identity)."""
    rows, D = dy.shape
    _lib.call("ppf_layernorm_bwd_f32", dy, x, row_map, w, dres_in, dx_out, dw, db, rows, D, float(eps))
    return dx_out


def ew_bwd_f32(kind, a, b=None, rowscale=None, rows_per_group=1):
    """kind 0: a * gelu'(b) | 1: a * b * (1 - b) | 2: a * rowscale[row // rows_per_group] (rowscale None: copy) | 3: a * b |
    4: a * rowscale[..] * b[col] (b a LayerScale vector) | 5: a where b > 0 else 0 (ReLU', b = the ReLU's output)."""
    M, N = a.shape
    out = torch.empty_like(a)
    _lib.call("ppf_ew_bwd_f32", int(kind), a, b, out, rowscale, rows_per_group, M, N)
    return out


def colsum_f32(x, out):
    """out[n] += sum_m x[m, n]."""
    M, N = x.shape
    _lib.call("ppf_colsum_f32", x, out, M, N)


def attn_bwd_f32(qkv, dout, B, H, N, D, policy=None, self_keep=True, eps_n=0):
    dqkv = torch.empty_like(qkv)
    scratch = torch.empty(B * H * 2 * N * N, dtype=torch.float32, device=qkv.device)
    _lib.call("ppf_attn_bwd_f32", qkv, dout, policy, dqkv, scratch, B, H, N, D, int(self_keep), int(eps_n))
    return dqkv


def linear_dgrad_f32(dy, w):
    """dx [M, K] = dy [M, N] @ w [N, K] through ppf_sgemm (fp32 FMA)."""
    M, N = dy.shape
    w2 = w.reshape(N, -1)
    K = w2.shape[1]
    out = torch.empty((M, K), dtype=torch.float32, device=dy.device)
    return sgemm(dy, w2, out, M, K, N, N, 1, 1, K)


def linear_wgrad_f32(dy, x, gw, gb=None):
    """gw [N, K] += dy [M, N]^T @ x [M, K] (and gb [N] += column sums of dy) through ppf_sgemm, accumulating into the flat gradient views."""
    M, N = dy.shape
    K = x.shape[1]
    sgemm(dy, x, gw.reshape(N, K), N, K, M, 1, N, 1, K, alpha=1.0, beta=1.0)
    if gb is not None:
        colsum_f32(dy, gb)


def th_attn_bwd_f32(qkv, dout, mix, gmix, B, H, N, D):
    """mix = (wl, bl, ww, bw) of the talking-heads mixers, gmix their gradient views (accumulated)."""
    dqkv = zeros(qkv.shape, torch.float32, qkv.device)
    _lib.call("ppf_th_attn_bwd_f32", qkv, dout, mix[0], mix[1], mix[2], mix[3], dqkv, gmix[0], gmix[1], gmix[2], gmix[3], B, H, N, D)
    return dqkv


def class_attn_bwd_f32(q, k, v, policy, dout, B, H, N1, D):
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _lib.call("ppf_class_attn_bwd_f32", q, k, v, policy, dout, dq, dk, dv, B, H, N1, D)
    return dq, dk, dv


def relu_f32_(x):
    """in place max(x, 0) on an fp32 [M, N] matrix."""
    M, N = x.shape
    _lib.call("ppf_epilogue_f32", x, None, 4, None, None, 1, None, M, N)
    return x

